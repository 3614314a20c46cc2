"""The host side of the one-call native forwards (impls/ep_native.py) without a GPU: what `forward`, `forward_from_logits` and
`forward_packed` hand to tutel_amd_ep_forward, tutel_amd_moe_forward, tutel_amd_moe_forward_packed and _glu.

The four entry points are replaced by a recorder (a proxy in front of the loaded library: everything else, the plans included, is
the real code), the layers and tensors live on the CPU, ops._stream answers 0 and pin_memory is the identity.  The recorder dumps
every struct it is handed -- integers verbatim, pointers as null / "<tensor name>+<byte offset>" / "fresh" for a per-call output --
plus the workspace's buffers (name, shape, dtype, which names share storage) and what the forward left on the layer.  The dumps
are compared, field for field, with tests/golden/native_args.json, which was recorded from the tree BEFORE the host side was
written once (three copies of the workspace / binding code then): a refactor of that code has to hand the library the same
arguments, oddities included (the packed calls carry row_align 0 where the padded ones carry 1).

    python tests/test_native_args_cpu.py --record     rewrites the golden file from the tree at hand
    python tests/test_native_args_cpu.py --time       per-call host cost of two forwards with the recorder answering at once
"""
import collections
import ctypes
import functools
import json
import os
import sys
import time
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_args.json")
FORWARDS = ("tutel_amd_ep_forward", "tutel_amd_moe_forward", "tutel_amd_moe_forward_packed", "tutel_amd_moe_forward_packed_glu")
ZERO_ROW_ARG = {"tutel_amd_expert_gemm_gather": 4, "tutel_amd_expert_ffn": 5}   # position of the zero row in ops.py's two users
FRESH = ("y", "dispatch_count", "l_aux", "logits_out")   # per-call outputs: allocated by the forward, named by the field
SEGMENT_PTR, SEGMENT_HANDLE = 0x7000_0000_0000, 0x5E6
T, T2, M, H, E, K = 512, 300, 256, 256, 8, 2


def _nbytes(t):
    return t.numel() * t.element_size()


class Recorder:
    """in front of the loaded library: records (and answers) the four forwards, counts every call by name, forwards the rest"""

    def __init__(self, real):
        self._real = real
        self.calls, self.counts, self.zero_rows = [], collections.Counter(), {}
        self.layer, self.named, self.answers, self.quiet = None, {}, [], False

    def __getattr__(self, name):
        if name in FORWARDS:
            return functools.partial(self._forward, name)
        if name in ZERO_ROW_ARG:
            return functools.partial(self._zero_row_user, name)
        fn = getattr(self._real, name)

        def counted(*args):
            self.counts[name] += 1
            return fn(*args)
        return counted

    def _zero_row_user(self, name, *args):
        self.zero_rows[name] = args[ZERO_ROW_ARG[name]]
        return 0

    # ---- names of the addresses a forward may pass ----------------------------------------------------------------------
    def _workspace(self):
        cache = self.layer.__dict__.get("_ep_workspaces")
        return next(reversed(cache.values())) if cache else None   # the one this call found or made: most recently used

    @staticmethod
    def _buffers(ws):
        out = {}
        for name, v in sorted(vars(ws).items()):
            if isinstance(v, torch.Tensor):
                out[name] = v
            elif name == "bufs":
                out.update({"bufs." + n: t for n, t in v.items()})
        return out

    def _registry(self, ws):
        ex = self.layer.experts
        reg = dict(self.named)
        reg.update({"experts." + n: p for n, p in ex.named_parameters()})
        reg.update({"kmajor." + n: hit[1] for n, hit in ex._kmajor._store.items()})
        if isinstance(getattr(self.layer, "dispatch_count", None), torch.Tensor):
            reg["layer.dispatch_count"] = self.layer.dispatch_count
        reg.update({"ws." + n: t for n, t in self._buffers(ws).items()})
        ranges = [(n, t.data_ptr(), t.data_ptr() + _nbytes(t)) for n, t in reg.items() if t.device.type == "cpu" and t.numel()]
        if getattr(ws, "segment", None) is not None:
            ranges.append(("segment", ws.segment.ptr, ws.segment.ptr + ws.segment.nbytes))
        return ranges

    @staticmethod
    def _name(ptr, ranges, fresh, field):
        if not ptr:
            return None
        if field in FRESH:
            return "fresh"
        if field == "peer_seg":
            return "segment.handle" if ptr == SEGMENT_HANDLE else "unknown"
        for name, lo, hi in ranges:   # (first match: a parameter before its views, an input before a workspace)
            if lo <= ptr < hi:
                return "%s+%d" % (name, ptr - lo)
        for name, p in fresh.items():
            if p == ptr:
                return "fresh:" + name
        return "unknown"

    def _fresh(self, struct, fresh):
        """the per-call outputs of this call, by field name (row_counts may name one of them)"""
        for field, _ in struct._fields_:
            v = getattr(struct, field)
            if isinstance(v, ctypes.Structure):
                self._fresh(v, fresh)
            elif field in FRESH and v:
                fresh[field] = v
        return fresh

    def _dump(self, struct, ranges, fresh):
        out = {}
        for field, ctype in struct._fields_:
            v = getattr(struct, field)
            if isinstance(v, ctypes.Structure):
                out[field] = self._dump(v, ranges, fresh)
            elif ctype is ctypes.c_void_p:
                out[field] = self._name(v, ranges, fresh, field)
            elif isinstance(v, ctypes._Pointer):
                out[field] = self._name(ctypes.cast(v, ctypes.c_void_p).value, ranges, fresh, field)
            else:
                out[field] = int(v)
        return out

    def _forward(self, name, comm, *rest):
        rc = self.answers.pop(0) if self.answers else 0
        structs = [r._obj for r in rest if hasattr(r, "_obj")]
        if isinstance(rc, tuple):    # (status, capacity the call reads back through capacity_out before it answers)
            rc, cap = rc
            structs[0].capacity_out[0] = cap
        if self.quiet:
            return rc
        ws = self._workspace()
        ranges, fresh = self._registry(ws), {}
        for st in structs:
            self._fresh(st, fresh)
        rec = {"entry": name, "comm": comm, "stream": rest[-1], "answer": rc,
               "structs": [self._dump(s, ranges, fresh) for s in structs]}
        if name.endswith("_glu"):
            rec["w_up"] = self._name(rest[-2], ranges, fresh, "w_up")
        bufs = self._buffers(ws)
        rec["workspace"] = {"class": type(ws).__name__, "T_cap": getattr(ws, "T_cap", None), "C_cap": getattr(ws, "C_cap", None),
                            "buffers": {n: [list(t.shape), str(t.dtype)] for n, t in bufs.items()}}
        groups = collections.defaultdict(list)
        for n, t in bufs.items():
            groups[t.untyped_storage().data_ptr()].append(n)
        rec["workspace"]["shared"] = sorted(sorted(g) for g in groups.values() if len(g) > 1)
        self.calls.append(rec)
        return rc


@pytest.fixture
def rec(monkeypatch):
    from tutel_amd import _lib, ops
    _lib.build()
    real = _lib.lib()
    r = Recorder(real)
    monkeypatch.setattr(_lib, "_lib", r)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_dev", lambda *a: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)
    yield r


def _layer(kind="ffn", hidden=H, **kw):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 0.0},
                              experts={"type": kind, "num_experts_per_device": E, "hidden_size_per_expert": hidden}, model_dim=M, **kw)
    finally:
        torch.set_default_dtype(old)
    return layer.eval()


def _inputs(Tn, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn([Tn, M], generator=g).to(torch.bfloat16)
    logits = torch.randn([Tn, E], generator=g).to(torch.bfloat16)
    return x, logits


def _left_on_layer(layer, stream=0):
    def key(k):
        return [["<stream>" if type(e) is int and e == stream else str(e) for e in part] if isinstance(part, tuple) else part for part in k]
    d = layer.__dict__
    return {"protected_shape": list(d["protected_shape"]) if d.get("protected_shape") is not None else None,
            "set": sorted(n for n in ("dropless_offsets", "dropless_capacity", "last_routing") if d.get(n) is not None),
            "dropless_cap": sorted([str(k), v] for k, v in d.get("_ep_dropless_cap", {}).items()),
            "workspaces": [key(k) for k in d.get("_ep_workspaces", {})],
            "allocations": d.get("_ep_workspace_allocations", 0)}


def _plan(Tn, capacity, seed):
    """a hand-made RoutingPlan: the arrays only have to exist (nothing reads them here)"""
    from tutel_amd.impls.fast_dispatch import RoutingPlan
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, E, [K, Tn], generator=g, dtype=torch.int32)
    loc = torch.randint(0, capacity, [K, Tn], generator=g, dtype=torch.int32)
    gates = torch.rand([K, Tn], generator=g).to(torch.bfloat16)
    smap = torch.full([E * capacity], -1, dtype=torch.int32)
    return RoutingPlan(E, idx, loc, gates, capacity, torch.zeros([E], dtype=torch.int32), slot_map=smap)


class _FakeComm:
    handle, world, rank, generic = None, 2, 0, True

    def __init__(self, ipc):
        self.ipc, self.asked = ipc, []

    def segment(self, key, nbytes):
        self.asked.append([[str(e) for e in key], int(nbytes)])
        return types.SimpleNamespace(ptr=SEGMENT_PTR, handle=SEGMENT_HANDLE, nbytes=int(nbytes))


# ---- the cases: name -> function(rec) that runs the forwards and returns what else is to be compared ------------------------
def _ep_case(rec, monkeypatch=None, postscore=True, mega=0, comm=None):
    from tutel_amd.impls import ep_native
    layer = _layer()
    layer.is_postscore = postscore
    if mega:
        layer.megablocks_size = mega
        layer.dispatch_count = torch.zeros([E], dtype=torch.int32)
    if comm is not None:
        layer.world_size = 2
        monkeypatch.setattr(ep_native, "communicator", lambda group, device: comm)
    rec.layer, out = layer, []
    for i, Tn in enumerate((T, T2)):
        x, _ = _inputs(Tn, i)
        crit = _plan(Tn, 128, i)
        rec.named = {"x": x, "crit.idx2d": crit.idx2d, "crit.loc2d": crit.loc2d, "crit.gates2d": crit.gates2d, "crit.slot_map": crit.slot_map}
        y = ep_native.forward(layer, x, crit, 2 if comm is not None else 1)
        out.append({"y": [list(y.shape), str(y.dtype)], "layer": _left_on_layer(layer)})
    if comm is not None:
        out.append({"segments_asked": comm.asked})
    return out


def _moe_case(rec, gate=False, mega=0, dropless=None, answers=(), capacity=128, keep=False):
    from tutel_amd.impls import ep_native
    layer = _layer()
    layer._keep_routing = keep
    rec.layer, out = layer, []
    for i, Tn in enumerate((T, T2)):
        x, logits = _inputs(Tn, i)
        gate_w = layer.gates[0].wg.weight if gate else None
        rec.named = {"x": x, "logits": logits, "gate_w": gate_w} if gate else {"x": x, "logits": logits}
        rec.answers = list(answers) if i == 0 else []
        res = ep_native.forward_from_logits(layer, x, logits.to("meta") if gate else logits, K, capacity, 1, True, True, dropless=dropless,
                                            megablocks_size=mega, gate_w=gate_w)
        y, l_aux, cnt, used = res
        out.append({"y": [list(y.shape), str(y.dtype)], "l_aux": list(l_aux.shape), "cnt": [list(cnt.shape), str(cnt.dtype)], "used": used,
                    "layer": _left_on_layer(layer)})
    return out


def _packed_case(rec, kind="ffn", hidden=H, gate=False, limit=lambda Tn: 0, alignment=1, keep=False):
    from tutel_amd.impls import ep_native
    layer = _layer(kind, hidden)
    layer._keep_routing = keep
    rec.layer, out = layer, []
    for i, Tn in enumerate((T, T2)):
        x, logits = _inputs(Tn, i)
        gate_w = layer.gates[0].wg.weight if gate else None
        rec.named = {"x": x, "logits": logits, "gate_w": gate_w} if gate else {"x": x, "logits": logits}
        with torch.no_grad():
            res = ep_native.forward_packed(layer, x, logits.to("meta") if gate else logits, K, True, limit(Tn), alignment, gate_w=gate_w)
        if res is None:
            out.append({"result": None, "layer": _left_on_layer(layer)})
            continue
        y, l_aux, cnt, cap = res
        ws = next(reversed(layer._ep_workspaces.values()))
        out.append({"y": [list(y.shape), str(y.dtype)], "l_aux": list(l_aux.shape), "cnt": [list(cnt.shape), str(cnt.dtype)],
                    "capacity_is_the_workspace's": cap is ws.capacity, "offsets_are_the_workspace's": layer.dropless_offsets is ws.offsets,
                    "layer": _left_on_layer(layer)})
    return out


def _eagain():
    from tutel_amd import _lib
    return [(_lib.EAGAIN, 300)]


CASES = {
    "ep/fused_encode": lambda rec, mp: _ep_case(rec),
    "ep/prescore_aliased_stages": lambda rec, mp: _ep_case(rec, postscore=False),
    "ep/megablocks_8": lambda rec, mp: _ep_case(rec, mega=8),
    "ep/comm_rccl": lambda rec, mp: _ep_case(rec, mp, comm=_FakeComm(False)),
    "ep/comm_ipc": lambda rec, mp: _ep_case(rec, mp, comm=_FakeComm(True)),
    "moe/static_capacity": lambda rec, mp: _moe_case(rec),
    "moe/gate_w": lambda rec, mp: _moe_case(rec, gate=True, keep=True),
    "moe/megablocks_8": lambda rec, mp: _moe_case(rec, mega=8, dropless=(0, 1)),
    "moe/dropless_eagain_once": lambda rec, mp: _moe_case(rec, dropless=(0, 1), answers=_eagain(), capacity=192),
    "packed/ffn_align1_nolimit": lambda rec, mp: _packed_case(rec),
    "packed/ffn_align4_limit": lambda rec, mp: _packed_case(rec, limit=lambda Tn: K * int(1.5 * ((Tn + E - 1) // E)), alignment=4, keep=True),
    "packed/gate_w": lambda rec, mp: _packed_case(rec, gate=True),
    "packed/llama_ffn_glu": lambda rec, mp: _packed_case(rec, kind="llama_ffn"),
    "packed/refused_H64": lambda rec, mp: _packed_case(rec, hidden=64),
}


def _run(name, rec, monkeypatch):
    rec.calls.clear()
    extra = CASES[name](rec, monkeypatch)
    return json.loads(json.dumps({"calls": rec.calls, "results": extra}))   # (through JSON: tuples become lists, as in the file)


def _diff(a, b, path=""):
    """the paths at which two JSON values differ (for a readable failure)"""
    if type(a) is not type(b):
        return ["%s: %r != %r" % (path, a, b)]
    if isinstance(a, dict):
        return [d for k in sorted(set(a) | set(b))
                for d in (_diff(a[k], b[k], path + "/" + k) if k in a and k in b else [path + "/" + k + ": on one side only"])]
    if isinstance(a, list):
        if len(a) != len(b):
            return ["%s: %d entries != %d" % (path, len(a), len(b))]
        return [d for i, (u, v) in enumerate(zip(a, b)) for d in _diff(u, v, "%s[%d]" % (path, i))]
    return [] if a == b else ["%s: %r != %r" % (path, a, b)]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_hands_the_library_the_recorded_arguments(name, rec, monkeypatch):
    want = json.load(open(GOLDEN))[name]
    got = _run(name, rec, monkeypatch)
    assert "unknown" not in json.dumps(got), "a pointer the recorder cannot name"
    if name == "packed/refused_H64":
        assert got["calls"] == [] and all(r["result"] is None for r in got["results"])
    else:
        assert len(got["calls"]) == (3 if name == "moe/dropless_eagain_once" else 2)
    assert _diff(want, got) == []


def _plans(rec, layer, x, logits, cf):
    before = rec.counts["tutel_amd_packed_plan"]
    with torch.no_grad():
        res = layer._run_native_moe(x, logits, K, cf, 1, 1, 0)
    return rec.counts["tutel_amd_packed_plan"] - before, res


def test_run_native_moe_plans_the_packed_forward_once(rec):
    """MOELayer._run_native_moe with dropless_packed on: ONE Python call of tutel_amd_packed_plan per forward (it used to be three:
    packed_unsupported in the layer, again in forward_packed, then the plan itself), a forward that allocates its workspace
    included when its token count is the bucket.  Only a forward that allocates a workspace for a LARGER bucket asks a second
    question, the plan of T_cap tokens, once per allocation."""
    layer = _layer()
    layer.dropless_packed = True
    rec.layer, rec.quiet = layer, True
    for Tn, cf in ((T, 0.0), (T2, 0.0), (T, -1.5)):
        x, logits = _inputs(Tn, 0)
        made = layer.__dict__.get("_ep_workspace_allocations", 0)
        n, res = _plans(rec, layer, x, logits, cf)
        assert res is not None and layer._dropless_packed_ran is True
        assert n == 1   # (512 is its own bucket; 300 finds the workspace of 512)
        made = layer._ep_workspace_allocations
        assert _plans(rec, layer, x, logits, cf)[0] == 1 and layer._ep_workspace_allocations == made   # the workspace is there
    other = _layer()   # T = 300 first: the workspace is made for the bucket of 512 tokens, whose plan is a second question
    other.dropless_packed = True
    rec.layer = other
    assert _plans(rec, other, *_inputs(T2, 0), 0.0)[0] == 2 and other._ep_workspace_allocations == 1
    assert _plans(rec, other, *_inputs(T2, 0), 0.0)[0] == 1
    # a layer the plan refuses: one call still, the reason handed on, the padded one-call path taken
    small = _layer(hidden=64)
    small.dropless_packed = True
    rec.layer = small
    n, res = _plans(rec, small, x, logits, 0.0)
    assert n == 1 and res is not None and "H and M_out" in small._dropless_packed_ran


def test_the_four_zero_row_users_share_one_row(rec):
    """the padded fused-encode workspace, the packed workspace, ops.expert_gemm_gather and ops.expert_ffn hand the library the row
    of ops.zero_row for their (device, dtype): one cache, no second one in ep_native"""
    from tutel_amd import ops
    from tutel_amd.impls import ep_native
    x, _ = _inputs(T, 0)
    _ep_case(rec)
    padded = next(reversed(rec.layer._ep_workspaces.values())).args.zero_row
    _packed_case(rec)
    packed = next(reversed(rec.layer._ep_workspaces.values())).margs.ep.zero_row
    smap = torch.full([E * 128], -1, dtype=torch.int32)
    w1, w2k = torch.zeros([E, H, M], dtype=torch.bfloat16), torch.zeros([E, M, H], dtype=torch.bfloat16)
    ops.expert_gemm_gather(x, smap, w1, None, True, "relu", 128)
    ops.expert_ffn(x, w1, None, w2k, None, "relu", R=128, smap=smap)
    z = ops.zero_row(M, torch.bfloat16, x.device)
    assert z.numel() >= 8192 and z.dtype == torch.bfloat16 and not z.any()
    assert [padded, packed, rec.zero_rows["tutel_amd_expert_gemm_gather"], rec.zero_rows["tutel_amd_expert_ffn"]] == [z.data_ptr()] * 4
    assert not hasattr(ep_native, "_zero_rows")
    assert ops.zero_row(M, torch.bfloat16, x.device) is z
    assert ops.zero_row(9000, torch.bfloat16, x.device).numel() >= 9000    # too short: replaced by a longer one


# ---- stand-alone: record the golden file / time the host side ----------------------------------------------------------------
class _Patch:
    """pytest's monkeypatch, as far as this file uses it, for the two stand-alone modes"""

    def __init__(self):
        self.undo_list = []

    def setattr(self, obj, name, value):
        self.undo_list.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, old in reversed(self.undo_list):
            setattr(obj, name, old)


def _standalone():
    from tutel_amd import _lib, ops
    _lib.build()
    mp = _Patch()
    r = Recorder(_lib.lib())
    mp.setattr(_lib, "_lib", r)
    mp.setattr(ops, "_stream", lambda: 0)
    mp.setattr(ops, "_dev", lambda *a: None)
    mp.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)
    return r, mp


def host_cost(calls=2000, repeats=3):
    """seconds per call of forward_from_logits (static capacity) and forward_packed (ffn), the recorder answering 0 at once:
    the Python cost of the host side alone (no GPU, no kernel)"""
    from tutel_amd.impls import ep_native
    r, mp = _standalone()
    r.quiet = True
    out = {}
    try:
        layer = _layer()
        x, logits = _inputs(T, 0)
        r.layer = layer
        runs = {"forward_from_logits": lambda: ep_native.forward_from_logits(layer, x, logits, K, 128, 1, True, True),
                "forward_packed": lambda: ep_native.forward_packed(layer, x, logits, K, True, 0, 1)}
        with torch.no_grad():
            for name, fn in runs.items():
                fn()
                out[name] = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        fn()
                    out[name].append((time.perf_counter() - t0) / calls)
    finally:
        mp.undo()
    return out


if __name__ == "__main__":
    if "--record" in sys.argv:
        r, mp = _standalone()
        gold = {}
        for name in CASES:
            inner = _Patch()
            gold[name] = _run(name, r, inner)
            inner.undo()
        mp.undo()
        assert "unknown" not in json.dumps(gold)
        json.dump(gold, open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("recorded", len(gold), "cases,", sum(len(g["calls"]) for g in gold.values()), "calls ->", GOLDEN)
    if "--time" in sys.argv:
        for name, ts in host_cost().items():
            print("%s: per call %s us, median %.2f us, spread %.2f us" % (name, ", ".join("%.2f" % (t * 1e6) for t in ts),
                                                                       sorted(ts)[1] * 1e6, (max(ts) - min(ts)) * 1e6))
