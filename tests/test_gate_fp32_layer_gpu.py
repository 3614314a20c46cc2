"""An fp32 gate (fp32_gate=True) over bf16 / fp16 experts with the projection INSIDE the native call (switch
impls/moe_layer.py::_NATIVE_GATE_FP32, off by default, set here with monkeypatch): the headline shape against the reference's
routing, every route the projection reaches against the same layer run through ops.gate_logits + the logits-given call (bit for
bit) and against the switch-off forward (same routing), and the layers that must keep F.linear."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL            # noqa: E402
import test_swiglu_packed_gpu as TS    # noqa: E402

pytestmark = pytest.mark.gpu

F32 = 0
FORWARDS = ("tutel_amd_moe_forward", "tutel_amd_moe_forward_packed", "tutel_amd_moe_forward_packed_glu")
T, M, H, E, K, SEED = 300, 256, 256, 8, 2, 4   # ragged T across four 64-token tiles; SEED: see _problem
DTYPES = [torch.bfloat16, torch.float16]
_dt = dict(ids=lambda d: str(d).split(".")[-1])


class Spy:
    """in front of the loaded library (as tests/test_native_args_cpu.py::Recorder, but every call goes through): counts the calls
    by name and notes, per one-call forward, where its logits come from"""

    def __init__(self, real):
        self._real, self.counts, self.forwards = real, collections.Counter(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args):
            self.counts[name] += 1
            if name in FORWARDS:
                m = args[1]._obj
                self.forwards.append(dict(entry=name, in_call=bool(m.gate_w) and not m.logits, logits_dtype=int(m.logits_dtype),
                                          dtype=int(m.ep.dtype)))
            return fn(*args)
        return counted

    def mixed(self):
        """one-call forwards that projected an fp32 gate over 16-bit tokens themselves"""
        return [f for f in self.forwards if f["in_call"] and f["logits_dtype"] == F32 and f["dtype"] != F32]


@pytest.fixture
def spy(monkeypatch):
    from tutel_amd import _lib
    s = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", s)
    return s


@pytest.fixture
def linear_calls(monkeypatch):
    calls, real = [], torch.nn.functional.linear

    def linear(inp, weight, bias=None):
        calls.append((tuple(inp.shape), inp.dtype, weight.dtype))
        return real(inp, weight, bias)
    monkeypatch.setattr(torch.nn.functional, "linear", linear)
    return calls


def _switch(monkeypatch, on):
    from tutel_amd.impls import moe_layer as ML
    monkeypatch.setattr(ML, "_NATIVE_GATE_FP32", on)


def _gate_projection_launches(fn):
    """launches the library booked under its gate-projection stage while fn() ran"""
    from tutel_amd import ops
    torch.cuda.synchronize()
    ops.stage_report()
    ops.stage_timing(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, ops.stage_report()["gate_projection"][1]
    finally:
        ops.stage_timing(0)


# ---- 5. the headline shape against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_dt)
def test_headline_shape_routes_as_the_reference_with_the_projection_in_the_call(oracle, monkeypatch, spy, linear_calls, dtype):
    """test_layer_gpu.py::test_headline_shape_layer_vs_oracle with the switch on: the reference's own routing of these tokens
    (tests/golden/headline_fp32gate_*.npz; smallest relative gap among a row's three largest scores 4e-5), element by element, and
    no F.linear anywhere in the forward"""
    Th, Mh, Hh, Eh, k = 4096, 2048, 2048, 64, 2
    x, *weights = oracle.make_problem(Th, Mh, Hh, Eh, dtype=dtype, seed=0)
    z = np.load(os.path.join(TL.GOLD, f"headline_fp32gate_{str(dtype).split('.')[-1]}.npz"))
    assert [int(v) for v in z["meta"]] == [Th, Mh, 8, Eh, k, 0]
    assert abs(float(z["in_checksum"][0]) - float(x.double().abs().sum() + weights[0].double().abs().sum())) < 1e-6 * float(z["in_checksum"][0])
    layer = TL.make_layer(Mh, Hh, Eh, k, 1.0, dtype, weights, gate={"fp32_gate": True}).eval()
    assert layer.gates[0].wg.weight.dtype == torch.float32
    layer._keep_routing = True
    _switch(monkeypatch, True)
    xd = x.cuda().view(16, 256, Mh)

    def run():
        with torch.no_grad():
            return layer(xd)
    y, launches = _gate_projection_launches(run)
    assert linear_calls == [], "F.linear ran"
    assert len(spy.forwards) == 1 and len(spy.mixed()) == 1 and spy.forwards[0]["entry"] == "tutel_amd_moe_forward", spy.forwards
    assert launches == 1, "the call launched the projection kernel once"
    assert layer.last_logits.dtype == torch.float32
    idx, loc = layer.last_routing
    assert torch.equal(idx.cpu(), torch.from_numpy(z["idx"])), "expert ids vs the reference, element-wise"
    assert torch.equal(loc.cpu(), torch.from_numpy(z["loc"])), "bucket slots vs the reference, element-wise"
    assert torch.equal(layer.dispatch_count.cpu(), torch.from_numpy(z["dispatch_count"])) and int(z["capacity"][0]) == 128
    assert int(layer.protected_shape[1]) == 128
    assert y.l_aux.dtype == torch.float32 and abs(float(y.l_aux) - float(z["l_aux"][0])) < 1e-5
    yo, lo, crit, _ = oracle.moe_forward(x, *weights, top_k=k, capacity_factor=1.0, fp32_gate=True, accum_fp32=True)
    assert crit[4] == 128 and y.shape == (16, 256, Mh)
    TL._close(y.view(Th, Mh), yo, dtype)
    assert abs(float(y.l_aux) - float(lo)) < 1e-5


# ---- 6. every route, one small shape each --------------------------------------------------------------------------------------
def _problem(dtype, n_experts=E):
    """tokens and an fp32 gate weight, seeded.  SEED was picked on the CPU so that every row's three largest reference-route scores
    (softmax of x.float() @ wg^T in fp32) are at least 1e-4 apart, relatively, in both dtypes: _routing_is_decided asserts it"""
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn([T, M], generator=g).to(dtype)
    wg = torch.randn([n_experts, M], generator=g) / M ** 0.5
    return x, wg


def _routing_is_decided(x, wg, k):
    s = torch.softmax(x.float() @ wg.t(), 1)
    top = s.topk(k + 1, dim=1).values
    gap = (top[:, :-1] - top[:, 1:]) / top[:, :-1]
    undecided = int((gap < 1e-4).any(1).sum())
    assert undecided == 0, f"{undecided} rows with a near-tie among their {k + 1} largest scores would have to be excluded"


def _layer(route, dtype, wg, cf, n_experts=E):
    torch.manual_seed(11)
    if route == "packed_swiglu":
        layer = TS.make_layer(M, H, n_experts, K, cf, dtype, gate={"fp32_gate": True})
    else:
        layer = TL.make_layer(M, H, n_experts, K, cf, dtype, gate={"fp32_gate": True}).eval()
        with torch.no_grad():   # a wider spread than the reference's init: outputs well above the dtype's smallest normals
            layer.experts.batched_fc1_w.normal_(0, M ** -0.5)
            layer.experts.batched_fc2_w.normal_(0, H ** -0.5)
    with torch.no_grad():
        layer.gates[0].wg.weight.copy_(wg)
    assert layer.gates[0].wg.weight.dtype == torch.float32 and next(layer.experts.parameters()).dtype == dtype
    layer.dropless_packed = route.startswith("packed") or route == "graphed_packed"
    return layer


ROUTES = {   # route -> (capacity_factor, entry point of the one-call forward)
    "padded_fused_location": (1.0, "tutel_amd_moe_forward"),
    "padded_location_launch": (1.0, "tutel_amd_moe_forward"),
    "dropless_read_back": (0.0, "tutel_amd_moe_forward"),
    "packed_ffn": (0.0, "tutel_amd_moe_forward_packed"),
    "packed_swiglu": (0.0, "tutel_amd_moe_forward_packed_glu"),
    "graphed_padded": (1.0, "tutel_amd_moe_forward"),
    "graphed_packed": (0.0, "tutel_amd_moe_forward_packed"),
}


@pytest.mark.parametrize("dtype", DTYPES, **_dt)
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_projects_in_the_call(monkeypatch, spy, linear_calls, route, dtype):
    from tutel_amd.impls import ep_native, moe_layer as ML
    from tutel_amd.impls.graph import GraphedForward
    cf, entry = ROUTES[route]
    x, wg = _problem(dtype)
    _routing_is_decided(x, wg, K)
    monkeypatch.setattr(ep_native, "_FUSED_LOCATION", route != "padded_location_launch")
    layer = _layer(route, dtype, wg, cf)
    graphed = route.startswith("graphed")
    layer._keep_routing = not graphed
    xd = x.cuda()

    def eager():
        with torch.no_grad():
            y = layer(xd).clone()
        routing = tuple(t.clone() for t in layer.last_routing) if layer._keep_routing else None
        return y, layer.l_aux.clone(), layer.dispatch_count.clone(), routing

    # switch off: the parent's route, x.float() + an fp32 F.linear, then the logits-given one-call forward
    _switch(monkeypatch, False)
    y_off, l_off, cnt_off, routing_off = eager()
    assert len(linear_calls) == 1 and linear_calls[0][1:] == (torch.float32, torch.float32) and spy.mixed() == []
    assert [f["entry"] for f in spy.forwards] == [entry] and not spy.forwards[0]["in_call"]

    # switch on, but the projection kept out of the call: ops.gate_logits + the logits-given call
    _switch(monkeypatch, True)
    real_run, given = ML.MOELayer._run_native_moe, []

    def logits_given_only(self, x_, logits, *args, gate_w=None, **kw):
        if gate_w is not None:
            return None
        given.append((logits.dtype, logits.device.type))
        return real_run(self, x_, logits, *args, **kw)
    monkeypatch.setattr(ML.MOELayer, "_run_native_moe", logits_given_only)
    del linear_calls[:], spy.forwards[:]
    before = spy.counts["tutel_amd_gate_proj_f32w"]
    y_ref, l_ref, cnt_ref, routing_ref = eager()
    assert given == [(torch.float32, "cuda")] and linear_calls == [] and spy.counts["tutel_amd_gate_proj_f32w"] == before + 1
    assert [f["entry"] for f in spy.forwards] == [entry] and spy.mixed() == []
    monkeypatch.setattr(ML.MOELayer, "_run_native_moe", real_run)

    # switch on: the projection inside the call
    del spy.forwards[:]
    before = spy.counts["tutel_amd_gate_proj_f32w"]
    if graphed:
        kw = dict(capacity_factor=0.0, dropless_packed=True) if cf <= 0 else {}
        g = GraphedForward(layer, xd, **kw)
        assert spy.forwards and all(f["entry"] == entry for f in spy.forwards) and len(spy.mixed()) == len(spy.forwards)
        scratch = torch.randn_like(xd)
        for _ in range(3):
            g(scratch)                       # another batch in between: the replay reads its static input anew
            y_on = g(xd).clone()
            assert torch.equal(y_on, y_ref), "a replay against the eager logits-given forward"
        l_on, cnt_on, routing_on = g.l_aux.clone(), layer.dispatch_count.clone(), None
    else:
        y_on, l_on, cnt_on, routing_on = eager()
        assert [f["entry"] for f in spy.forwards] == [entry] and len(spy.mixed()) == 1
    assert linear_calls == [] and spy.counts["tutel_amd_gate_proj_f32w"] == before, "the projection ran inside the call, not from Python"

    # bit for bit the logits-given forward on ops.gate_logits
    assert torch.equal(y_on, y_ref), float((y_on.float() - y_ref.float()).abs().max())
    assert l_on.dtype == torch.float32 and torch.equal(l_on, l_ref) and torch.equal(cnt_on, cnt_ref)
    if routing_on is not None:
        assert torch.equal(routing_on[0], routing_ref[0]) and torch.equal(routing_on[1], routing_ref[1])
    # the routing of the switch-off forward (no near-tie on any row: _routing_is_decided)
    assert torch.equal(cnt_on, cnt_off) and abs(float(l_on) - float(l_off)) <= 1e-5
    if routing_on is not None:
        assert torch.equal(routing_on[0], routing_off[0]) and torch.equal(routing_on[1], routing_off[1])
    # same routing, gates a few fp32 ulps apart: the outputs agree to the output dtype's rounding
    tol = 2 ** -7 if dtype == torch.bfloat16 else 2 ** -10
    err = (y_on.double() - y_off.double()).abs()
    assert bool((err <= tol * y_off.double().abs() + 1e-3).all()), float(err.max())
    assert bool(torch.isfinite(y_on).all()) and float(y_on.float().abs().max()) > 0.05


# ---- 7. layers that keep F.linear ----------------------------------------------------------------------------------------------
def _cast_gate(layer):
    layer.gates[0].bfloat16()


def _hook_gate(layer):
    layer.gates[0].register_forward_hook(lambda mod, args, out: None)


FALLBACKS = {   # name -> (experts E, what to do to the layer, grad mode, autocast)
    "gate_cast_to_bf16": (E, _cast_gate, False, False),
    "forward_hook_on_the_gate": (E, _hook_gate, False, False),
    "requires_grad_under_grad_mode": (E, None, True, False),
    "autocast": (E, None, False, True),
    "six_experts": (6, None, False, False),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_keep_f_linear(oracle, monkeypatch, spy, linear_calls, case):
    n_experts, prepare, grad, autocast = FALLBACKS[case]
    dtype = torch.bfloat16
    x, wg = _problem(dtype, n_experts)
    layer = _layer("padded", dtype, wg, 1.0, n_experts)
    if prepare is not None:
        prepare(layer)
    assert layer.gates[0].wg.weight.requires_grad
    xd = x.cuda()

    def run():
        with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=dtype, enabled=autocast):
            y = layer(xd)
        return y.detach().clone(), layer.l_aux.detach().clone(), layer.dispatch_count.clone()
    _switch(monkeypatch, False)
    y_off, l_off, cnt_off = run()
    n_off = len(linear_calls)
    assert n_off >= 1
    _switch(monkeypatch, True)
    y_on, l_on, cnt_on = run()
    assert len(linear_calls) == 2 * n_off and spy.mixed() == [] and spy.counts["tutel_amd_gate_proj_f32w"] == 0
    assert torch.equal(y_on, y_off) and torch.equal(l_on, l_off) and torch.equal(cnt_on, cnt_off)
    # and that output is the layer's: the fp32-accumulating oracle on the same weights
    ex = layer.experts
    weights = [t.detach().cpu() for t in (layer.gates[0].wg.weight.float(), ex.batched_fc1_w, ex.batched_fc1_bias, ex.batched_fc2_w,
                                           ex.batched_fc2_bias)]
    yo, lo, crit, _ = oracle.moe_forward(x, weights[0], *[w.to(dtype) for w in weights[1:]], top_k=K, capacity_factor=1.0,
                                         fp32_gate=True, accum_fp32=True)
    TL._close(y_on, yo, dtype)
    assert abs(float(l_on) - float(lo)) < 1e-5 and torch.equal(cnt_on.cpu(), crit[5])
