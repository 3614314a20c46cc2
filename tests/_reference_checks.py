"""Replayable form of the function-level and drop-in-surface checks of tests/golden/make_golden.py --check and of the tutel.net
check of tests/golden/make_golden_ep.py --check.

Each check is written ONCE, as a function of an implementation `impl` that returns named observations; it is run with the
reference (tests/golden/make_golden_checks.py, where the reference tree is present: the observations are stored in
tests/golden/reference_checks.npz) and with this repository's oracle / product (tests/test_reference_checks.py, on any box:
the observations are compared with the stored ones).  An observation is (value, mode):
  "exact"  -- must be the reference's bits (stored as a sha256 of dtype, shape and bytes);
  "host"   -- a reduction or GEMM result: the reference's bits on the host that wrote the fixture; elsewhere ATen may reduce in
              another order, so up to 4 places of the largest element (of the value's dtype) are accepted, with a warning;
  "grad"   -- router / expert gradients, compared as make_golden.py compares them (rtol 1e-5, atol 1e-5 * max(1, |ref|max));
  "close"  -- the load-importance loss, compared as make_golden.py compares it (rtol 1e-6, atol 1e-7);
  "allclose" -- tutel.net gradients, compared as make_golden_ep.py compares them (torch.allclose defaults).
Inputs are seeded; the softmax scores are computed with libm exp and an exactly rounded sum (softmax_rows), so that every host
gets the same bits, and their digests are stored with the fixture."""
import hashlib
import json

import torch

DT = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16, "float16": torch.float16}
SWEEP_SHAPES = [(512, 16, 2, 1.0), (512, 16, 1, 1.0), (4096, 64, 2, 1.0), (512, 16, 2, 0.0),
                (300, 7, 3, 1.5), (512, 16, 2, -0.5), (64, 2, 2, 1.0), (1000, 130, 4, 1.0)]
FULL_LIMIT = 65536   # non-"exact" tensors up to this many elements are stored in full beside their digest


def digest(t):
    t = t.detach().contiguous().cpu()
    raw = t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t
    return hashlib.sha256(f"{t.dtype}|{list(t.shape)}|".encode() + raw.numpy().tobytes()).hexdigest()


def softmax_rows(logits):
    """fp32 softmax of each row, computed so that every host gets the same bits (ATen's and numpy's vectorised exp differ between
    instruction sets): libm exp per element in float64, an exactly rounded row sum (math.fsum), one rounding to fp32"""
    import math
    out = []
    for row in logits.double().tolist():
        m = max(row)
        e = [math.exp(v - m) for v in row]
        s = math.fsum(e)
        out.append([v / s for v in e])
    return torch.tensor(out, dtype=torch.float64).to(torch.float32)


def score_inputs():
    """name -> fp32 softmax scores of seeded logits, the scores the checks route on (their digests are stored with the fixture)"""
    out = {}
    for (T, E, k, _) in SWEEP_SHAPES:
        g = torch.Generator().manual_seed(T + E + k)
        out[f"sweep_{T}_{E}_{k}"] = softmax_rows(torch.randn([T, E], generator=g))
    for name, seed, T, E in (("gate_grad", 9, 200, 6), ("masked", 13, 300, 8), ("losses", 77, 640, 24)):
        g = torch.Generator().manual_seed(seed)
        out[name] = softmax_rows(torch.randn([T, E], generator=g))
    g = torch.Generator().manual_seed(78)
    out["losses_logits_softmax"] = softmax_rows(torch.randn([640, 24], generator=g))
    return out


def function_checks(impl, scores):
    """make_golden.py check_oracle_against_reference: routing, encode / decode, cumsum, gate_grad, masked dispatcher, losses.
    `impl` has route(scores, k, cf, norm) -> (crit, l_aux), encode, decode, cumsum_sub_one, gate_grad, dispatch(E, C, M, idx, loc,
    gates, post, x) -> (encoded, decoded), gshard_loss, load_importance_loss."""
    obs = {}
    for dts, dtype in DT.items():
        for (T, E, k, cf) in SWEEP_SHAPES:
            g = torch.Generator().manual_seed(T + E + k)
            torch.randn([T, E], generator=g)              # (the raw logits: the scores themselves come from `scores`)
            sc = scores[f"sweep_{T}_{E}_{k}"].to(dtype)
            for norm in (True, False):
                crit, l_aux = impl.route(sc, k, cf, norm)
                tag = f"{dts} T={T} E={E} k={k} cf={cf} norm={norm}"
                obs["topk indices " + tag] = (torch.stack([i.long() for i in crit[1]]), "exact")
                obs["locations " + tag] = (torch.stack([i.long() for i in crit[2]]), "exact")
                obs["gates " + tag] = (torch.stack(list(crit[3])), "exact")
                obs["capacity " + tag] = (int(crit[4]), "exact")
                obs["dispatch_count " + tag] = (crit[5].to(torch.int32), "exact")
                obs["l_aux " + tag] = (l_aux, "host")
            M = 48
            x = torch.randn([T, M], generator=g).to(dtype)
            y = torch.randn([E * crit[4], M], generator=g).to(dtype).view(E, -1, M)
            for post in (True, False):
                obs[f"encode post={post} " + tag] = (impl.encode(x, crit, post), "exact")
                obs[f"decode post={post} " + tag] = (impl.decode(y, crit, post), "exact")
        m = (torch.rand([777, 33], generator=torch.Generator().manual_seed(5)) < 0.2).to(torch.int64)
        obs[f"cumsum_sub_one {dts}"] = (impl.cumsum_sub_one(m).to(torch.int32), "exact")
    # gate gradient kernel (backward-only row)
    g = torch.Generator().manual_seed(9)
    T, E, k, M = 200, 6, 2, 40
    torch.randn([T, E], generator=g)
    cr, _ = impl.route(scores["gate_grad"], k, 0.75, True)
    x, buf = torch.randn([T, M], generator=g), torch.randn([E * cr[4], M], generator=g)
    for j in range(k):
        obs[f"gate_grad j={j}"] = (impl.gate_grad(x, buf, cr[1][j], cr[2][j], cr[4]), "exact")
    # the dispatcher with MASKED tokens (idx < 0 is skipped by the kernels)
    g = torch.Generator().manual_seed(13)
    T, E, k, M = 300, 8, 2, 24
    torch.randn([T, E], generator=g)
    cr, _ = impl.route(scores["masked"], k, 1.0, True)
    idx = [i.clone() for i in cr[1]]
    idx[0][::7] = -1
    idx[1][::5] = -1
    x = torch.randn([T, M], generator=g)
    for post in (True, False):
        enc, dec = impl.dispatch(E, cr[4], M, idx, cr[2], cr[3], post, x)
        obs[f"dispatcher encode with masked tokens post={post}"] = (enc.reshape(-1, M), "exact")
        obs[f"dispatcher decode with masked tokens post={post}"] = (dec.reshape(-1, M), "exact")
    # host-side loss functions
    sc = scores["losses"]
    ids = torch.topk(sc, 2, dim=1).indices
    obs["gshard_loss (torch form)"] = (impl.gshard_loss(sc, ids), "host")
    g = torch.Generator().manual_seed(78)
    logits = torch.randn([640, 24], generator=g)
    obs["load_importance_loss"] = (impl.load_importance_loss(scores["losses_logits_softmax"], logits.gather(1, ids), 24, 0.7), "close")
    return obs


def surface_checks(build):
    """make_golden.py check_product_host_logic_against_reference: the drop-in layer built by `build` (the reference's
    tutel.moe.moe_layer, or tutel_amd's MOELayer with the oracle's CPU ops in place of the HIP kernels)."""
    obs = {}
    relu = lambda t: torch.nn.functional.relu(t)

    def fresh(d):   # (the reference pops keys out of the dicts it is given)
        gt = d["gate_type"]
        return {**d, "experts": dict(d["experts"]),
                "gate_type": [dict(g_) for g_ in gt] if isinstance(gt, list) else (dict(gt) if isinstance(gt, dict) else gt)}
    # seeds -> identical parameters
    kw = dict(gate_type=[{"type": "top", "k": 1}, {"type": "top", "k": 2, "capacity_factor": 1.5}],
              experts={"type": "ffn", "num_experts_per_device": 4, "hidden_size_per_expert": 24, "activation_fn": relu},
              model_dim=32, seeds=(5, 6, 7), is_postscore=False)
    lay = build(**fresh(kw))
    sd = lay.state_dict()
    obs["state_dict keys"] = (sorted(sd), "exact")
    for n in sorted(sd):
        obs[f"seeded initial parameter {n}"] = (sd[n], "exact")
    # multiple gates, gate_index, forward-time overrides
    g = torch.Generator().manual_seed(2)
    x = torch.randn([3, 50, 32], generator=g)
    lay.eval()
    for kwargs in ({}, {"gate_index": 1}, {"gate_index": 1, "top_k": 1}, {"capacity_factor": 2.0}, {"gate_index": 1, "capacity_factor": 0.0},
                   {"gate_index": 0, "capacity_factor": -0.5, "top_k": 3}):
        with torch.no_grad():
            y = lay(x, **kwargs)
        obs[f"forward{kwargs}"] = (y, "host")
        obs[f"l_aux forward{kwargs}"] = (y.l_aux, "host")
        obs[f"dispatch_count forward{kwargs}"] = (lay.dispatch_count.to(torch.int32), "exact")
    for attr in ("num_global_experts", "num_local_experts", "sharded_count", "world_size", "valid_rs", "adaptive_degree", "model_dim"):
        obs[f"attribute {attr}"] = (getattr(lay, attr), "exact")
    obs["gate attributes"] = ([[g_.top_k, g_.gate_noise, g_.capacity_factor] for g_ in lay.gates], "exact")
    # training: forward + backward through dispatch / combine and the experts
    for post in (True, False):
        kw_t = dict(gate_type={"type": "top", "k": 2}, experts={"type": "ffn", "num_experts_per_device": 4, "hidden_size_per_expert": 24,
                                                                 "activation_fn": relu}, model_dim=32, seeds=(5, 6, 7), is_postscore=post)
        lay_t = build(**fresh(kw_t)).train()
        xi = torch.randn([100, 32], generator=g).requires_grad_(True)
        y = lay_t(xi)
        (y.square().sum() + 3.0 * y.l_aux).backward()
        obs[f"training gradient is_postscore={post} input"] = (xi.grad, "grad")
        for n, p in sorted(lay_t.named_parameters()):
            if p.grad is not None:
                obs[f"training gradient is_postscore={post} {n}"] = (p.grad, "grad")

    # reserve_dims = 2 with a custom expert module, result_func, scan_expert_func
    class Scale(torch.nn.Module):
        def __init__(self, model_dim, num_experts_per_device, sharded_count, **kw_):
            super().__init__()
            torch.manual_seed(3)
            self.s = torch.nn.Parameter(torch.rand(num_experts_per_device, 1, 1, 1))

        def forward(self, x, ctx):
            assert x.dim() == 4
            return x * self.s + 1.0
    seen = []
    kw = dict(gate_type={"type": "top", "k": 2}, experts={"type": "custom", "module": Scale, "num_experts_per_device": 3}, model_dim=24,
              seeds=(1, 2, 3), result_func=lambda t: t * 2)
    lay = build(scan_expert_func=lambda n, p: seen.append(n), **fresh(kw)).eval()
    x = torch.randn([2, 30, 4, 6], generator=g)
    with torch.no_grad():
        y = lay(x, reserve_dims=2)
    obs["reserve_dims = 2 + custom expert + result_func"] = (y, "host")
    obs["scan_expert_func names"] = (seen, "exact")
    obs["protected_shape"] = ([int(v) for v in lay.protected_shape], "exact")
    # deprecated spellings and error behaviour
    lay = build(gate_type="Top2Gate", experts={"type": "ffn", "count_per_node": 2, "hidden_size_per_expert": 8, "activation_fn": relu},
                model_dim=8, pad_samples=True)
    obs["deprecated spellings"] = ([lay.gates[0].top_k, lay.num_local_experts], "exact")
    for badkw in (dict(no_such_option=1), dict(parallel_type="nonsense")):
        try:
            build(gate_type={"type": "top", "k": 1}, experts={"type": "ffn", "num_experts_per_device": -1 if "parallel_type" in badkw else 1,
                                                               "hidden_size_per_expert": 8, "activation_fn": relu}, model_dim=8, **badkw)
            raised = False
        except Exception:   # noqa: BLE001
            raised = True
        obs[f"raises on {sorted(badkw)}"] = (raised, "exact")
    return {"layer: " + n: v for n, v in obs.items()}


def to_record(obs):
    """observations -> four arrays for np.savez: "meta" (JSON: per observation its name, mode, dtype, shape, plain value or where its
    full values lie), "sha256" ([N, 32] uint8 digests), "full32" / "full64" (the concatenated values of the small non-"exact" tensors)"""
    import numpy as np
    meta, shas, full = [], [], {"full32": [], "full64": []}
    offs = {"full32": 0, "full64": 0}
    for name, (v, mode) in obs.items():
        ent = {"name": name, "mode": mode}
        if torch.is_tensor(v):
            v = v.detach().cpu()
            ent.update(dtype=str(v.dtype), shape=list(v.shape), sha=len(shas))
            shas.append(np.frombuffer(bytes.fromhex(digest(v)), dtype=np.uint8))
            if mode != "exact" and v.numel() <= FULL_LIMIT and v.is_floating_point():
                key = "full64" if v.dtype == torch.float64 else "full32"
                a = v.to(torch.float64 if key == "full64" else torch.float32).reshape(-1).numpy()
                ent["full"] = [key, offs[key], int(a.size)]
                full[key].append(a)
                offs[key] += a.size
        else:
            ent["json"] = json.loads(json.dumps(v))
        meta.append(ent)
    return {"meta": np.array([json.dumps(meta)]), "sha256": np.stack(shas) if shas else np.zeros([0, 32], np.uint8),
            "full32": np.concatenate(full["full32"]).astype(np.float32) if full["full32"] else np.zeros([0], np.float32),
            "full64": np.concatenate(full["full64"]) if full["full64"] else np.zeros([0], np.float64)}


def from_record(z):
    """to_record's arrays (an np.load result or the dict itself) -> {name: {"mode", "sha256", "dtype", "shape", "full" | "json"}}"""
    meta = json.loads(str(z["meta"][0]))
    shas, full = z["sha256"], {"full32": z["full32"], "full64": z["full64"]}
    out = {}
    for ent in meta:
        if "sha" in ent:
            ent["sha256"] = bytes(shas[ent["sha"]]).hex()
        if "full" in ent:
            key, off, n = ent["full"]
            ent["full"] = full[key][off:off + n].reshape(ent["shape"])
        out[ent["name"]] = ent
    return out


def compare(name, mine, mode, ref, live=False):
    """None when `mine` matches the stored reference observation `ref` (a from_record entry), else the reason.  live=True (both sides
    computed in one process) takes "host" as "exact"."""
    import warnings
    import numpy as np
    if not torch.is_tensor(mine):
        want = ref.get("json", "<a tensor>")
        return None if json.loads(json.dumps(mine)) == want else f"{mine!r} vs the reference's {want!r}"
    mine = mine.detach().cpu()
    if "sha256" not in ref:
        return f"a tensor where the reference observed {ref.get('json')!r}"
    if str(mine.dtype) != ref["dtype"] or list(mine.shape) != ref["shape"]:
        return f"{mine.dtype} {list(mine.shape)} vs the reference's {ref['dtype']} {ref['shape']}"
    if digest(mine) == ref["sha256"]:
        return None
    if mode == "exact" or "full" not in ref or (live and mode == "host"):
        return "differs from the reference bit for bit"
    got, want = mine.to(torch.float64), torch.from_numpy(np.ascontiguousarray(ref["full"])).to(torch.float64)
    big = float(want.abs().max()) if want.numel() else 0.0
    if mode == "grad":
        ok = torch.allclose(got, want, rtol=1e-5, atol=1e-5 * max(1.0, big))
    elif mode == "allclose":
        ok = torch.allclose(got, want)
    elif mode == "close":
        ok = torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    else:   # "host": up to 4 places of the largest element, in the value's dtype
        place = float(torch.finfo(mine.dtype).eps) * max(big, float(torch.finfo(mine.dtype).tiny))
        ok = float((got - want).abs().max()) <= 4 * place
        if ok:
            warnings.warn(f"{name}: not the reference's bits on this host (max diff {float((got - want).abs().max()):.3e}, within 4 places "
                          f"of {mine.dtype}): ATen reduces / multiplies in another order here than where the fixture was written")
    return None if ok else f"max diff {float((got - want).abs().max()):.3e}"


class OracleImpl:
    """this repository's side of function_checks: the oracle (oracle/moe_oracle.py + its C port) and tutel_amd's loss functions"""

    def __init__(self):
        from oracle import moe_oracle as O
        from tutel_amd.impls import losses
        self.O, self.losses = O, losses

    def route(self, scores, k, cf, norm):
        return self.O.extract_critical(scores, k, cf, normalize_gate=norm)

    def encode(self, x, crit, post):
        return self.O.fast_encode(x, crit, post)

    def decode(self, y, crit, post):
        return self.O.fast_decode(y, crit, post)

    def cumsum_sub_one(self, m):
        return self.O.cumsum_sub_one(m)

    def gate_grad(self, x, buf, idx, loc, C):
        return self.O.gate_grad(x, buf, idx, loc, C)

    def dispatch(self, E, C, M, idx, loc, gates, post, x):
        crit = (E, idx, loc, gates, C, None)
        enc = self.O.fast_encode(x, crit, post)
        return enc, self.O.fast_decode(enc, crit, post)

    def gshard_loss(self, scores, ids):
        return self.losses.gshard_loss(scores, ids)

    def load_importance_loss(self, *a):
        return self.losses.load_importance_loss(*a)


PRODUCT_OPS = ("gate_topk", "compute_location", "slot_map", "cumsum_sub_one", "fast_encode", "fast_decode", "gate_grad")


def product_build(setattr_=setattr):
    """tutel_amd's MOELayer with the oracle's CPU ops (tests/_cpu_ops.py) in place of the HIP kernels; `setattr_` lets a test
    undo the patch (monkeypatch.setattr)"""
    import _cpu_ops
    from tutel_amd import ops
    from tutel_amd.impls import moe_layer
    for name in PRODUCT_OPS:
        setattr_(ops, name, getattr(_cpu_ops, name))
    return moe_layer.MOELayer


def net_checks(net, rank, world):
    """make_golden_ep.py check_net_against_reference, one rank's side: tutel.net's collectives with and without autograd (outputs,
    and gradients of a fixed weighted sum), TutelDistributedOptimizer, create_groups_from_world -- inside a gloo group of `world`
    ranks.  A call that raises is observed as "<name> raises" (the reference cannot run some of them on gloo: not compared)."""
    obs = {}
    g = torch.Generator().manual_seed(40 + rank)

    def call(name, fn, *tensors, grad=False):
        ins = [t.clone().requires_grad_(grad) for t in tensors]
        try:
            y = fn(net, *ins)
        except Exception as ex:   # noqa: BLE001
            obs[f"{name} raises"] = (type(ex).__name__, "exact")
            return
        ys = [t for t in (list(y) if isinstance(y, (tuple, list)) else [y]) if torch.is_tensor(t)]
        for i, t in enumerate(ys):
            obs[f"{name} output {i}"] = (t.detach(), "exact")
        if grad:
            sum((t.float() * torch.arange(t.numel(), dtype=torch.float32).view(t.shape)).sum() for t in ys).backward()
            for i, t in enumerate(ins):
                obs[f"{name} gradient {i}"] = (t.grad, "allclose") if t.grad is not None else ("none", "exact")
    x = torch.randn([4 * world, 6, 8], generator=g)
    call("simple_all_reduce", lambda n, t: n.simple_all_reduce(t), x)
    call("simple_all_to_all", lambda n, t: n.simple_all_to_all(t), x)
    call("simple_split", lambda n, t: n.simple_split(t), x)
    call("simple_all_gather", lambda n, t: n.simple_all_gather(t), x)
    call("simple_reduce_scatter", lambda n, t: n.simple_reduce_scatter(t), x)
    for i, o in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (0, 0)):
        xx = torch.randn([2 * world, 3 * world, 4 * world], generator=g)
        call(f"all_to_all({i},{o})", lambda n, t, i=i, o=o: n.all_to_all(t, i, o), xx, grad=True)
        call(f"all_to_all({i},{o},use_2dh)", lambda n, t, i=i, o=o: n.all_to_all(t, i, o, use_2dh=True), xx, grad=True)
    call("all_to_all_single", lambda n, t: n.all_to_all_single(t), x, grad=True)
    for d in (0, 1, 2):
        call(f"all_gather(dim={d})", lambda n, t, d=d: n.all_gather(t, d), x, grad=True)
        call(f"reduce_scatter(dim={d})", lambda n, t, d=d: n.reduce_scatter(t, d), torch.randn([2 * world, 2 * world, 2 * world], generator=g), grad=True)
        call(f"spatial_split(dim={d})", lambda n, t, d=d: n.spatial_split(t, d), torch.randn([2 * world, 2 * world, 2 * world], generator=g), grad=True)
    call("allreduce_forward", lambda n, t: n.allreduce_forward(t), x, grad=True)
    call("allreduce_backward", lambda n, t: n.allreduce_backward(t), x, grad=True)
    call("zero_gather", lambda n, t: n.zero_gather(t), torch.randn([5, 3], generator=g), grad=True)
    call("zero_scatter", lambda n, t: n.zero_scatter(t, n.simple_split)[0], torch.randn([7, 3], generator=g))
    # TutelDistributedOptimizer: three SGD steps on a shared parameter of awkward size + an "expert" one
    torch.manual_seed(11)
    shared, expert = torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(4, 2) + rank)
    expert._tutel_expert = True
    opt = net.TutelDistributedOptimizer([shared, expert], average_shared=True).warp_local(torch.optim.SGD, lr=0.1, momentum=0.5)
    for step in range(3):
        opt.zero_grad()
        ((shared * (rank + 1 + step)).sum() ** 2 + (expert ** 2).sum()).backward()
        opt.step()
    obs["TutelDistributedOptimizer shared parameter after 3 steps"] = (shared.data.clone(), "exact")
    obs["TutelDistributedOptimizer expert parameter after 3 steps"] = (expert.data.clone(), "exact")
    for gc in (1, 2, -2):
        try:
            grp = net.create_groups_from_world(group_count=gc)
            obs[f"create_groups_from_world({gc})"] = ([getattr(grp, a, None) for a in ("global_size", "global_rank", "group_count", "data_rank",
                                                                                          "model_rank", "is_distributed")], "exact")
        except Exception as ex:   # noqa: BLE001
            obs[f"create_groups_from_world({gc}) raises"] = (type(ex).__name__, "exact")
    return {"net: " + n: v for n, v in obs.items()}


NET_WORLD = 2


def comparable_net_names(ref, mine):
    """the observations of calls the reference could run (its "raises" ones are not compared, as make_golden_ep.py does not)"""
    skipped = {n[:-len(" raises")] for n in ref if n.endswith(" raises")}
    keep = lambda n: not any(n == s + " raises" or n.startswith(s + " output ") or n.startswith(s + " gradient ") for s in skipped)
    return {n for n in ref if keep(n)}, {n for n in mine if keep(n)}


def net_worker(rank, world, port, q, which, fixture):
    """one rank: `which` = "reference" (record: returns to_record of the observations) or "product" (replay: compares tutel_amd.net
    with the stored observations of the reference for this rank and returns the mismatches)"""
    import os
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        if which == "reference":
            from tutel import net
        else:
            from tutel_amd import net
        obs = net_checks(net, rank, world)
        if which == "reference":
            res = to_record(obs)
        else:
            import numpy as np
            z = np.load(fixture)
            pre = f"net{rank}:"
            ref = from_record({f[len(pre):]: z[f] for f in z.files if f.startswith(pre)})
            names_ref, names_mine = comparable_net_names(ref, obs)
            res = [f"{n}: only on one side" for n in sorted(names_ref ^ names_mine)]
            res += [f"{n}: {why}" for n in sorted(names_ref & names_mine) for why in [compare(n, obs[n][0], obs[n][1], ref[n])] if why]
            res = (res, len(names_ref))
        q.put((rank, res, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:   # noqa: BLE001
        import traceback
        q.put((rank, None, traceback.format_exc()))


def run_net(which, fixture=None, world=NET_WORLD):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=net_worker, args=(r, world, port, q, which, fixture)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    errs = [tb for _, _, tb in res if tb]
    assert not errs, errs[0]
    return dict((r, v) for r, v, _ in res)
