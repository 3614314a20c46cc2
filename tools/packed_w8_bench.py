#!/usr/bin/env python3
"""What FP8 expert weights cost on the PACKED dropless forward (layer.dropless_packed_fp8; impls/packed_w8.py, the W8A16 GEMMs over the
packed tables of csrc/expert_gemm_w8.hip), bf16, against the forwards it stands between.

  --what layer   E = 64, T = 4096, k = 2, M = H = 2048, capacity_factor 0, `ffn` and `llama_ffn` experts; arms alternated sample by
                 sample in ONE process, each sample timed with device events after a warm-up:
                   packed16_eager / packed16_graph   the 16-bit packed forward, eager and graph-replayed
                   fp8_padded_eager                  experts.fp8_weights on the padded layout: the capacity is read back to the host
                                                     (the only FP8 dropless path without the route; not capturable)
                   fp8_packed_eager / fp8_packed_graph   the new route, eager and graph-replayed
                 On a tree without the route (--root of an older checkout), or with --existing-only, the last two are left out: the
                 first three, measured with the same arm set on both trees, show that the existing forwards did not move.
  --what kernel  tutel_amd_expert_gemm_w8_packed (N = K = 2048, bias + ReLU, plain rows) on synthesised layouts:
                   r128   64 experts x 128 rows   against the padded tutel_amd_expert_gemm_w8 on [64, 128, K]: the same work items
                   r160   64 experts x 160 rows (both halves of every table tile live)   against the 16-bit packed GEMM
                          (tutel_amd_expert_gemm_packed, k-major) on the same layout
                 The XCD mapping of the packed kernel is a process-wide setting (TUTEL_AMD_W8_PACKED_MAP=bound cuts the XCD chunks from
                 the grid instead of the live tile count): run the tool once with --map live and once with --map bound.
  --only ARM     run that one kernel arm --iters times and nothing else: the command of a counter-only profiler run (FETCH_SIZE)

Prints one JSON line: per arm median / min / max in microseconds over --samples samples (a kernel sample is --inner back-to-back
launches between one pair of events; a layer sample is one forward).

    python tools/packed_w8_bench.py --what kernel layer [--map live|bound] [--root DIR] [--samples 30] [--warmup 5] [--inner 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

DT = torch.bfloat16
LAYER = dict(E=64, T=4096, K=2, M=2048, H=2048)
KERNEL = dict(E=64, N=2048, Kdim=2048)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def alternate(arms, samples, warmup, inner):
    """{name: fn} -> {name: {median_us, min_us, max_us, samples}}; the arms take turns, sample by sample"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in arms}
    for _ in range(samples):
        for name, fn in arms.items():
            got[name].append(timed(fn, inner))
    return {name: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2), samples=len(v))
            for name, v in got.items()}


# ---- kernel ---------------------------------------------------------------------------------------------------------------------------------
def layout_of(ops, ep_native, rows):
    """the library's own layout of a routing in which expert e keeps rows[e] entries (k = 1, one token per entry)"""
    n, E = sum(rows), len(rows)
    r = torch.tensor(rows, dtype=torch.int64)
    idx = torch.repeat_interleave(torch.arange(E), r).int().view(1, n).cuda()
    start = torch.cumsum(r, 0) - r
    loc = (torch.arange(n) - torch.repeat_interleave(start, r)).int().view(1, n).cuda()
    plan, why = ep_native.packed_plan(n, E, 1, 128, 128, 128, DT, 0, 1)
    assert plan is not None, why
    return ops.packed_layout(torch.tensor(rows, dtype=torch.int32).cuda(), idx, loc, 0, 1, plan["rows_bound"], plan["tiles_bound"], plan["row_limit"])


def kernel_arms(ops, ep_native, w8):
    E, N, Kd = KERNEL["E"], KERNEL["N"], KERNEL["Kdim"]
    g = torch.Generator().manual_seed(E)
    w = (torch.randn([E, N, Kd], generator=g) / Kd ** 0.5).to(DT).cuda()
    bias = torch.randn([E, N], generator=g).to(DT).cuda()
    image, scale = w8.prepare(w, True)
    arms, info = {}, {}
    for name, R in (("r128", 128), ("r160", 160)):
        lay = layout_of(ops, ep_native, [R] * E)
        a = (torch.randn([lay.rows_bound, Kd], generator=g) * 0.5).to(DT).cuda()
        out = torch.empty([lay.rows_bound, N], dtype=DT, device="cuda")
        info[name] = dict(rows=E * R, rows_bound=lay.rows_bound, tiles_bound=lay.tiles_bound, live_tiles=int(lay.ntiles),
                          grid=lay.tiles_bound * 2 * (N // 128))
        arms["w8_packed_" + name] = (lambda lay=lay, a=a, out=out: ops.expert_gemm_w8_packed(a, image, scale, bias, N, Kd, lay, act="relu", out=out))
        if R == 128:
            ab = a[:E * R].view(E, R, Kd)
            ob = torch.empty([E, R, N], dtype=DT, device="cuda")
            arms["w8_padded_r128"] = (lambda ab=ab, ob=ob: ops.expert_gemm_w8(ab, image, scale, bias, N, Kd, act="relu", out=ob))
            # the same rows, the same experts: the same bits
            assert torch.equal(arms["w8_packed_r128"]()[:E * R].view(E, R, N), arms["w8_padded_r128"]()), "packed rows differ from the padded kernel's"
        else:
            o16 = torch.empty([lay.rows_bound, N], dtype=DT, device="cuda")
            arms["packed16_" + name] = (lambda lay=lay, a=a, o16=o16: ops.expert_gemm_packed(a, w, bias, True, lay, act="relu", out=o16))
    return arms, info


# ---- layer ----------------------------------------------------------------------------------------------------------------------------------
def make_layer(kind):
    from tutel import moe
    E, M, H, K = LAYER["E"], LAYER["M"], LAYER["H"], LAYER["K"]
    torch.manual_seed(E)
    old = torch.get_default_dtype()
    torch.set_default_dtype(DT)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 0.0},
                              experts={"type": kind, "num_experts_per_device": E, "hidden_size_per_expert": H}, model_dim=M)
    finally:
        torch.set_default_dtype(old)
    if kind == "llama_ffn":
        with torch.no_grad():   # a wider spread than the reference's normal(0, 0.01)
            layer.experts.W_fc1.normal_(0, M ** -0.5); layer.experts.W_fc2.normal_(0, M ** -0.5); layer.experts.W_fc3.normal_(0, H ** -0.5)
    layer = layer.cuda().eval()
    for p in layer.parameters():
        p.requires_grad_(False)
    return layer


def layer_arms(kind, has_route):
    from tutel_amd.impls.graph import GraphedForward
    layer = make_layer(kind)
    x = torch.randn([LAYER["T"], LAYER["M"]], device="cuda").to(DT)
    ran = {}

    def setup(fp8, packed, route):
        layer.experts.fp8_weights, layer.dropless_packed = fp8, packed
        if has_route:
            layer.dropless_packed_fp8 = route

    def eager(name, fp8, packed, route):
        def run():
            setup(fp8, packed, route)
            with torch.no_grad():
                layer(x)
            ran[name] = (layer._dropless_packed_ran, layer._fp8_weights_ran)
        return run

    def graphed(name, fp8, route):
        setup(fp8, True, route)
        with torch.no_grad():
            layer(x)   # one eager forward: workspaces, cached images
        g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
        ran[name] = (layer._dropless_packed_ran, layer._fp8_weights_ran)
        return lambda: g(x)

    arms = {"packed16_eager": eager("packed16_eager", False, True, False), "packed16_graph": graphed("packed16_graph", False, False),
            "fp8_padded_eager": eager("fp8_padded_eager", True, False, False)}
    if has_route:
        arms["fp8_packed_eager"] = eager("fp8_packed_eager", True, True, True)
        arms["fp8_packed_graph"] = graphed("fp8_packed_graph", True, True)
    return arms, ran, layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["kernel", "layer"], choices=["kernel", "layer"])
    ap.add_argument("--kinds", nargs="+", default=["ffn", "llama_ffn"], choices=["ffn", "llama_ffn"])
    ap.add_argument("--map", default="live", choices=["live", "bound"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--existing-only", action="store_true", help="layer: leave the new route's two arms out (the arm set of an older checkout)")
    ap.add_argument("--only", default=None, help="run this kernel arm --iters times, untimed (a counter-only profiler run)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["TUTEL_AMD_W8_PACKED_MAP"] = args.map   # read once, when the library launches its first packed W8 kernel
    sys.path.insert(0, os.path.abspath(args.root))
    if not torch.cuda.is_available():
        sys.exit("packed_w8_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    from tutel_amd.experts import w8
    from tutel_amd.impls import ep_native
    has_route = hasattr(ops, "expert_gemm_w8_packed")
    if args.only:
        arms, _ = kernel_arms(ops, ep_native, w8)
        for _ in range(args.iters):
            arms[args.only]()
        torch.cuda.synchronize()
        return
    out = {"tool": "tools/packed_w8_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "root": os.path.basename(os.path.abspath(args.root)),
           "has_route": has_route, "map": args.map, "samples": args.samples, "warmup": args.warmup, "inner": args.inner}
    if "kernel" in args.what and has_route:
        arms, info = kernel_arms(ops, ep_native, w8)
        res = alternate(arms, args.samples, args.warmup, args.inner)
        out["kernel"] = dict(shape=KERNEL, layouts=info, arms=res,
                             packed_over_padded_r128=round(res["w8_packed_r128"]["median_us"] / res["w8_padded_r128"]["median_us"], 3),
                             w8_over_16bit_r160=round(res["w8_packed_r160"]["median_us"] / res["packed16_r160"]["median_us"], 3))
        del arms
        torch.cuda.empty_cache()
    if "layer" in args.what:
        out["layer"] = {"shape": LAYER}
        for kind in args.kinds:
            arms, ran, layer = layer_arms(kind, has_route and not args.existing_only)
            res = alternate(arms, args.samples, args.warmup, 1)
            assert ran["packed16_eager"][0] is True and ran["packed16_graph"][0] is True, ran
            assert ran["fp8_padded_eager"][1] is True, ran
            if "fp8_packed_eager" in arms:
                assert ran["fp8_packed_eager"] == (True, True) and ran["fp8_packed_graph"] == (True, True), ran
            out["layer"][kind] = res
            del arms, layer
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
