#!/usr/bin/env python3
"""What W8A8 costs on the PACKED dropless forward (layer.dropless_packed_w8a8; impls/packed_w8.py under its W8A8 format, the fp8 x fp8 GEMMs
over the packed tables of csrc/expert_gemm_w8a8.hip), bf16, in ONE process; the helpers are tools/packed_w8_bench.py's.

  kernel  N = K = 2048, plain rows, on synthesised layouts of 64 experts x 128 rows (r128) and 64 x 160 rows (r160), arms alternated
          sample by sample, each as fc1 (bias + ReLU), fc2 (bias) and the SwiGLU gate / up launch (glu, H = 2048):
            wide_*      one work item per 256-row table tile (TUTEL_AMD_W8A8_PACKED_TILE=wide; the variable is read at every call)
            halves_*    two 128-row halves per table tile (TUTEL_AMD_W8A8_PACKED_TILE=halves)
            w8a16_*     the packed W8A16 kernel (tutel_amd_expert_gemm_w8_packed / _glu_packed) on the 16-bit rows
            padded_*    the padded tutel_amd_expert_gemm_w8a8 / _glu on [64, R, K] (fc1 and glu)
          The fc1 A/B decides the library's default form together with the resource table: wide only if it has no scratch, its median is
          below halves' at r160 and not above it at r128 beyond the min - max spread of the halves samples (DESIGN 4.4 holds the result).
  layer   E = 64, T = 4096, k = 2, M = H = 2048, capacity_factor 0, eager and graph-replayed:
            packed16_*      the 16-bit packed forward
            fp8_packed_*    the packed FP8 (W8A16) forward
            w8a8_packed_*   the packed W8A8 forward, in the library's default form

Prints one JSON line: per arm median / min / max in microseconds over --samples samples.

    python tools/packed_w8a8_bench.py [--what kernel layer] [--kinds ffn llama_ffn] [--samples 30] [--warmup 5] [--inner 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import packed_w8_bench as B  # noqa: E402

TILE_ENV = "TUTEL_AMD_W8A8_PACKED_TILE"
RUNS = ("r128", "r160")


def kernel_arms(ops, ep_native, w8):
    E, N, Kd = B.KERNEL["E"], B.KERNEL["N"], B.KERNEL["Kdim"]
    g = torch.Generator().manual_seed(E)

    def weights(channels):
        return (torch.randn([E, channels, Kd], generator=g) / Kd ** 0.5).to(B.DT).cuda()
    image, scale = w8.prepare(weights(N), True)
    image_gu, scale_gu = w8.prepare_gate_up(weights(N), weights(N), True)
    bias = torch.randn([E, N], generator=g).to(B.DT).cuda()
    arms = {}

    def formed(form, fn):
        def run():
            os.environ[TILE_ENV] = form
            return fn()
        return run

    for name, R in zip(RUNS, (128, 160)):
        lay = B.layout_of(ops, ep_native, [R] * E)
        a = (torch.randn([lay.rows_bound, Kd], generator=g) * 0.5).to(B.DT).cuda()
        q, s = ops.quantize_rows_a8(a)
        out = torch.empty([lay.rows_bound, N], dtype=B.DT, device="cuda")
        for form in ("wide", "halves"):
            arms[f"{form}_fc1_{name}"] = formed(form, lambda lay=lay, q=q, s=s, out=out: ops.expert_gemm_w8a8_packed(
                q, s, image, scale, bias, N, Kd, B.DT, lay, act="relu", out=out))
            arms[f"{form}_fc2_{name}"] = formed(form, lambda lay=lay, q=q, s=s, out=out: ops.expert_gemm_w8a8_packed(
                q, s, image, scale, bias, N, Kd, B.DT, lay, out=out))
            arms[f"{form}_glu_{name}"] = formed(form, lambda lay=lay, q=q, s=s, out=out: ops.expert_gemm_w8a8_glu_packed(
                q, s, image_gu, scale_gu, N, Kd, B.DT, lay, act="silu", out=out))
        arms["w8a16_fc1_" + name] = lambda lay=lay, a=a, out=out: ops.expert_gemm_w8_packed(a, image, scale, bias, N, Kd, lay, act="relu", out=out)
        arms["w8a16_fc2_" + name] = lambda lay=lay, a=a, out=out: ops.expert_gemm_w8_packed(a, image, scale, bias, N, Kd, lay, out=out)
        arms["w8a16_glu_" + name] = lambda lay=lay, a=a, out=out: ops.expert_gemm_w8_glu_packed(a, image_gu, scale_gu, N, Kd, lay, act="silu", out=out)
        qb, sb = q[:E * R].view(E, R, Kd), s[:E * R].contiguous()
        ob = torch.empty([E, R, N], dtype=B.DT, device="cuda")
        arms["padded_fc1_" + name] = lambda qb=qb, sb=sb, ob=ob: ops.expert_gemm_w8a8(qb, sb, image, scale, bias, N, Kd, B.DT, act="relu", out=ob)
        arms["padded_glu_" + name] = lambda qb=qb, sb=sb, ob=ob: ops.expert_gemm_w8a8_glu(qb, sb, image_gu, scale_gu, N, Kd, B.DT, act="silu", out=ob)
        # the same quantised rows, the same experts: the same bits, whichever form
        for op in ("fc1", "fc2", "glu"):
            want = arms[f"halves_{op}_{name}"]().clone()
            assert torch.equal(arms[f"wide_{op}_{name}"]()[:E * R], want[:E * R]), op + ": the wide form's rows differ from the halves form's"
    return arms


def layer_arms(kind):
    from tutel_amd.impls.graph import GraphedForward
    layer = B.make_layer(kind)
    x = torch.randn([B.LAYER["T"], B.LAYER["M"]], device="cuda").to(B.DT)
    ran = {}

    def setup(fmt):
        layer.dropless_packed = True
        layer.experts.fp8_weights = layer.dropless_packed_fp8 = fmt is not None
        layer.experts.fp8_activations = layer.dropless_packed_w8a8 = fmt == "w8a8"

    def report():
        return layer._dropless_packed_ran, layer._fp8_weights_ran, layer._fp8_activations_ran

    def eager(name, fmt):
        def run():
            setup(fmt)
            with torch.no_grad():
                layer(x)
            ran[name] = report()
        return run

    def graphed(name, fmt):
        eager(name, fmt)()   # one eager forward: workspaces, cached images
        g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
        ran[name] = report()
        return lambda: g(x)

    arms = {}
    for fmt, stem in ((None, "packed16"), ("fp8", "fp8_packed"), ("w8a8", "w8a8_packed")):
        arms[stem + "_eager"] = eager(stem + "_eager", fmt)
        arms[stem + "_graph"] = graphed(stem + "_graph", fmt)
    return arms, ran, layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["kernel", "layer"], choices=["kernel", "layer"])
    ap.add_argument("--kinds", nargs="+", default=["ffn", "llama_ffn"], choices=["ffn", "llama_ffn"])
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("packed_w8a8_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    from tutel_amd.experts import w8
    from tutel_amd.impls import ep_native
    out = {"tool": "tools/packed_w8a8_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "samples": args.samples,
           "warmup": args.warmup, "inner": args.inner}
    if "kernel" in args.what:
        res = B.alternate(kernel_arms(ops, ep_native, w8), args.samples, args.warmup, args.inner)
        os.environ.pop(TILE_ENV, None)
        wide, halves = ({r: res[f"{form}_fc1_{r}"] for r in RUNS} for form in ("wide", "halves"))
        # the timing half of the docstring's rule, on this run's samples (the other half is the resource table's scratch column)
        faster = (wide["r160"]["median_us"] < halves["r160"]["median_us"] and
                  wide["r128"]["median_us"] <= halves["r128"]["median_us"] + (halves["r128"]["max_us"] - halves["r128"]["min_us"]))
        out["kernel"] = dict(shape=B.KERNEL, arms=res, timing_rule_admits_wide=bool(faster),
                             wide_over_halves={r: round(wide[r]["median_us"] / halves[r]["median_us"], 3) for r in RUNS})
        torch.cuda.empty_cache()
    if "layer" in args.what:
        out["layer"] = {"shape": B.LAYER}
        for kind in args.kinds:
            arms, ran, layer = layer_arms(kind)
            res = B.alternate(arms, args.samples, args.warmup, 1)
            for stem, want in (("packed16", (True, None, None)), ("fp8_packed", (True, True, None)), ("w8a8_packed", (True, None, True))):
                for mode in ("_eager", "_graph"):
                    got = ran[stem + mode]
                    assert got[0] is True and all(w is None or g is True for g, w in zip(got, want)), (stem + mode, got)
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
