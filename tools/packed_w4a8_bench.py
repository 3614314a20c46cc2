#!/usr/bin/env python3
"""What W4A8 costs on the PACKED dropless forward (layer.dropless_packed_w4a8; impls/packed_w8.py under its W4A8 format, the block-scaled
fp4 x fp8 GEMMs over the packed tables of csrc/expert_gemm_w4a8.hip), bf16, in ONE process; the helpers are tools/packed_w8_bench.py's.

  kernel  N = K = 2048, bias + ReLU, plain rows, on synthesised layouts of 64 experts x 128 rows (r128) and 64 x 160 rows (r160), arms
          alternated sample by sample:
            w4a8_wide_*     one work item per 256-row table tile (TUTEL_AMD_W4A8_PACKED_TILE=wide; the variable is read at every call)
            w4a8_halves_*   two 128-row halves per table tile (TUTEL_AMD_W4A8_PACKED_TILE=halves)
            w4a8_padded_*   the padded tutel_amd_expert_gemm_w4a8 on [64, R, K]
            w4_halves_*     the packed W4A16 halves kernel (tutel_amd_expert_gemm_w4_packed) on the 16-bit rows
            quantize_*      the bounded row quantiser over the [rows_bound, K] rows, the bound offsets[E] on the device
          The A/B decides the library's default form: wide only if its median is below halves' at r160 and not above it at r128 beyond
          the min - max spread of the samples, else halves (DESIGN 4.4 holds the result).
  layer   E = 64, T = 4096, k = 2, M = H = 2048, capacity_factor 0, eager and graph-replayed:
            packed16_*      the 16-bit packed forward
            fp4_packed_*    the packed FP4 (W4A16) forward
            w4a8_packed_*   the packed W4A8 forward, in the library's default form

Prints one JSON line: per arm median / min / max in microseconds over --samples samples.

    python tools/packed_w4a8_bench.py [--what kernel layer] [--kinds ffn llama_ffn] [--samples 30] [--warmup 5] [--inner 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import packed_w8_bench as B  # noqa: E402

TILE_ENV = "TUTEL_AMD_W4A8_PACKED_TILE"
RUNS = ("r128", "r160")


def kernel_arms(ops, ep_native, w4):
    E, N, Kd = B.KERNEL["E"], B.KERNEL["N"], B.KERNEL["Kdim"]
    g = torch.Generator().manual_seed(E)
    w = (torch.randn([E, N, Kd], generator=g) / Kd ** 0.5).to(B.DT).cuda()
    bias = torch.randn([E, N], generator=g).to(B.DT).cuda()
    codes, scales = w4.prepare(w, True)
    del w
    arms = {}

    def formed(env, form, fn):
        def run():
            os.environ[env] = form
            return fn()
        return run

    for name, R in zip(RUNS, (128, 160)):
        lay = B.layout_of(ops, ep_native, [R] * E)
        a = (torch.randn([lay.rows_bound, Kd], generator=g) * 0.5).to(B.DT).cuda()
        q, s = ops.quantize_rows_a8(a)
        outs = [torch.empty([lay.rows_bound, N], dtype=B.DT, device="cuda") for _ in range(3)]
        qb, ob = q[:E * R].view(E, R, Kd), torch.empty([E, R, N], dtype=B.DT, device="cuda")
        for form, out in (("wide", outs[0]), ("halves", outs[1])):
            arms[f"w4a8_{form}_{name}"] = formed(TILE_ENV, form, lambda lay=lay, q=q, s=s, out=out: ops.expert_gemm_w4a8_packed(
                q, s, codes, scales, bias, N, Kd, B.DT, lay, act="relu", out=out))
        arms["w4a8_padded_" + name] = (lambda qb=qb, s=s[:E * R].contiguous(), ob=ob: ops.expert_gemm_w4a8(
            qb, s, codes, scales, bias, N, Kd, B.DT, act="relu", out=ob))
        arms["w4_halves_" + name] = formed("TUTEL_AMD_W4_PACKED_TILE", "halves", lambda lay=lay, a=a, o=outs[2]: ops.expert_gemm_w4_packed(
            a, codes, scales, bias, N, Kd, lay, act="relu", out=o))
        arms["quantize_" + name] = (lambda lay=lay, a=a, q=torch.empty_like(q), s=torch.empty_like(s): ops.quantize_rows_a8(
            a, out=q, scale=s, rows_dev=lay.offsets[E:]))
        # the same quantised rows, the same experts: the same bits, whichever form
        want = arms["w4a8_padded_" + name]()
        for form in ("wide", "halves"):
            assert torch.equal(arms[f"w4a8_{form}_{name}"]()[:E * R].view(E, R, N), want), form + ": packed rows differ from the padded kernel's"
    return arms


def layer_arms(kind):
    from tutel_amd.impls.graph import GraphedForward
    layer = B.make_layer(kind)
    x = torch.randn([B.LAYER["T"], B.LAYER["M"]], device="cuda").to(B.DT)
    ran = {}

    def setup(fmt):
        layer.dropless_packed = True
        layer.experts.fp4_weights = layer.dropless_packed_fp4 = fmt is not None
        layer.experts.w4a8 = layer.dropless_packed_w4a8 = fmt == "w4a8"

    def eager(name, fmt):
        def run():
            setup(fmt)
            with torch.no_grad():
                layer(x)
            ran[name] = (layer._dropless_packed_ran, layer._fp4_weights_ran, layer._w4a8_ran)
        return run

    def graphed(name, fmt):
        eager(name, fmt)()   # one eager forward: workspaces, cached images
        g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
        ran[name] = (layer._dropless_packed_ran, layer._fp4_weights_ran, layer._w4a8_ran)
        return lambda: g(x)

    arms = {}
    for fmt, stem in ((None, "packed16"), ("fp4", "fp4_packed"), ("w4a8", "w4a8_packed")):
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
        sys.exit("packed_w4a8_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    from tutel_amd.experts import w4
    from tutel_amd.impls import ep_native
    out = {"tool": "tools/packed_w4a8_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "samples": args.samples,
           "warmup": args.warmup, "inner": args.inner}
    if "kernel" in args.what:
        res = B.alternate(kernel_arms(ops, ep_native, w4), args.samples, args.warmup, args.inner)
        os.environ.pop(TILE_ENV, None)
        os.environ.pop("TUTEL_AMD_W4_PACKED_TILE", None)
        wide, halves = ({r: res[f"w4a8_{form}_{r}"] for r in RUNS} for form in ("wide", "halves"))
        # the rule of the docstring, on this run's samples
        pick_wide = (wide["r160"]["median_us"] < halves["r160"]["median_us"] and
                     wide["r128"]["median_us"] <= halves["r128"]["median_us"] + (halves["r128"]["max_us"] - halves["r128"]["min_us"]))
        out["kernel"] = dict(shape=B.KERNEL, arms=res, rule_picks="wide" if pick_wide else "halves",
                             wide_over_halves={r: round(wide[r]["median_us"] / halves[r]["median_us"], 3) for r in RUNS})
        torch.cuda.empty_cache()
    if "layer" in args.what:
        out["layer"] = {"shape": B.LAYER}
        for kind in args.kinds:
            arms, ran, layer = layer_arms(kind)
            res = B.alternate(arms, args.samples, args.warmup, 1)
            for stem, want in (("packed16", (True, None, None)), ("fp4_packed", (True, True, None)), ("w4a8_packed", (True, None, True))):
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
