#!/usr/bin/env python3
"""What MXFP4 expert weights cost on the PACKED dropless forward (layer.dropless_packed_fp4; impls/packed_w8.py under its FP4 format,
the W4A16 GEMMs over the packed tables of csrc/expert_gemm_w4.hip), bf16, in ONE process; the helpers are tools/packed_w8_bench.py's.

  kernel  tutel_amd_expert_gemm_w4_packed (N = K = 2048, bias + ReLU, plain rows) on synthesised layouts of 64 experts x 128 rows (r128)
          and 64 x 160 rows (r160), arms alternated sample by sample:
            w4_wide_*      one work item per 256-row table tile (TUTEL_AMD_W4_PACKED_TILE=wide; the variable is read at every call)
            w4_halves_*    two 128-row halves per table tile (TUTEL_AMD_W4_PACKED_TILE=halves)
            w4_padded_*    the padded tutel_amd_expert_gemm_w4 on [64, R, K]
            packed16_*     the 16-bit packed GEMM (tutel_amd_expert_gemm_packed, k-major) on the same layout
          This A/B decides the library's default form: wide if it is faster than halves at r160 and not slower at r128 beyond the
          spread, else halves (measured: halves).
  layer   E = 64, T = 4096, k = 2, M = H = 2048, capacity_factor 0, `ffn` and `llama_ffn` experts:
            fp4_padded_eager                      experts.fp4_weights on the padded layout (the capacity is read back to the host)
            fp4_packed_eager / fp4_packed_graph   the packed FP4 forward (the library's default form), eager and graph-replayed
            packed16_graph / fp8_packed_graph     the 16-bit and the FP8 packed forwards, graph-replayed

Prints one JSON line: per arm median / min / max in microseconds over --samples samples.

    python tools/packed_w4_bench.py [--what kernel layer] [--samples 30] [--warmup 5] [--inner 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import packed_w8_bench as B  # noqa: E402

TILE_ENV = "TUTEL_AMD_W4_PACKED_TILE"


def kernel_arms(ops, ep_native, w4):
    E, N, Kd = B.KERNEL["E"], B.KERNEL["N"], B.KERNEL["Kdim"]
    g = torch.Generator().manual_seed(E)
    w = (torch.randn([E, N, Kd], generator=g) / Kd ** 0.5).to(B.DT).cuda()
    bias = torch.randn([E, N], generator=g).to(B.DT).cuda()
    codes, scales = w4.prepare(w, True)
    arms = {}

    def formed(form, fn):
        def run():
            os.environ[TILE_ENV] = form
            return fn()
        return run

    for name, R in (("r128", 128), ("r160", 160)):
        lay = B.layout_of(ops, ep_native, [R] * E)
        a = (torch.randn([lay.rows_bound, Kd], generator=g) * 0.5).to(B.DT).cuda()
        outs = [torch.empty([lay.rows_bound, N], dtype=B.DT, device="cuda") for _ in range(3)]
        ab, ob = a[:E * R].view(E, R, Kd), torch.empty([E, R, N], dtype=B.DT, device="cuda")
        for form, out in (("wide", outs[0]), ("halves", outs[1])):
            arms[f"w4_{form}_{name}"] = formed(form, lambda lay=lay, a=a, out=out: ops.expert_gemm_w4_packed(a, codes, scales, bias, N, Kd, lay,
                                                                                                            act="relu", out=out))
        arms["w4_padded_" + name] = (lambda ab=ab, ob=ob: ops.expert_gemm_w4(ab, codes, scales, bias, N, Kd, act="relu", out=ob))
        arms["packed16_" + name] = (lambda lay=lay, a=a, o=outs[2]: ops.expert_gemm_packed(a, w, bias, True, lay, act="relu", out=o))
        # the same rows, the same experts: the same bits, whichever form
        want = arms["w4_padded_" + name]()
        for form in ("wide", "halves"):
            assert torch.equal(arms[f"w4_{form}_{name}"]()[:E * R].view(E, R, N), want), form + ": packed rows differ from the padded kernel's"
    return arms


def layer_arms(kind):
    from tutel_amd.impls.graph import GraphedForward
    layer = B.make_layer(kind)
    x = torch.randn([B.LAYER["T"], B.LAYER["M"]], device="cuda").to(B.DT)
    ran = {}

    def setup(fmt, packed):
        layer.experts.fp8_weights, layer.experts.fp4_weights, layer.dropless_packed = fmt == "fp8", fmt == "fp4", packed
        layer.dropless_packed_fp8 = layer.dropless_packed_fp4 = packed

    def eager(name, fmt, packed):
        def run():
            setup(fmt, packed)
            with torch.no_grad():
                layer(x)
            ran[name] = (layer._dropless_packed_ran, layer._fp8_weights_ran, layer._fp4_weights_ran)
        return run

    def graphed(name, fmt):
        setup(fmt, True)
        with torch.no_grad():
            layer(x)   # one eager forward: workspaces, cached images
        g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
        ran[name] = (layer._dropless_packed_ran, layer._fp8_weights_ran, layer._fp4_weights_ran)
        return lambda: g(x)

    arms = {"fp4_padded_eager": eager("fp4_padded_eager", "fp4", False), "fp4_packed_eager": eager("fp4_packed_eager", "fp4", True),
            "fp4_packed_graph": graphed("fp4_packed_graph", "fp4"), "packed16_graph": graphed("packed16_graph", None),
            "fp8_packed_graph": graphed("fp8_packed_graph", "fp8")}
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
        sys.exit("packed_w4_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    from tutel_amd.experts import w4
    from tutel_amd.impls import ep_native
    out = {"tool": "tools/packed_w4_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "samples": args.samples,
           "warmup": args.warmup, "inner": args.inner}
    if "kernel" in args.what:
        res = B.alternate(kernel_arms(ops, ep_native, w4), args.samples, args.warmup, args.inner)
        os.environ.pop(TILE_ENV, None)
        out["kernel"] = dict(shape=B.KERNEL, arms=res,
                             wide_over_halves={r: round(res[f"w4_wide_{r}"]["median_us"] / res[f"w4_halves_{r}"]["median_us"], 3) for r in ("r128", "r160")})
        torch.cuda.empty_cache()
    if "layer" in args.what:
        out["layer"] = {"shape": B.LAYER}
        for kind in args.kinds:
            arms, ran, layer = layer_arms(kind)
            res = B.alternate(arms, args.samples, args.warmup, 1)
            assert ran["fp4_padded_eager"][2] is True and ran["packed16_graph"][0] is True, ran
            assert ran["fp4_packed_eager"][::2] == (True, True) and ran["fp4_packed_graph"][::2] == (True, True), ran
            assert ran["fp8_packed_graph"][:2] == (True, True), ran
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
