#!/usr/bin/env python3
"""What the native fp32 grouped GEMM (csrc/expert_gemm_f32.hip) costs against what it replaces, at two shapes:

  c0        BASELINE configs[0]: E = 2 experts, 1024 rows each, M = 2048, H = 128          (fp32)
  headline  the headline shape in fp32: E = 64, 128 rows each, M = H = 2048

Two comparisons per shape, each with its arms alternated sample by sample in ONE process so that clock and thermal drift hit them
alike, every sample timed with device events after a warm-up:

  ffn    on the same [E, R, M] buckets
         (a) torch.matmul + bias + relu + torch.matmul + bias   -- the five ATen launches of FusedExpertsNetwork.forward
         (b) two launches of tutel_amd_expert_gemm_f32           -- fc1 k-major with bias + relu, fc2 n-major with bias
         and each product alone: (a1) matmul + bias + relu against (b1) fc1, (a2) matmul + bias against (b2) fc2.
         A sample is --inner back-to-back repetitions between one pair of events.
  layer  the whole MOELayer forward (top-2, capacity_factor 1, T = E * rows / 2 tokens), switch _NATIVE_FP32 off and on; off is the
         code path of the commit before the switch existed

Before anything is timed the two routes are compared on the timed operands (max |native - ATen| over the output scale).
Prints one JSON line: per arm the median, minimum and maximum of the samples in microseconds; per native arm its FLOP, the TFLOP/s
at the median and that as a fraction of the 157 TFLOP/s fp32-matrix peak (for the kernel arms this is the kernel's share of peak --
the products are compute-bound at both shapes: FLOP / 157 TF exceeds bytes / 8 TB/s); the layer arms are end-to-end times.

    python tools/expert_gemm_f32_bench.py [--samples 30] [--warmup 5] [--inner 10] [--shapes c0 headline] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

PEAK_TF = 157.0   # fp32 matrix (v_mfma_f32_32x32x2_f32): 256 CUs x 4 SIMDs x 64 FLOP / clk x 2.4 GHz
SHAPES = {"c0": dict(E=2, R=1024, M=2048, H=128), "headline": dict(E=64, R=128, M=2048, H=2048)}
K = 2


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner   # microseconds per repetition


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


def ffn_arms(ops, E, R, M, H):
    g = torch.Generator().manual_seed(E)
    x = torch.randn([E, R, M], generator=g).cuda()
    w1 = (torch.randn([E, H, M], generator=g) / M ** 0.5).cuda()
    w2 = (torch.randn([E, H, M], generator=g) / H ** 0.5).cuda()
    b1, b2 = torch.randn([E, H], generator=g).cuda(), torch.randn([E, M], generator=g).cuda()
    w1t, b1u, b2u = w1.permute(0, 2, 1), b1.unsqueeze(1), b2.unsqueeze(1)
    hid = torch.relu(torch.matmul(x, w1t) + b1u)

    def aten_fc1():
        return torch.relu(torch.matmul(x, w1t) + b1u)

    def aten_fc2():
        return torch.matmul(hid, w2) + b2u

    def aten_ffn():
        return torch.matmul(torch.relu(torch.matmul(x, w1t) + b1u), w2) + b2u

    def native_fc1():
        return ops.expert_gemm_f32(x, w1, b1, True, act="relu")

    def native_fc2():
        return ops.expert_gemm_f32(hid, w2, b2, False)

    def native_ffn():
        return ops.expert_gemm_f32(ops.expert_gemm_f32(x, w1, b1, True, act="relu"), w2, b2, False)
    # faster and different is not faster
    ya, yn = aten_ffn(), native_ffn()
    err = float((ya.double() - yn.double()).abs().max()) / max(1.0, float(ya.abs().max()))
    print(f"# E={E} R={R} M={M} H={H}: max |native - ATen| / max(1, |y|_inf) = {err:.3g}", file=sys.stderr)
    arms = dict(aten_fc1=aten_fc1, native_fc1=native_fc1, aten_fc2=aten_fc2, native_fc2=native_fc2, aten_ffn=aten_ffn, native_ffn=native_ffn)
    flop = 2 * E * R * M * H
    return arms, dict(native_fc1=flop, native_fc2=flop, native_ffn=2 * flop), err


def layer_arms(E, R, M, H):
    from tutel import moe
    from tutel_amd.experts import ffn
    torch.manual_seed(E)
    layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 1.0},
                          experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H,
                                   "activation_fn": lambda t: torch.nn.functional.relu(t)}, model_dim=M)
    layer = layer.cuda().eval()
    x = torch.randn([E * R // K, M], device="cuda")
    ran = {}

    def forward(on):
        def run():
            ffn._NATIVE_FP32 = on
            with torch.no_grad():
                layer(x)
            ran[on] = layer._native_fp32_ran
        return run
    return {"switch_off": forward(False), "switch_on": forward(True)}, ran


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        sys.exit("expert_gemm_f32_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    out = {"tool": "tools/expert_gemm_f32_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "float32", "peak_tflops": PEAK_TF,
           "samples": args.samples, "warmup": args.warmup, "inner": args.inner, "shapes": {}}
    for name in args.shapes:
        s = SHAPES[name]
        arms, flops, err = ffn_arms(ops, **s)
        res = alternate(arms, args.samples, args.warmup, args.inner)
        for arm, flop in flops.items():
            tf = flop / (res[arm]["median_us"] * 1e-6) / 1e12
            res[arm].update(flop=flop, tflops=round(tf, 1), fraction_of_fp32_matrix_peak=round(tf / PEAK_TF, 3))
        larms, ran = layer_arms(**s)
        layer = alternate(larms, args.samples, args.warmup, 1)
        assert ran[True] is True, f"the switched-on layer did not run natively: {ran[True]}"
        out["shapes"][name] = dict(shape=s, tokens=s["E"] * s["R"] // K, max_rel_diff_vs_aten=err, ffn=res, layer=layer)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
