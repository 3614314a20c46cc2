#!/usr/bin/env python3
"""What the native projection of an fp32 gate costs and saves, at the headline shape (T = 4096, M = 2048, top-2, bf16 tokens,
fp32 gate weight; E = 64 and E = 128).  Two comparisons, each with its arms alternated sample by sample in ONE process so that
clock and thermal drift hit them alike, every sample timed with device events after a warm-up:

  routing   (a) x.float() + F.linear + gate_topk            -- what an fp32-gate layer runs today
            (b) gate_proj_f32w + gate_topk_partials(fp32)   -- the new kernel and its consumer
            a sample is --inner back-to-back repetitions between one pair of events (the kernels are tens of microseconds)
  layer     the whole MOELayer forward (H = 2048, capacity_factor 1), switch _NATIVE_GATE_FP32 off and on; off is the code
            path of the commit before the switch existed, unchanged

Prints one JSON line: per arm the median, minimum and maximum of the samples in microseconds, and the algorithmic bytes / FLOP
of the projection.  --tree PATH imports the package from another checkout instead (one built from an older commit: the arms it
does not have are reported as null), which is how a figure is confirmed against the parent commit itself.

    python tools/gate_fp32_bench.py [--samples 40] [--warmup 10] [--inner 20] [--experts 64 128] [--tree PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

T, M, H, K = 4096, 2048, 2048, 2


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


def routing_arms(ops, E):
    g = torch.Generator().manual_seed(E)
    x = torch.randn([T, M], generator=g).to(torch.bfloat16).cuda()
    wg = (torch.randn([E, M], generator=g) / M ** 0.5).cuda()
    ws = ops.routing_workspace(T, E, K, x.device)

    def parent():
        ops.gate_topk(torch.nn.functional.linear(x.float(), wg), K, apply_softmax=True, ws=ws)
    arms = {"float_linear_topk": parent}
    if hasattr(ops, "gate_proj_f32w"):
        S = ops.gate_proj_f32w_splits(T, M, E, x.dtype)
        part = torch.empty([S, T, E], dtype=torch.float32, device=x.device)

        def native():
            ops.gate_topk_partials(ops.gate_proj_f32w(x, wg, partials=part), torch.float32, K, ws=ws)

        def kernel_only():
            ops.gate_proj_f32w(x, wg, partials=part)
        arms.update(proj_f32w_topk_partials=native, proj_f32w_alone=kernel_only)
        # faster and different is not faster: the two routes must pick the same experts wherever the scores leave no near-tie
        idx_a = ops.gate_topk(torch.nn.functional.linear(x.float(), wg), K, apply_softmax=True)[0]
        idx_b, _, _, logits, _ = ops.gate_topk_partials(ops.gate_proj_f32w(x, wg), torch.float32, K, want_logits=True)
        err = float((logits.double() - x.double() @ wg.double().t()).abs().max())
        print(f"# E={E}: splits {S}, rows routed differently {int((idx_a != idx_b).any(0).sum())} of {T}, "
              f"max |logit - fp64| {err:.3g}", file=sys.stderr)
    return arms


def layer_arms(E):
    from tutel import moe
    from tutel_amd.impls import moe_layer as ML
    torch.manual_seed(E)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 1.0, "fp32_gate": True},
                              experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H,
                                       "activation_fn": lambda t: torch.nn.functional.relu(t)}, model_dim=M)
    finally:
        torch.set_default_dtype(old)
    layer = layer.cuda().eval()
    x = torch.randn([T, M], device="cuda").to(torch.bfloat16)

    def forward(on):
        def run():
            if hasattr(ML, "_NATIVE_GATE_FP32"):
                ML._NATIVE_GATE_FP32 = on
            with torch.no_grad():
                layer(x)
        return run
    arms = {"switch_off": forward(False)}
    if hasattr(ML, "_NATIVE_GATE_FP32"):
        arms["switch_on"] = forward(True)
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--experts", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        sys.exit("gate_fp32_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import _lib, ops
    out = {"tool": "tools/gate_fp32_bench.py", "tree": os.path.relpath(os.path.dirname(os.path.dirname(_lib.LIB_PATH))),
           "device": torch.cuda.get_device_name(0), "shape": dict(T=T, M=M, H=H, k=K, tokens="bfloat16", gate="float32"),
           "samples": args.samples, "warmup": args.warmup, "inner": args.inner, "routing": {}, "layer": {}}
    for E in args.experts:
        out["routing"][str(E)] = alternate(routing_arms(ops, E), args.samples, args.warmup, args.inner)
        out["routing"][str(E)]["projection_needs"] = dict(flop=2 * T * M * E, token_bytes=2 * T * M, weight_bytes=4 * E * M)
        out["layer"][str(E)] = alternate(layer_arms(E), args.samples, args.warmup, 1)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
