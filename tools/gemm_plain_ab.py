"""In-process A/B of the PLAIN ring GEMM kernel on the headline forward (bench.py's layer and tokens): the forward is captured twice,
once with tutel_amd_gemm_plain(0) (the general kernel) and once with (1), and the two HIP graphs are replayed interleaved -- arm 0,
arm 1, arm 0, ... -- in regions of `--steps` replays between HIP events.  Prints one JSON line: per arm the median and the spread of
the region means, the difference, and whether the two arms return the same bits.

    python tools/gemm_plain_ab.py [--regions 5] [--steps 20] [--warmup 5]
    python tools/gemm_plain_ab.py --arm 1 --steps 60        one arm only, no timing: the run to put under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arm", type=int, default=None, choices=[0, 1])
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    args = ap.parse_args()
    from tutel_amd import ops
    from tutel_amd.impls.graph import GraphedForward
    T, M, H, E, k = 4096, 2048, 2048, 64, 2
    dtype, dev = getattr(torch, args.dtype), torch.device("cuda", 0)
    layer = bench.build_layer(M, H, E, k, 0, 1, dtype, False).to(dev).eval()
    torch.manual_seed(0)
    x = torch.randn([16, T // 16, M], dtype=torch.float32).to(dtype).to(dev)
    was = ops.gemm_plain(-2)
    graphs, forms, outs = {}, {}, {}
    try:
        for arm in ([args.arm] if args.arm is not None else [0, 1]):
            ops.gemm_plain(arm)
            n0 = ops.expert_gemm_last_form()[1]
            with torch.no_grad():
                graphs[arm] = GraphedForward(layer, x)
            n1 = ops.expert_gemm_last_form()[1]
            forms[arm] = [n1[0] - n0[0], n1[1] - n0[1]]     # launches enqueued while warming up and capturing: general, PLAIN
            outs[arm] = graphs[arm](x).clone()
    finally:
        ops.gemm_plain(was)
    torch.cuda.synchronize()
    if args.arm is not None:
        for _ in range(args.steps):
            graphs[args.arm](x)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "gemm_plain_ab", "arm": args.arm, "replays": args.steps, "launches_general_plain": forms[args.arm]}), flush=True)
        return
    ms = {0: [], 1: []}
    for _ in range(args.regions):
        for arm in (0, 1):
            for _ in range(args.warmup):
                graphs[arm](x)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                graphs[arm](x)
            b.record()
            b.synchronize()
            ms[arm].append(a.elapsed_time(b) / args.steps)
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    print(json.dumps({
        "tool": "gemm_plain_ab", "shape": dict(T=T, M=M, H=H, E=E, k=k, dtype=args.dtype), "regions": args.regions, "steps": args.steps,
        "ms_per_step_general": [round(v, 5) for v in ms[0]], "ms_per_step_plain": [round(v, 5) for v in ms[1]],
        "median_general": round(med[0], 5), "median_plain": round(med[1], 5), "plain_minus_general_us": round((med[1] - med[0]) * 1e3, 2),
        "spread_general_us": round((max(ms[0]) - min(ms[0])) * 1e3, 2), "spread_plain_us": round((max(ms[1]) - min(ms[1])) * 1e3, 2),
        "launches_general_plain": forms, "same_bits": bool(torch.equal(outs[0], outs[1])),
    }), flush=True)


if __name__ == "__main__":
    main()
