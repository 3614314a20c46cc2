#!/usr/bin/env python3
"""SwiGLU experts on the packed dropless layout at the BASELINE configs[2] shape (T = 4096, M = H = 2048, E = 64, top-2,
capacity_factor = 0, megablocks_size = 4, bf16; experts={'type': 'llama_ffn'}).

    python tools/swiglu_packed_bench.py [--steps 50] [--warmup 10]
        device-event times (ms per forward, median of --steps) of the eager padded dropless forward, the eager packed forward and the
        graph-replayed packed forward; one JSON line

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/swiglu_packed_bench.py --trace [--steps 20]
    python tools/swiglu_packed_bench.py --summarize OUT/.../*_kernel_trace.csv
        the fused gate/up kernel of the packed forward against the pair it replaces in the padded forward (the act GEMM on W_fc1 and
        the gated GEMM on W_fc2), per-dispatch microseconds from the kernel trace; one JSON line

--trace runs --steps padded forwards, synchronises, then --steps packed forwards: in the trace the padded forward's expert GEMMs come
in threes (act, gated, W_fc3), the packed forward's in twos (gate/up, W_fc3); the gate/up kernel is the ping-pong instantiation whose
last template argument (GATE_UP) is true.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T, M, H, E, K, MEGA = 4096, 2048, 2048, 64, 2, 4


def build_layer(dtype):
    import torch
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 0.0},
                              experts={"type": "llama_ffn", "num_experts_per_device": E, "hidden_size_per_expert": H}, model_dim=M)
    finally:
        torch.set_default_dtype(old)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        ex = layer.experts
        ex.W_fc1.copy_((torch.randn([E, M, H], generator=g) / M ** 0.5).reshape(-1))
        ex.W_fc2.copy_((torch.randn([E, M, H], generator=g) / M ** 0.5).reshape(-1))
        ex.W_fc3.copy_((torch.randn([E, H, M], generator=g) / H ** 0.5).reshape(-1))
    return layer.cuda().eval()


def time_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def run(args):
    import torch
    from tutel_amd.impls.graph import GraphedForward
    torch.manual_seed(0)
    layer = build_layer(torch.bfloat16)
    x = torch.randn(T, M, device="cuda", dtype=torch.bfloat16)

    def fwd(packed):
        layer.dropless_packed = packed
        with torch.no_grad():
            y = layer(x, megablocks_size=MEGA)
        return y

    if args.trace:
        for _ in range(args.steps):
            fwd(False)
        torch.cuda.synchronize()
        for _ in range(args.steps):
            fwd(True)
        torch.cuda.synchronize()
        assert layer._dropless_packed_ran is True, layer._dropless_packed_ran
        print(json.dumps({"trace": "done", "steps": args.steps}))
        return
    res = {"tool": "swiglu_packed_bench", "shape": {"T": T, "M": M, "H": H, "E": E, "k": K, "megablocks_size": MEGA, "dtype": "bf16"}}
    res["padded_eager"] = time_ms(lambda: fwd(False), args.steps, args.warmup)
    res["packed_eager"] = time_ms(lambda: fwd(True), args.steps, args.warmup)
    assert layer._dropless_packed_ran is True, layer._dropless_packed_ran
    same = torch.equal(fwd(False), fwd(True).clone())
    layer.dropless_packed = False
    g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True, megablocks_size=MEGA)
    res["packed_graph"] = time_ms(lambda: g(x), args.steps, args.warmup)
    res["packed_equals_padded"] = bool(same and torch.equal(g(x), fwd(False)))
    print(json.dumps(res))


def summarize(path):
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "expert_gemm" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    gate_up = [i for i, r in enumerate(rows) if r["Kernel_Name"].replace(" ", "").endswith(",true>(GemmArgs)")]
    assert gate_up, "no gate/up kernel in the trace"
    first = gate_up[0]
    assert first % 3 == 0, "the padded forwards' expert GEMMs should come in threes"
    act = [us[i] for i in range(0, first, 3)]
    glu = [us[i] for i in range(1, first, 3)]
    fc3_padded = [us[i] for i in range(2, first, 3)]
    fused = [us[i] for i in gate_up]
    fc3_packed = [us[i + 1] for i in gate_up if i + 1 < len(us)]
    med = statistics.median
    out = {"tool": "swiglu_packed_bench --summarize", "dispatches": {"padded_forwards": len(act), "packed_forwards": len(fused)},
           "padded_act_gemm_us": med(act), "padded_glu_gemm_us": med(glu), "padded_pair_us": med([a + b for a, b in zip(act, glu)]),
           "packed_gate_up_us": med(fused), "padded_fc3_us": med(fc3_padded), "packed_fc3_us": med(fc3_packed),
           "kernels": {"act": rows[0]["Kernel_Name"], "glu": rows[1]["Kernel_Name"], "gate_up": rows[first]["Kernel_Name"]}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--trace", action="store_true", help="padded then packed forwards, for a rocprofv3 kernel trace")
    ap.add_argument("--summarize", metavar="KERNEL_TRACE_CSV", help="gate/up kernel vs the act + gated pair from a kernel trace")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
    else:
        run(args)


if __name__ == "__main__":
    main()
