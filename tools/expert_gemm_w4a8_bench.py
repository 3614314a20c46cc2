#!/usr/bin/env python3
"""What MXFP4 weights with FP8 activations on the block-scaled fp4 x fp8 matrix instruction (W4A8, csrc/expert_gemm_w4a8.hip +
csrc/quantize_a8.hip) cost against W4A16, W8A8 and the 16-bit launches, bf16:

  headline  E = 64 experts, 128 rows each, M = H = 2048   (the weight-streaming case)
  r1024     E = 8, 1024 rows each, M = H = 2048

Per shape, arms alternated sample by sample in ONE process, every sample timed with device events after a warm-up (the method and
the helpers of tools/expert_gemm_w8_bench.py):

  fc1       gathered from the tokens through top-2 routing's slot map: 16-bit  /  W4A16  /  W8A8  /  W4A8
  fc2       on the [E, R, H] buckets:                                  16-bit  /  W4A16  /  W8A8  /  W4A8
  gate_up   the SwiGLU gate / up launch on the [E, R, M] buckets:      16-bit (ops.expert_gemm_gate_up)  /  W4A16  /  W8A8  /  W4A8
  quantise  the two quantiser launches of a forward: the T tokens, the E * R hidden rows
  layer     the whole MOELayer forward (top-2, capacity_factor 1) with fp4_weights on and w4a8 off / on

Before anything is timed the W4A8 outputs are compared with W4A16's (the activations' quantisation error: reported, with a loose bar).
Prints one JSON line per shape.

    python tools/expert_gemm_w4a8_bench.py [--samples 30] [--warmup 5] [--inner 10] [--shapes headline r1024] [--no-layer] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from expert_gemm_w8_bench import DT, K, alternate  # noqa: E402

SHAPES = {"headline": dict(E=64, R=128, M=2048, H=2048), "r1024": dict(E=8, R=1024, M=2048, H=2048)}


def gemm_arms(ops, w8, w4, E, R, M, H):
    g = torch.Generator().manual_seed(E)
    T = E * R // K
    x = torch.randn([T, M], generator=g).to(DT).cuda()
    w1 = (torch.randn([E, H, M], generator=g) / M ** 0.5).to(DT).cuda()
    wu = (torch.randn([E, H, M], generator=g) / M ** 0.5).to(DT).cuda()
    w2 = (torch.randn([E, H, M], generator=g) / H ** 0.5).to(DT).cuda()     # [E, H, M_out] as stored
    b1, b2 = torch.randn([E, H], generator=g).to(DT).cuda(), torch.randn([E, M], generator=g).to(DT).cuda()
    smap = torch.cat([torch.randperm(T, generator=g), torch.randperm(T, generator=g) + T]).to(torch.int32).cuda()
    w2k = w2.transpose(1, 2).contiguous()
    i1, s1 = w8.prepare(w1, True)
    i2, s2 = w8.prepare(w2, False)
    igu, sgu = w8.prepare_gate_up(w1, wu, True)
    (c1, t1), (c2, t2), (cgu, tgu) = w4.prepare(w1, True), w4.prepare(w2, False), w4.prepare_gate_up(w1, wu, True)
    hid = ops.expert_gemm_gather(x, smap, w1, b1, True, "relu", R)
    xe = x[smap.long() % T].view(E, R, M).contiguous()   # the buckets, for the gate / up launch
    xq, sx = ops.quantize_rows_a8(x)
    hq, sh = ops.quantize_rows_a8(hid.view(-1, H))
    xeq, sxe = ops.quantize_rows_a8(xe.view(-1, M))
    hq3, xeq3 = hq.view(E, R, H), xeq.view(E, R, M)
    arms = {
        "fc1_16bit": lambda: ops.expert_gemm_gather(x, smap, w1, b1, True, "relu", R),
        "fc1_w4a16": lambda: ops.expert_gemm_w4(x, c1, t1, b1, H, M, act="relu", slot_map=smap, R=R),
        "fc1_w8a8": lambda: ops.expert_gemm_w8a8(xq, sx, i1, s1, b1, H, M, DT, act="relu", slot_map=smap, R=R),
        "fc1_w4a8": lambda: ops.expert_gemm_w4a8(xq, sx, c1, t1, b1, H, M, DT, act="relu", slot_map=smap, R=R),
        "fc2_16bit": lambda: ops.expert_gemm(hid, w2k, b2, True),
        "fc2_w4a16": lambda: ops.expert_gemm_w4(hid, c2, t2, b2, M, H),
        "fc2_w8a8": lambda: ops.expert_gemm_w8a8(hq3, sh, i2, s2, b2, M, H, DT),
        "fc2_w4a8": lambda: ops.expert_gemm_w4a8(hq3, sh, c2, t2, b2, M, H, DT),
        "gate_up_16bit": lambda: ops.expert_gemm_gate_up(xe, w1, wu, act="silu"),
        "gate_up_w4a16": lambda: ops.expert_gemm_w4_glu(xe, cgu, tgu, H, M, act="silu"),
        "gate_up_w8a8": lambda: ops.expert_gemm_w8a8_glu(xeq3, sxe, igu, sgu, H, M, DT, act="silu"),
        "gate_up_w4a8": lambda: ops.expert_gemm_w4a8_glu(xeq3, sxe, cgu, tgu, H, M, DT, act="silu"),
        "quantise_tokens": lambda: ops.quantize_rows_a8(x, out=xq, scale=sx),
        "quantise_hidden": lambda: ops.quantize_rows_a8(hid.view(-1, H), out=hq, scale=sh),
    }
    errs = {n: float((arms[n + "_w4a8"]().float() - arms[n + "_w4a16"]().float()).abs().max()) for n in ("fc1", "fc2", "gate_up")}
    print(f"# E={E} R={R} M={M} H={H}: max |w4a8 - w4a16|: {errs}", file=sys.stderr)
    assert all(v < 1.0 for v in errs.values()), errs
    return arms, errs


def layer_arms(E, R, M, H):
    from tutel import moe
    torch.manual_seed(E)
    old = torch.get_default_dtype()
    torch.set_default_dtype(DT)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 1.0},
                              experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H,
                                       "activation_fn": lambda t: torch.nn.functional.relu(t)}, model_dim=M)
    finally:
        torch.set_default_dtype(old)
    layer = layer.cuda().eval()
    layer.experts.fp4_weights = True
    x = torch.randn([E * R // K, M], device="cuda").to(DT)
    ran = {}

    def forward(on):
        def run():
            layer.experts.w4a8 = on
            with torch.no_grad():
                layer(x)
            ran[on] = layer._w4a8_ran
        return run
    return {"w4a8_off": forward(False), "w4a8_on": forward(True)}, ran


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-layer", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        sys.exit("expert_gemm_w4a8_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    from tutel_amd.experts import w4, w8
    lines = []
    for name in args.shapes:
        s = SHAPES[name]
        arms, errs = gemm_arms(ops, w8, w4, **s)
        entry = dict(tool="tools/expert_gemm_w4a8_bench.py", device=torch.cuda.get_device_name(0), dtype="bfloat16", name=name, shape=s,
                     samples=args.samples, warmup=args.warmup, inner=args.inner, max_abs_diff_w4a8_vs_w4a16=errs,
                     gemm=alternate(arms, args.samples, args.warmup, args.inner))
        del arms
        torch.cuda.empty_cache()
        if not args.no_layer:
            larms, ran = layer_arms(**s)
            entry["layer"] = alternate(larms, args.samples, args.warmup, 1)
            assert ran[True] is True, f"the switched-on layer did not run W4A8: {ran[True]}"
            del larms
            torch.cuda.empty_cache()
        lines.append(json.dumps(entry))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
