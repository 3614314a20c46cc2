#!/usr/bin/env python3
"""What streaming the expert weights as MXFP4 (W4A16, csrc/expert_gemm_w4.hip) costs against the 16-bit launches and the FP8 (W8A16)
launches it would replace, bf16:

  headline  E = 64 experts, 128 rows each, M = H = 2048   (the weight-streaming case the kernel is built for)
  r1024     E = 8, 1024 rows each, M = H = 2048           (MFMA-bound: the kernel streams the weights once per 128 rows)

Per shape, arms alternated sample by sample in ONE process (clock and thermal drift hit them alike), every sample timed with device
events after a warm-up, a sample being --inner back-to-back repetitions between one pair of events:

  fc1    gathered from the tokens through a slot map (top-2 routing's): ops.expert_gemm_gather (16-bit), ops.expert_gemm_w8, ops.expert_gemm_w4
  fc2    on the [E, R, H] buckets: ops.expert_gemm on the k-major copy (16-bit), ops.expert_gemm_w8, ops.expert_gemm_w4
  glu    (headline only) the SwiGLU gate / up launch on the buckets: ops.expert_gemm_w8_glu against ops.expert_gemm_w4_glu
  layer  the whole MOELayer forward (top-2, capacity_factor 1), experts.fp4_weights off -- the one-call pipeline -- and on (routing +
         two launches + decode: more launches, reported apart from the GEMM times)

Before anything is timed the w4 outputs are compared with the 16-bit GEMM run on the dequantised weights (exact in bf16).
Prints one JSON line: per arm median / min / max in microseconds, per GEMM arm its algorithmic bytes (weights + scales + rows in +
rows out) and the bandwidth at the median.

    python tools/expert_gemm_w4_bench.py [--samples 30] [--warmup 5] [--inner 10] [--shapes headline r1024] [--no-layer] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

SHAPES = {"headline": dict(E=64, R=128, M=2048, H=2048), "r1024": dict(E=8, R=1024, M=2048, H=2048)}
K = 2
DT = torch.bfloat16


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


def gemm_arms(ops, w4, w8, E, R, M, H, glu):
    g = torch.Generator().manual_seed(E)
    T = E * R // K
    x = torch.randn([T, M], generator=g).to(DT).cuda()
    w1 = (torch.randn([E, H, M], generator=g) / M ** 0.5).to(DT).cuda()
    w2 = (torch.randn([E, H, M], generator=g) / H ** 0.5).to(DT).cuda()     # [E, H, M_out] as stored
    b1, b2 = torch.randn([E, H], generator=g).to(DT).cuda(), torch.randn([E, M], generator=g).to(DT).cuda()
    # top-2 routing's slot map with every bucket full: row (e, r) reads one of the T tokens, each token read twice
    smap = torch.cat([torch.randperm(T, generator=g), torch.randperm(T, generator=g) + T]).to(torch.int32).cuda()
    w2k = w2.transpose(1, 2).contiguous()
    i1, s1 = w8.prepare(w1, True)
    i2, s2 = w8.prepare(w2, False)
    q1, q2 = w4.quantize_mxfp4(w1, True), w4.quantize_mxfp4(w2, False)
    (c1, t1), (c2, t2) = w4.pack(*q1), w4.pack(*q2)
    hid = ops.expert_gemm_gather(x, smap, w1, b1, True, "relu", R)
    arms = dict(
        fc1_16bit=lambda: ops.expert_gemm_gather(x, smap, w1, b1, True, "relu", R),
        fc1_w8=lambda: ops.expert_gemm_w8(x, i1, s1, b1, H, M, act="relu", slot_map=smap, R=R),
        fc1_w4=lambda: ops.expert_gemm_w4(x, c1, t1, b1, H, M, act="relu", slot_map=smap, R=R),
        fc2_16bit=lambda: ops.expert_gemm(hid, w2k, b2, True),
        fc2_w8=lambda: ops.expert_gemm_w8(hid, i2, s2, b2, M, H),
        fc2_w4=lambda: ops.expert_gemm_w4(hid, c2, t2, b2, M, H))
    # faster and different is not faster: against the 16-bit kernel on the dequantised weights (exact in bf16; the two kernels sum in
    # different orders, so a bar of a few bf16 ulps of the output scale)
    d1, d2 = w4.dequantize(*q1, DT), w4.dequantize(*q2, DT)
    e1 = float((arms["fc1_w4"]().float() - ops.expert_gemm_gather(x, smap, d1, b1, True, "relu", R).float()).abs().max())
    e2 = float((arms["fc2_w4"]().float() - ops.expert_gemm(hid, d2, b2, True).float()).abs().max())
    print(f"# E={E} R={R} M={M} H={H}: max |w4 - 16-bit on dequantised weights|: fc1 {e1:.3g}, fc2 {e2:.3g}", file=sys.stderr)
    assert e1 < 0.25 and e2 < 0.25, (e1, e2)
    rows = 2 * E * R * (M + H)            # rows in + rows out, 2 bytes each, per GEMM (M_out = M)
    w = E * H * M
    algo = dict(fc1_16bit=2 * w + rows, fc1_w8=w + 4 * E * H + rows, fc1_w4=w // 2 + w // 32 + rows,
                fc2_16bit=2 * w + rows, fc2_w8=w + 4 * E * M + rows, fc2_w4=w // 2 + w // 32 + rows)
    if glu:
        wu = (torch.randn([E, H, M], generator=g) / M ** 0.5).to(DT).cuda()
        xb = torch.randn([E, R, M], generator=g).to(DT).cuda()
        ig, sg = w8.prepare_gate_up(w1, wu, True)
        cg, tg = w4.prepare_gate_up(w1, wu, True)
        arms["glu_w8"] = lambda: ops.expert_gemm_w8_glu(xb, ig, sg, H, M, act="silu")
        arms["glu_w4"] = lambda: ops.expert_gemm_w4_glu(xb, cg, tg, H, M, act="silu")
        algo["glu_w8"] = 2 * w + 8 * E * H + rows
        algo["glu_w4"] = w + w // 16 + rows
    return arms, algo, (e1, e2)


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
    x = torch.randn([E * R // K, M], device="cuda").to(DT)
    ran = {}

    def forward(on):
        def run():
            layer.experts.fp4_weights = on
            with torch.no_grad():
                layer(x)
            ran[on] = layer._fp4_weights_ran
        return run
    return {"switch_off": forward(False), "switch_on": forward(True)}, ran


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
        sys.exit("expert_gemm_w4_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    from tutel_amd.experts import w4, w8
    out = {"tool": "tools/expert_gemm_w4_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16",
           "samples": args.samples, "warmup": args.warmup, "inner": args.inner, "shapes": {}}
    for name in args.shapes:
        s = SHAPES[name]
        arms, algo, errs = gemm_arms(ops, w4, w8, glu=(name == "headline"), **s)
        res = alternate(arms, args.samples, args.warmup, args.inner)
        for arm, nbytes in algo.items():
            res[arm].update(algorithmic_bytes=nbytes, tb_per_s=round(nbytes / (res[arm]["median_us"] * 1e-6) / 1e12, 3))
        entry = dict(shape=s, tokens=s["E"] * s["R"] // K, max_abs_diff_vs_16bit_on_dequantised=errs, gemm=res)
        for fc in ("fc1", "fc2"):
            entry[fc + "_w4_over_16bit"] = round(res[fc + "_w4"]["median_us"] / res[fc + "_16bit"]["median_us"], 3)
            entry[fc + "_w4_over_w8"] = round(res[fc + "_w4"]["median_us"] / res[fc + "_w8"]["median_us"], 3)
        if "glu_w4" in res:
            entry["glu_w4_over_w8"] = round(res["glu_w4"]["median_us"] / res["glu_w8"]["median_us"], 3)
        del arms
        torch.cuda.empty_cache()
        if not args.no_layer and name == "headline":
            larms, ran = layer_arms(**s)
            entry["layer"] = alternate(larms, args.samples, args.warmup, 1)
            assert ran[True] is True, f"the switched-on layer did not read FP4 weights: {ran[True]}"
            entry["layer_on_over_off"] = round(entry["layer"]["switch_on"]["median_us"] / entry["layer"]["switch_off"]["median_us"], 3)
            del larms
            torch.cuda.empty_cache()
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
