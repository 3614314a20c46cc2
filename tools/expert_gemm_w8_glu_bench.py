#!/usr/bin/env python3
"""What streaming a SwiGLU expert's weights as FP8 (W8A16; csrc/expert_gemm_w8.hip, tutel_amd_expert_gemm_w8_glu) costs against the
16-bit launches it replaces, bf16:

  headline  E = 64 experts, 128 rows each, M = H = 2048     (the weight-streaming case the kernel is built for)
  r1024     E = 8, 1024 rows each, M = H = 2048             (MFMA-bound: the w8 kernel streams the weights once per 128 rows and is
                                                            known to lose there)

Per shape, arms alternated sample by sample in ONE process (clock and thermal drift hit them alike), every sample timed with device
events after a warm-up, a sample being --inner back-to-back repetitions between one pair of events:

  gate_up  on the [E, R, M] buckets: ops.expert_gemm_gate_up on the k-major copies (16-bit, one launch)   against  ops.expert_gemm_w8_glu
  ffn      the whole expert: LlamaFFNNetwork.forward_fused (16-bit, three launches)   against   forward_fused_w8 (two launches)
  layer    the whole MOELayer forward (llama_ffn experts, top-2, capacity_factor 1), experts.fp8_weights off and on

Before anything is timed the FP8 outputs are compared with the 16-bit launch run on the dequantised weights rounded to bf16.
Prints one JSON line: per arm median / min / max in microseconds, per gate_up arm its algorithmic bytes (weights + rows in + rows
out + scales) and the bandwidth at the median.

    python tools/expert_gemm_w8_glu_bench.py [--samples 30] [--warmup 5] [--inner 10] [--shapes headline r1024] [--no-layer] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from expert_gemm_w8_bench import alternate   # noqa: E402  (the same timing loop)

SHAPES = {"headline": dict(E=64, R=128, M=2048, H=2048), "r1024": dict(E=8, R=1024, M=2048, H=2048)}
K = 2
DT = torch.bfloat16


class _Ctx:
    group = None


def expert_arms(ops, w8, E, R, M, H):
    from tutel_amd.experts.llama_ffn import LlamaFFNNetwork
    g = torch.Generator().manual_seed(E)
    x = (torch.randn([E, R, M], generator=g) * 0.5).to(DT).cuda()
    net = LlamaFFNNetwork(M, H, E, 1).to(DT)
    with torch.no_grad():
        net.W_fc1.copy_((torch.randn([E, M, H], generator=g) / M ** 0.5).reshape(-1))
        net.W_fc2.copy_((torch.randn([E, M, H], generator=g) / M ** 0.5).reshape(-1))
        net.W_fc3.copy_((torch.randn([E, H, M], generator=g) / H ** 0.5).reshape(-1))
    net = net.cuda().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    act = net.fused_activation()
    wg, wu, _ = net.kmajor_weights()
    (igu, sgu), _ = net.w8_params()

    def gate_up_16():
        return ops.expert_gemm_gate_up(x, wg, wu, act=act)

    def gate_up_w8():
        return ops.expert_gemm_w8_glu(x, igu, sgu, H, M, act=act)

    def ffn_16():
        return net.forward_fused(x)

    def ffn_w8():
        return net.forward_fused_w8(x)
    # faster and different is not faster: against the 16-bit launches on the dequantised weights (rounded to bf16: not exact, so a
    # bar of a few bf16 ulps of the output scale)
    qg, qu = w8.deinterleave_gate_up(w8.unpack(igu, 2 * H, M))
    sg, su = w8.deinterleave_gate_up(sgu)
    dg, du = w8.dequantize(qg, sg, DT), w8.dequantize(qu, su, DT)
    e1 = float((gate_up_w8().float() - ops.expert_gemm_gate_up(x, dg, du, act=act).float()).abs().max())
    q3, s3 = w8.quantize_e4m3(net.W_fc3.view(net.W_fc3_full_shape), False)
    h = ops.expert_gemm_gate_up(x, dg, du, act=act)
    e2 = float((ffn_w8().float() - ops.expert_gemm(h, w8.dequantize(q3, s3, DT), None, True).float()).abs().max())
    print(f"# E={E} R={R} M={M} H={H}: max |w8 - 16-bit on dequantised weights|: gate_up {e1:.3g}, ffn {e2:.3g}", file=sys.stderr)
    assert e1 < 0.25 and e2 < 0.25, (e1, e2)
    rows = 2 * E * R * (M + H)                 # rows in + rows out, 2 bytes each
    arms = dict(gate_up_16bit=gate_up_16, gate_up_w8=gate_up_w8, ffn_16bit=ffn_16, ffn_w8=ffn_w8)
    algo = dict(gate_up_16bit=2 * 2 * E * H * M + rows, gate_up_w8=2 * E * H * M + rows + 4 * E * 2 * H)
    return arms, algo, (e1, e2)


def layer_arms(E, R, M, H):
    from tutel import moe
    torch.manual_seed(E)
    old = torch.get_default_dtype()
    torch.set_default_dtype(DT)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 1.0},
                              experts={"type": "llama_ffn", "num_experts_per_device": E, "hidden_size_per_expert": H}, model_dim=M)
    finally:
        torch.set_default_dtype(old)
    with torch.no_grad():   # a wider spread than the reference's normal(0, 0.01)
        layer.experts.W_fc1.normal_(0, M ** -0.5); layer.experts.W_fc2.normal_(0, M ** -0.5); layer.experts.W_fc3.normal_(0, H ** -0.5)
    layer = layer.cuda().eval()
    x = torch.randn([E * R // K, M], device="cuda").to(DT)
    ran = {}

    def forward(on):
        def run():
            layer.experts.fp8_weights = on
            with torch.no_grad():
                layer(x)
            ran[on] = layer._fp8_weights_ran
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
        sys.exit("expert_gemm_w8_glu_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd import ops
    from tutel_amd.experts import w8
    out = {"tool": "tools/expert_gemm_w8_glu_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16",
           "samples": args.samples, "warmup": args.warmup, "inner": args.inner, "shapes": {}}
    for name in args.shapes:
        s = SHAPES[name]
        arms, algo, errs = expert_arms(ops, w8, **s)
        res = alternate(arms, args.samples, args.warmup, args.inner)
        for arm, nbytes in algo.items():
            res[arm].update(algorithmic_bytes=nbytes, tb_per_s=round(nbytes / (res[arm]["median_us"] * 1e-6) / 1e12, 3))
        entry = dict(shape=s, max_abs_diff_vs_16bit_on_dequantised=errs, gemm=res,
                     gate_up_w8_over_16bit=round(res["gate_up_w8"]["median_us"] / res["gate_up_16bit"]["median_us"], 3),
                     ffn_w8_over_16bit=round(res["ffn_w8"]["median_us"] / res["ffn_16bit"]["median_us"], 3))
        del arms
        torch.cuda.empty_cache()
        if not args.no_layer:
            larms, ran = layer_arms(**s)
            entry["layer"] = alternate(larms, args.samples, args.warmup, 1)
            assert ran[True] is True, f"the switched-on layer did not read FP8 weights: {ran[True]}"
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
