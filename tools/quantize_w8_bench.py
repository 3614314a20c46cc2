#!/usr/bin/env python3
"""What quantising the expert weights to FP8 costs, and what fp8_freeze() does to memory, at the headline experts (E = 64,
M = H = 2048, bf16), `ffn` and SwiGLU:

  quantise  all of a module's parameters: the torch quantiser on the device (w8.prepare / w8.prepare_gate_up, the derived-copy path)
            against the HIP quantiser (csrc/quantize_w8.hip through w8.prepare_native / prepare_gate_up_native).  Arms alternated
            sample by sample in one process, every sample timed with device events after a warm-up; the results are dropped between
            samples, so each sample allocates afresh (from the caching allocator, as a real call does).
  peak      torch.cuda.max_memory_allocated over one call of each arm, above the memory allocated before it (the parameters).
  freeze    torch.cuda.memory_allocated before and after module.fp8_freeze(), and the peak over it.

Byte model of the kernel, per parameter of P elements in 16 bits: 2 P read for the amax, 2 P read again for the codes (from L2
where a workgroup's 32 x K tile stays resident), P written -- 3 P to 5 P bytes of HBM traffic.  The outputs are compared bit for
bit before anything is timed.  Prints one JSON line.

    python tools/quantize_w8_bench.py [--samples 10] [--warmup 2] [--kinds ffn swiglu] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

E, M, H = 64, 2048, 2048
DT = torch.bfloat16


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # microseconds


def alternate(arms, samples, warmup):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in arms}
    for _ in range(samples):
        for name, fn in arms.items():
            got[name].append(timed(fn))
    return {name: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1), samples=len(v))
            for name, v in got.items()}


def peak_over(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del keep
    return peak - base


def params(kind):
    g = torch.Generator().manual_seed(3)

    def w(*shape):
        return (torch.randn(shape, generator=g) / 45.0).to(DT).cuda()
    if kind == "ffn":
        return dict(fc1=w(E, H, M), fc2=w(E, H, M))
    return dict(gate=w(E, M, H), up=w(E, M, H), down=w(E, H, M))


def arms_of(kind, p, w8):
    if kind == "ffn":
        return (lambda: (w8.prepare(p["fc1"], True), w8.prepare(p["fc2"], False)),
                lambda: (w8.prepare_native(p["fc1"], True), w8.prepare_native(p["fc2"], False)))
    return (lambda: (w8.prepare_gate_up(p["gate"], p["up"], False), w8.prepare(p["down"], False)),
            lambda: (w8.prepare_gate_up_native(p["gate"], p["up"], False), w8.prepare_native(p["down"], False)))


def module_of(kind):
    from tutel_amd.experts import ffn, llama_ffn
    old = torch.get_default_dtype()
    torch.set_default_dtype(DT)
    try:
        with torch.device("cuda"):   # (the initialisation runs on the device: E nn.Linear pairs on the host take minutes at this size)
            mod = ffn.FusedExpertsNetwork(M, H, E, 1) if kind == "ffn" else llama_ffn.LlamaFFNNetwork(M, H, E, 1)
    finally:
        torch.set_default_dtype(old)
    return mod.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", nargs="+", default=["ffn", "swiglu"], choices=["ffn", "swiglu"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        sys.exit("quantize_w8_bench: no GPU visible -- these are device timings, there is nothing to fall back to")
    from tutel_amd.experts import w8
    out = {"tool": "tools/quantize_w8_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "E": E, "M": M, "H": H,
           "samples": args.samples, "warmup": args.warmup, "kinds": {}}
    for kind in args.kinds:
        p = params(kind)
        torch_arm, hip_arm = arms_of(kind, p, w8)
        a, b = torch_arm(), hip_arm()
        same = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
        assert same, "the HIP quantiser's bits differ from the torch quantiser's"
        del a, b
        elements = sum(t.numel() for t in p.values())
        entry = dict(parameters=len(p), parameter_bytes=2 * elements, image_and_scale_bytes=elements + 4 * E * (H + M if kind == "ffn" else 2 * H + M),
                     bit_equal=same, byte_model=dict(read_once_write_once=3 * elements, read_twice_write_once=5 * elements))
        entry["quantise"] = alternate(dict(torch=torch_arm, hip=hip_arm), args.samples, args.warmup)
        entry["hip_over_torch"] = round(entry["quantise"]["hip"]["median_us"] / entry["quantise"]["torch"]["median_us"], 4)
        us = entry["quantise"]["hip"]["median_us"]
        entry["hip_tb_per_s"] = dict(read_once_write_once=round(3 * elements / (us * 1e-6) / 1e12, 3),
                                     read_twice_write_once=round(5 * elements / (us * 1e-6) / 1e12, 3))
        entry["peak_bytes_above_parameters"] = dict(torch=peak_over(torch_arm), hip=peak_over(hip_arm))
        del p, torch_arm, hip_arm
        torch.cuda.empty_cache()
        mod = module_of(kind)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        mod.fp8_freeze()
        torch.cuda.synchronize()
        entry["freeze"] = dict(allocated_before=before, allocated_after=torch.cuda.memory_allocated(),
                               peak=torch.cuda.max_memory_allocated(),
                               after_over_before=round(torch.cuda.memory_allocated() / before, 4))
        del mod
        torch.cuda.empty_cache()
        out["kinds"][kind] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
