#!/usr/bin/env python3
"""One dropless training step at the configs[2] shape (T = 4096, M = H = 2048, E = 64, top-2, bf16, capacity_factor = 0):
forward, loss = y.float().square().mean() + l_aux, backward.  Three variants, interleaved round-robin so that clock and thermal
drift hit all of them alike: the padded eager step (dropless_packed off), the packed eager step, and the packed step replayed
from a torch.cuda.graph capture.  Each step is timed with device events; the median over the steps is printed as one JSON line.
--amp bf16|fp16: fp32 master weights and an fp32 input, the step under torch.autocast (examples/helloworld_amp.py) -- the packed
step then casts its 16-bit compute copies per call and takes fp32 weight gradients straight from the accumulators.
--reps N: the timed window N times over in the same process (same capture), one median per repetition: the spread.
--accum N: gradient accumulation instead -- one sample is the time of N packed micro-steps (forward + backward over N different
batches, gradients summed), the zeroing before them outside the timed window.  Arm packed_eager: autograd accumulates into
p.grad (N - 1 AccumulateGrad adds per parameter).  With --main_grad two more arms, where the gradient kernels add into the expert
parameters' fp32 main_grad (layer.dropless_packed_main_grad): main_grad_eager, and main_grad_graph, ONE captured micro-step
replayed N times.  zero_main_grads is timed on its own (zero_main_grads_ms).

    python tools/packed_train_bench.py [--steps 50] [--warmup 10] [--amp bf16] [--reps 5]
    python tools/packed_train_bench.py --accum 4 --main_grad --amp bf16 --steps 20 --reps 3
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def accum(args, layer, amp, shape):
    """--accum N: see the module docstring"""
    N, (T, M) = args.accum, shape
    params = list(layer.parameters())
    xs = [torch.randn(T, M, device="cuda", dtype=torch.float32 if amp is not None else torch.bfloat16) * (1 + i % 3) for i in range(N)]
    static_x = xs[0].clone()
    layer.dropless_packed = True

    def micro(x):
        with (torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()):
            y = layer(x)
            loss = y.float().square().mean() + y.l_aux.float()
        loss.backward()

    def zero_grads():
        for p in params:
            p.grad = None

    arms, zero = {}, {}
    if args.main_grad:
        from tutel_amd.impls import packed_train
        packed_train.attach_main_grads(layer)
        layer.dropless_packed_main_grad = True
        # capture FIRST, warmed up on a side stream (see main())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                zero_grads()
                micro(static_x)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        zero_grads()
        with torch.cuda.graph(g):
            micro(static_x)
        layer.l_aux = None
        assert layer._dropless_packed_ran is True, layer._dropless_packed_ran

        def eager_main():
            layer.dropless_packed_main_grad = True
            for x in xs:
                micro(x)

        def graph_main():
            for x in xs:
                static_x.copy_(x)
                g.replay()

        def zero_main():
            zero_grads()
            packed_train.zero_main_grads(layer)
        arms.update(main_grad_eager=eager_main, main_grad_graph=graph_main)
        zero.update(main_grad_eager=zero_main, main_grad_graph=zero_main)

    def eager_unfused():
        layer.dropless_packed_main_grad = False
        for x in xs:
            micro(x)
    arms = dict(packed_eager=eager_unfused, **arms)
    zero["packed_eager"] = zero_grads
    reps = {n: [] for n in arms}
    zero_ms = []
    for rep in range(max(args.reps, 1)):
        times = {n: [] for n in arms}
        for i in range(args.warmup + args.steps):
            for n, fn in arms.items():          # interleaved: drift hits every arm alike
                zero[n]()
                t = timed(fn)
                if i >= args.warmup:
                    times[n].append(t)
            if args.main_grad and i >= args.warmup:
                zero_ms.append(timed(lambda: packed_train.zero_main_grads(layer)))
        assert layer._dropless_packed_ran is True, layer._dropless_packed_ran
        for n, v in times.items():
            reps[n].append((statistics.median(v), min(v)))
    out = {"accum": N, "main_grad": bool(args.main_grad), "steps": args.steps,
           "median_ms": {n: round(statistics.median(m for m, _ in v), 4) for n, v in reps.items()},
           "min_ms": {n: round(min(lo for _, lo in v), 4) for n, v in reps.items()}}
    if zero_ms:
        out["zero_main_grads_ms"] = round(statistics.median(zero_ms), 4)
    if args.reps > 1:
        out["reps"] = args.reps
        out["rep_median_ms"] = {n: [round(m, 4) for m, _ in v] for n, v in reps.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--T", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--E", type=int, default=64)
    ap.add_argument("--amp", choices=["bf16", "fp16"], default=None, help="fp32 master weights, the step under torch.autocast in this dtype")
    ap.add_argument("--reps", type=int, default=1, help="repetitions of the timed window (the median of each is reported)")
    ap.add_argument("--accum", type=int, default=0, help="time N micro-steps of gradient accumulation (packed step only)")
    ap.add_argument("--main_grad", action="store_true", help="with --accum: add the arms that accumulate into fp32 main_grad")
    args = ap.parse_args()
    if args.main_grad and args.accum < 1:
        ap.error("--main_grad goes with --accum N")
    from tutel import moe
    T, M, E = args.T, args.dim, args.E
    torch.manual_seed(0)
    amp = {"bf16": torch.bfloat16, "fp16": torch.float16, None: None}[args.amp]
    torch.set_default_dtype(torch.float32 if amp is not None else torch.bfloat16)
    layer = moe.moe_layer(gate_type={"type": "top", "k": 2, "capacity_factor": 0.0},
                          experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": M,
                                   "activation_fn": lambda t: torch.nn.functional.relu(t)}, model_dim=M)
    torch.set_default_dtype(torch.float32)
    layer = layer.cuda().train()
    shape = {"T": T, "M": M, "H": M, "E": E, "k": 2, "dtype": args.amp or "bf16", "masters": "fp32" if amp is not None else "bf16"}
    if args.accum > 0:
        print(json.dumps(dict({"shape": shape, "amp": args.amp}, **accum(args, layer, amp, (T, M)))))
        return
    params = list(layer.parameters())
    x = torch.randn(T, M, device="cuda", dtype=torch.float32 if amp is not None else torch.bfloat16)

    def step(packed):
        layer.dropless_packed = packed
        for p in params:
            p.grad = None
        with (torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()):
            y = layer(x)
            loss = y.float().square().mean() + y.l_aux.float()
        loss.backward()

    # capture FIRST: warmed up on a side stream, before any eager step on the default stream -- an autograd graph kept alive by the
    # layer's l_aux would otherwise hold AccumulateGrad nodes bound to the default stream into the capture (torch.cuda.graph docs)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    for p in params:
        p.grad = None
    with torch.cuda.graph(g):
        step(True)
    layer.l_aux = None
    assert layer._dropless_packed_ran is True, layer._dropless_packed_ran
    for _ in range(3):
        step(False)
        step(True)
    variants = {"padded_eager": lambda: step(False), "packed_eager": lambda: step(True), "packed_graph": g.replay}
    reps = {n: [] for n in variants}
    for rep in range(max(args.reps, 1)):
        times = {n: [] for n in variants}
        for i in range(args.warmup + args.steps):
            for n, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    times[n].append(a.elapsed_time(b))
        for n, v in times.items():
            reps[n].append((statistics.median(v), min(v)))
    out = {"shape": shape,
           "amp": args.amp, "steps": args.steps,
           "median_ms": {n: round(statistics.median(m for m, _ in v), 4) for n, v in reps.items()},
           "min_ms": {n: round(min(lo for _, lo in v), 4) for n, v in reps.items()}}
    if args.reps > 1:
        out["reps"] = args.reps
        out["rep_median_ms"] = {n: [round(m, 4) for m, _ in v] for n, v in reps.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
