"""The order of the checks by which a layer's experts are admitted to an opt-in GEMM (fp32 experts on tutel_amd_expert_gemm_f32, FP8
weights on tutel_amd_expert_gemm_w8) is behaviour: the first failing check is the reason a user reads.  For each of the two, a state
that fails EVERY check at once is repaired one check at a time, and the reason must move down the ladder in this order, down to None."""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_expert_gemm_w8_cpu import L, _CudaLike   # noqa: E402,F401  (the built library; the device tensor's stand-in)


def _walk(refusal, steps):
    for want, repair in steps:
        assert refusal() == want
        repair()
    assert refusal() is None


def _resize(net, M, H, dtype):
    """the experts' parameters at another shape, frozen"""
    E = net.batched_fc1_w.size(0)
    for name, shape in (("batched_fc1_w", [E, H, M]), ("batched_fc2_w", [E, H, M]), ("batched_fc1_bias", [E, H]), ("batched_fc2_bias", [E, M])):
        setattr(net, name, torch.nn.Parameter(torch.zeros(shape, dtype=dtype), requires_grad=False))


def _all_wrong(monkeypatch, net, x_dtype):
    """what both ladders share, every check failing: SKIP_EXPERT, a host tensor of the wrong dtype, autocast, a live parameter, sharded
    experts, megablocks row counts, an activation that is no epilogue"""
    net.skip_expert = True
    x = _CudaLike()
    x.is_cuda, x.dtype = False, x_dtype
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    for p in net.parameters():
        p.requires_grad_(p is net.batched_fc1_w)
    ctx = types.SimpleNamespace(sharded_count=2, adaptive_degree=1, megablocks_size=4)
    net.activation_fn, net._act_cache = (lambda t: t.clamp(0, 6)), {}
    return x, ctx


def _relu(net):
    net.activation_fn, net._act_cache = torch.nn.functional.relu, {}


def test_fp32_ladder_order(L, monkeypatch):
    from tutel_amd.experts import ffn
    net = ffn.FusedExpertsNetwork(64, 24, 2, 1)   # hidden size 24: fc2's K is no multiple of 32
    x, ctx = _all_wrong(monkeypatch, net, torch.bfloat16)
    monkeypatch.setattr(ffn, "_NATIVE_FP32", False)
    with torch.enable_grad():
        _walk(lambda: net.f32_refusal(x, ctx), [
            ("TUTEL_AMD_NATIVE_FP32 is off", lambda: monkeypatch.setattr(ffn, "_NATIVE_FP32", True)),
            ("SKIP_EXPERT is set", lambda: setattr(net, "skip_expert", False)),
            ("the input is not on the HIP device", lambda: setattr(x, "is_cuda", True)),
            ("autocast is on", lambda: monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: False)),
            ("the input and the experts' parameters are not all fp32", lambda: setattr(x, "dtype", torch.float32)),
            ("autograd is live (training stays on ATen)", lambda: net.batched_fc1_w.requires_grad_(False)),
            ("gathered-weight modes (sharded experts, adaptive_r = 0) are not covered", lambda: setattr(ctx, "sharded_count", 1)),
            ("megablocks row counts are not covered", lambda: setattr(ctx, "megablocks_size", 0)),
            ("the activation is not one of the fused epilogues", lambda: _relu(net)),
            ("the shape is not covered (M and H multiples of 32, H and M_out multiples of 4)", lambda: _resize(net, 64, 32, torch.float32)),
        ])
        assert net.can_fuse_f32(x, ctx) is True


def test_fp8_weights_ladder_order(L, monkeypatch):
    from tutel_amd.experts import ffn
    net = ffn.FusedExpertsNetwork(64, 48, 2, 1).to(torch.bfloat16)   # hidden size 48: no multiple of 64 (fc2's K)
    x, ctx = _all_wrong(monkeypatch, net, torch.float32)
    net.fp8_weights = False
    net.train()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with torch.enable_grad():
        _walk(lambda: net.w8_refusal(x, ctx), [
            ("fp8_weights is off (TUTEL_AMD_FP8_WEIGHTS)", lambda: setattr(net, "fp8_weights", True)),
            ("SKIP_EXPERT is set", lambda: setattr(net, "skip_expert", False)),
            ("the input is not on the HIP device", lambda: setattr(x, "is_cuda", True)),
            ("autograd is live (FP8 weights are inference only)", lambda: net.batched_fc1_w.requires_grad_(False)),
            ("the module is in training mode (FP8 weights are inference only)", lambda: net.eval()),
            ("autocast is on", lambda: monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: False)),
            ("the input is not bf16 / fp16 in the experts' own dtype", lambda: setattr(x, "dtype", torch.bfloat16)),
            ("gathered-weight modes (sharded experts, adaptive_r = 0) are not covered", lambda: setattr(ctx, "sharded_count", 1)),
            ("megablocks row counts are not covered", lambda: setattr(ctx, "megablocks_size", 0)),
            ("the activation is not one of the fused epilogues", lambda: _relu(net)),
            ("the shape is not covered (M and H multiples of 64, H and M_out multiples of 32)", lambda: _resize(net, 64, 64, torch.bfloat16)),
            ("the quantised weights are not cached yet: run one eager forward before capturing a graph", lambda: net.w8_params()),
        ])
