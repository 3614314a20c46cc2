"""Dropless training on the packed layout without a GPU: why a layer's training step is refused (impls/packed_train.unsupported on
CPU-built layers), the planner's decisions with the flag off, and the new entry points on the C-ABI boundary -- declared, exported,
bound, and their argument errors / uncovered cases reported before anything is enqueued."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tutel_amd_packed_layout", "tutel_amd_expert_gemm_packed", "tutel_amd_expert_wgrad_packed", "tutel_amd_expert_bgrad_packed",
       "tutel_amd_gate_grad_packed", "tutel_amd_fast_decode_packed")


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _layer(M=256, H=256, E=8, k=2, dtype=torch.bfloat16, experts="ffn", **kw):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        spec = {"type": experts, "num_experts_per_device": E, "hidden_size_per_expert": H}
        if experts == "ffn":
            spec["activation_fn"] = kw.pop("act", torch.nn.functional.relu)
        layer = moe.moe_layer(gate_type=dict({"type": "top", "k": k, "capacity_factor": 0.0}, **kw.pop("gate", {})), experts=spec,
                              model_dim=M, **kw)
    finally:
        torch.set_default_dtype(old)
    return layer.train()


def _why(layer, T=512, E=8, k=2, M=256, dtype=torch.bfloat16, cf=0.0, alignment=1, **kw):
    from tutel_amd.impls import packed_train
    return packed_train.unsupported(layer, layer.gates[0], T, E, k, M, dtype, cf, alignment, **kw)


def test_covered_layer_has_no_reason(L):
    assert _why(_layer()) is None
    assert _why(_layer(gate={"fp32_gate": True})) is None
    assert _why(_layer(), cf=-0.5) is None
    assert _why(_layer(dtype=torch.float16), dtype=torch.float16) is None


def test_each_uncovered_case_has_its_reason(L):
    assert "inference" in _why(_layer(experts="llama_ffn"))          # SwiGLU training keeps its reason
    assert "ReLU" in _why(_layer(act=torch.nn.functional.gelu))
    assert "ReLU" in _why(_layer(act=lambda t: torch.clamp(t, -1.0, 1.0)))
    assert "bf16 / fp16" in _why(_layer(dtype=torch.float32), dtype=torch.float32)
    layer = _layer()
    layer.is_postscore = False
    assert "is_postscore" in _why(layer)
    layer = _layer()
    layer.gates[0].gate_noise = 0.5
    assert "gate noise" in _why(layer)
    layer = _layer()
    layer.batch_prioritized_routing = True
    assert "batch-prioritised" in _why(layer)
    layer = _layer()
    layer.is_gshard_loss = False
    assert "gshard" in _why(layer)
    layer = _layer()
    layer.world_size = 2
    assert "single rank" in _why(layer)
    assert "dropless" in _why(_layer(), cf=1.0)
    assert "HIP device" in _why(_layer(), on_device=False)
    assert "HIP device" in _why(_layer(), T=0)
    assert "multiples of 64" in _why(_layer(H=160))                   # the plan's shape rule
    assert "k * E" in _why(_layer(E=4096, k=4), E=4096, k=4)
    if torch.cuda.is_available() or hasattr(torch, "autocast"):
        with torch.autocast("cpu", dtype=torch.bfloat16):
            layer32 = _layer(dtype=torch.float32)
            assert "autocast" in _why(layer32) or "bf16 / fp16" in _why(layer32)


def test_autograd_live_predicate(L):
    """the packed training path is consulted only with autograd live: grad enabled and the input or an expert requiring grad"""
    from tutel_amd.impls import packed_train
    layer = _layer()
    x = torch.randn(4, 256)
    assert packed_train.autograd_live(layer, x)
    with torch.no_grad():
        assert not packed_train.autograd_live(layer, x)
    for p in layer.experts.parameters():
        p.requires_grad_(False)
    assert not packed_train.autograd_live(layer, x)
    assert packed_train.autograd_live(layer, x.requires_grad_(True))


def test_saved_tensor_sizes_follow_the_plan(L):
    from tutel_amd.impls import ep_native
    plan, why = ep_native.packed_plan(4096, 64, 2, 2048, 2048, 2048, torch.bfloat16, 0, 1)
    assert why is None
    # hid [rows_bound, H] and Y [rows_bound, M_out] kept for the backward; rows_bound = k*T + min(E, k*T)*(alignment - 1)
    assert plan["rows_bound"] == 8192 and plan["tiles_bound"] == 8192 // 256 + 64
    plan, _ = ep_native.packed_plan(4096, 64, 2, 2048, 2048, 2048, torch.bfloat16, 0, 8)
    assert plan["rows_bound"] == 8192 + 64 * 7


def test_new_symbols_declared_exported_bound(L):
    from tutel_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", hdr)
        assert m is not None, n
        assert hasattr(raw, n)
        assert len(_lib.SIGNATURES[n][1]) == m.group(1).count(",") + 1, n


def test_argument_errors_before_any_launch(L):
    from tutel_amd import _lib
    ENOTSUP = _lib.ENOTSUP
    # weight gradient: fp32 operands are not covered; N not a multiple of 8; bad gather code
    assert L.tutel_amd_expert_wgrad_packed(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 128, 128, 0, None, None) == ENOTSUP
    assert b"16-bit" in L.tutel_amd_last_error()
    assert L.tutel_amd_expert_wgrad_packed(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 100, 128, 2, None, None) == ENOTSUP
    assert b"multiples of 8" in L.tutel_amd_last_error()
    assert L.tutel_amd_expert_wgrad_packed(None, 128, None, 128, None, 3, 4, None, None, 8, 64, 128, 128, 2, None, None) not in (0, ENOTSUP)
    assert L.tutel_amd_expert_wgrad_packed(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 128, 128, 2, None, None) not in (0, ENOTSUP)
    assert b"null" in L.tutel_amd_last_error()
    assert L.tutel_amd_expert_bgrad_packed(None, 128, None, 8, 128, 0, None, None) == ENOTSUP
    # packed GEMM: n-major weights take no activation but none / relu and no gating operand
    assert L.tutel_amd_expert_gemm_packed(None, 256, None, 0, None, None, 0, 0, 256, None, 0, None, None, 256, 8, 512, 256, 256, 2, 2,
                                          None, None, None, None, 4, None) == ENOTSUP
    assert b"n-major" in L.tutel_amd_last_error()
    assert L.tutel_amd_expert_gemm_packed(None, 256, None, 0, None, None, 0, 0, 256, None, 0, 16, None, 256, 8, 512, 256, 256, 2, 0,
                                          None, None, None, None, 4, None) == ENOTSUP
    assert b"gated" in L.tutel_amd_last_error()
    assert L.tutel_amd_expert_gemm_packed(None, 256, None, 0, None, None, 1, 0, 256, None, 0, None, None, 256, 8, 512, 256, 256, 2, 0,
                                          None, None, None, None, 4, None) not in (0, ENOTSUP)
    # layout: the plan refuses k * E > 8192; buffers below the bound
    assert L.tutel_amd_packed_layout(None, None, None, 64, 4096, 4, 0, 1, 1 << 20, 1 << 20, None, None, None, None, None, None) == ENOTSUP
    assert L.tutel_amd_packed_layout(None, None, None, 64, 8, 2, 0, 1, 1, 1, None, None, None, None, None, None) not in (0, ENOTSUP)
    assert b"bounds" in L.tutel_amd_last_error()
    # decode / gate gradient over the packed rows
    assert L.tutel_amd_fast_decode_packed(None, 0, None, None, None, 0, 4, 8, 2, 1, None, None, None) not in (0,)
    assert L.tutel_amd_fast_decode_packed(None, 2, None, None, None, 0, 4, 8, 17, 1, None, None, None) == ENOTSUP
    assert L.tutel_amd_gate_grad_packed(None, None, 2, None, None, 4, 8, 2, 1, None, None, None) not in (0, ENOTSUP)
    assert L.tutel_amd_gate_grad_packed(None, None, 2, None, None, 0, 8, 2, 1, None, None, None) == 0   # empty: nothing to launch
