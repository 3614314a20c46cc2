"""Packed dropless training under autocast over fp32 master weights, without a GPU: the two fp32-output gradient entry points on
the C-ABI boundary (declared, exported, bound; their refusals and argument errors before anything is enqueued) and the host logic
of impls/packed_train.unsupported for the autocast case (CPU-built layers, the CUDA autocast predicates patched)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tutel_amd_expert_wgrad_packed_f32", "tutel_amd_expert_bgrad_packed_f32")


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def test_f32_symbols_declared_exported_bound(L):
    from tutel_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", hdr)
        assert m is not None, n
        assert hasattr(raw, n), n
        assert len(_lib.SIGNATURES[n][1]) == m.group(1).count(",") + 1, n
        # the same argument list as the 16-bit sibling
        sib = re.search(r"\b" + n[:-4] + r"\s*\(([^)]*)\)", hdr)
        assert m.group(1).count(",") == sib.group(1).count(","), n
        assert len(_lib.SIGNATURES[n][1]) == len(_lib.SIGNATURES[n[:-4]][1]), n


def test_f32_argument_errors_before_any_launch(L):
    from tutel_amd import _lib
    ENOTSUP = _lib.ENOTSUP
    wg, bg = L.tutel_amd_expert_wgrad_packed_f32, L.tutel_amd_expert_bgrad_packed_f32
    fake, odd = 1 << 20, (1 << 20) + 8      # never dereferenced: every call below returns before a launch
    # fp32 operands (dtype code 0): not covered
    assert wg(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 128, 128, _lib.F32, None, None) == ENOTSUP
    assert b"16-bit" in L.tutel_amd_last_error() and b"_f32" in L.tutel_amd_last_error()
    assert bg(None, 128, None, 8, 128, _lib.F32, None, None) == ENOTSUP
    assert b"16-bit" in L.tutel_amd_last_error()
    # N_b = 100, and a leading dimension that is no multiple of 8
    assert wg(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 128, 100, _lib.BF16, None, None) == ENOTSUP
    assert b"multiples of 8" in L.tutel_amd_last_error()
    assert wg(None, 132, None, 128, None, 0, 0, None, None, 8, 64, 128, 128, _lib.F16, None, None) == ENOTSUP
    assert b"multiples of 8" in L.tutel_amd_last_error()
    # null D; D 8-byte but not 16-byte aligned (the 16-bit entry point takes that address, the fp32 one stores 16 bytes)
    assert wg(fake, 128, fake, 128, None, 0, 0, None, None, 8, 64, 128, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"null" in L.tutel_amd_last_error()
    assert wg(fake, 128, fake, 128, None, 0, 0, None, odd, 8, 64, 128, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"16-byte" in L.tutel_amd_last_error()
    assert bg(fake, 128, None, 8, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"null" in L.tutel_amd_last_error()
    assert bg(fake, 128, odd, 8, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"16-byte" in L.tutel_amd_last_error()
    # a bad gather code is an argument error as on the 16-bit entry point
    assert wg(None, 128, None, 128, None, 3, 4, None, None, 8, 64, 128, 128, _lib.BF16, None, None) not in (0, ENOTSUP)
    # ops: out_dtype is None, the operands' dtype or torch.float32
    from tutel_amd import ops
    with pytest.raises(_lib.TutelAmdError, match="float32"):
        ops._grad_out_dtype(torch.float64, torch.bfloat16)
    with pytest.raises(_lib.TutelAmdError, match="float32"):
        ops._grad_out_dtype(torch.float16, torch.bfloat16)
    assert ops._grad_out_dtype(None, torch.float16) == (torch.float16, "")
    assert ops._grad_out_dtype(torch.float32, torch.float16) == (torch.float32, "_f32")


def _layer(M=256, H=256, E=8, k=2, dtype=torch.float32, act=torch.nn.functional.relu):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": k, "capacity_factor": 0.0},
                              experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H, "activation_fn": act},
                              model_dim=M)
    finally:
        torch.set_default_dtype(old)
    return layer.train()


def _why(layer, dtype, T=512, E=8, k=2, M=256):
    from tutel_amd.impls import packed_train
    return packed_train.unsupported(layer, layer.gates[0], T, E, k, M, dtype, 0.0, 1)


def _cuda_autocast(monkeypatch, amp):
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda device_type: amp)


def test_unsupported_under_autocast_host_logic(L, monkeypatch):
    # fp32 masters without autocast, and under a real CPU autocast context (the CUDA predicate stays False): refused as before
    assert "bf16 / fp16" in _why(_layer(), torch.float32)
    assert "bf16 / fp16" in _why(_layer(), torch.bfloat16)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert isinstance(_why(_layer(), torch.float32), str)
        assert "bf16 / fp16" in _why(_layer(), torch.bfloat16)
    for amp in (torch.bfloat16, torch.float16):
        with monkeypatch.context() as mp:
            _cuda_autocast(mp, amp)
            assert _why(_layer(), amp) is None
    with monkeypatch.context() as mp:
        _cuda_autocast(mp, torch.bfloat16)
        assert isinstance(_why(_layer(), torch.float16), str)            # tokens not in the autocast dtype
        assert isinstance(_why(_layer(), torch.float32), str)
        assert "ReLU" in _why(_layer(act=torch.nn.functional.gelu), torch.bfloat16)
        mixed = _layer()
        mixed.experts.batched_fc1_bias.data = mixed.experts.batched_fc1_bias.data.to(torch.bfloat16)
        assert "fp32" in _why(mixed, torch.bfloat16)                      # expert parameters of mixed dtypes
        # 16-bit experts under autocast: tokens in their dtype, as without it
        assert _why(_layer(dtype=torch.bfloat16), torch.bfloat16) is None
        assert "bf16 / fp16" in _why(_layer(dtype=torch.bfloat16), torch.float16)
        # the other refusals keep their words
        layer = _layer()
        layer.batch_prioritized_routing = True
        assert "batch-prioritised" in _why(layer, torch.bfloat16)
        layer = _layer()
        layer.gates[0].gate_noise = 0.5
        assert "gate noise" in _why(layer, torch.bfloat16)
        layer = _layer()
        layer.world_size = 2
        assert "single rank" in _why(layer, torch.bfloat16)
        assert "multiples of 64" in _why(_layer(H=160), torch.bfloat16)
    with monkeypatch.context() as mp:
        _cuda_autocast(mp, torch.float32)                                  # an autocast dtype the kernels do not take
        assert isinstance(_why(_layer(), torch.float32), str)
