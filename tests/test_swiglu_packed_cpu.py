"""The packed dropless forward for SwiGLU experts without a GPU: why a llama_ffn layer is refused (ep_native.packed_unsupported on
CPU-built layers), and the new entry points on the C-ABI boundary -- declared, exported, bound with the header's arity, and their
argument errors / uncovered cases reported before anything is enqueued."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tutel_amd_expert_gemm_gate_up", "tutel_amd_moe_forward_packed_glu")


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _layer(M=256, H=256, E=8, dtype=torch.bfloat16, **experts):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        spec = {"type": "llama_ffn", "num_experts_per_device": E, "hidden_size_per_expert": H}
        spec.update(experts)
        layer = moe.moe_layer(gate_type={"type": "top", "k": 2, "capacity_factor": 0.0}, experts=spec, model_dim=M)
    finally:
        torch.set_default_dtype(old)
    return layer.eval()


def _why(layer, T=512, E=8, M=256, dtype=torch.bfloat16, limit=0, alignment=1):
    from tutel_amd.impls import ep_native
    with torch.no_grad():
        return ep_native.packed_unsupported(layer, T, E, 2, M, dtype, limit, alignment)


def test_covered_llama_layer_has_no_reason(L):
    assert _why(_layer()) is None
    assert _why(_layer(activation_fn=torch.nn.functional.gelu)) is None
    assert _why(_layer(activation_fn=torch.nn.ReLU())) is None


def test_each_uncovered_case_has_its_reason(L):
    layer = _layer()
    layer.train()
    assert "inference" in _why(layer)
    layer.eval()
    with torch.enable_grad():   # parameters that require grad under autograd
        from tutel_amd.impls import ep_native
        assert "inference" in ep_native.packed_unsupported(layer, 512, 8, 2, 256, torch.bfloat16, 0, 1)
    layer.experts.sharded_count = 2
    assert "sharded" in _why(layer)
    layer.experts.sharded_count = 1
    assert "activation" in _why(_layer(activation_fn=lambda t: torch.clamp(t, -1.0, 1.0)))
    assert "dtype" in _why(layer, dtype=torch.float16)
    assert "H and M_out" in _why(_layer(H=64))                 # the plan's shape rule
    assert "16-bit" in _why(_layer(dtype=torch.float32), dtype=torch.float32)
    layer.is_postscore = False
    assert "is_postscore" in _why(layer)
    layer.is_postscore = True
    layer.world_size = 2   # (an attribute of the layer: what a multi-rank group would give)
    assert "single rank" in _why(layer)


def test_workspace_sized_for_the_swiglu_shapes(L):
    """workspace: the plan with H and M_out = M (the down projection's output is the model dimension)"""
    from tutel_amd import _lib
    b = L.tutel_amd_moe_packed_workspace_bytes(4096, 64, 2, 2048, 2048, 2048, _lib.BF16, 0, 4)
    assert b > 0 and b % 256 == 0


def _arity(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return len([p for p in m.group(1).split(",") if p.strip()])


def test_new_entry_points_declared_exported_bound(L):
    from tutel_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(raw, name)
        assert len(_lib.SIGNATURES[name][1]) == _arity(name), name
    assert L.tutel_amd_abi_version() == 1


def test_gate_up_rejects_before_enqueueing(L):
    from tutel_amd import _lib
    fake = ctypes.c_void_p(0x10000)

    def call(K=256, act=_lib.ACT_SILU, E=2, R=64, N=128, w_up=fake, dtype=_lib.BF16):
        return L.tutel_amd_expert_gemm_gate_up(fake, R * K, 0, R, K, fake, w_up, N * K, K, fake, R * N, 0, R, N, E, R, N, K, dtype, act,
                                               None, 1, None)
    assert call(act=_lib.ACT_NONE) == _lib.ENOTSUP and b"relu, gelu or silu" in L.tutel_amd_last_error()
    assert call(K=100) not in (0, _lib.ENOTSUP) and b"multiple of 64" in L.tutel_amd_last_error()
    assert call(dtype=_lib.F32) not in (0, _lib.ENOTSUP) and b"dtype" in L.tutel_amd_last_error()
    assert call(w_up=None) not in (0, _lib.ENOTSUP) and b"W_up" in L.tutel_amd_last_error()
    assert call(E=0) == 0 and call(R=0) == 0   # empty problems: nothing to launch


def test_forward_packed_glu_rejects_before_enqueueing(L):
    from tutel_amd import _lib
    m, pk = _lib.MoeArgs(), _lib.PackedArgs()
    a = m.ep
    a.T, a.M, a.H, a.M_out, a.num_experts, a.world, a.k, a.dtype, a.act = 64, 256, 256, 256, 8, 1, 2, _lib.BF16, _lib.ACT_SILU
    a.is_postscore, a.w2_kmajor = 1, 1
    m.alignment, m.logits_dtype = 1, _lib.BF16
    fake = ctypes.c_void_p(0x10000)
    assert L.tutel_amd_moe_forward_packed_glu(None, ctypes.byref(m), ctypes.byref(pk), None, None) != 0
    assert b"w_up" in L.tutel_amd_last_error()
    pk.offsets = pk.capacity = m.dispatch_count = m.ws = m.logits = fake
    pk.ws, pk.ws_bytes = fake, L.tutel_amd_moe_packed_workspace_bytes(64, 8, 2, 256, 256, 256, _lib.BF16, 0, 1)
    a.x = a.idx = a.loc = a.gates = a.w1 = a.w2 = a.y = a.zero_row = fake
    m.ws_bytes = 1 << 20
    a.b1 = fake   # SwiGLU experts have no biases
    assert L.tutel_amd_moe_forward_packed_glu(None, ctypes.byref(m), ctypes.byref(pk), fake, None) not in (0, _lib.ENOTSUP)
    assert b"biases" in L.tutel_amd_last_error()
    a.b1 = None
    a.act = _lib.ACT_NONE   # the fused gate/up GEMM takes relu, gelu, silu
    assert L.tutel_amd_moe_forward_packed_glu(None, ctypes.byref(m), ctypes.byref(pk), fake, None) == _lib.ENOTSUP
    a.act, a.H = _lib.ACT_SILU, 64
    assert L.tutel_amd_moe_forward_packed_glu(None, ctypes.byref(m), ctypes.byref(pk), fake, None) == _lib.ENOTSUP
    a.H, a.world = 256, 2
    assert L.tutel_amd_moe_forward_packed_glu(None, ctypes.byref(m), ctypes.byref(pk), fake, None) != 0
    assert b"single rank" in L.tutel_amd_last_error()
