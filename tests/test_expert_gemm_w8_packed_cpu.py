"""The W8A16 grouped GEMMs over the packed dropless layout (csrc/expert_gemm_w8.hip, tutel_amd_expert_gemm_w8_packed /
tutel_amd_expert_gemm_w8_glu_packed) without a GPU: both entry points are declared, exported and bound, every refusal names its
reason in front of any HIP call (null operands everywhere: only the argument checks can answer), the empty problem is a no-op, and
the layer's switch is off unless the environment asks."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLAIN, GLU = "tutel_amd_expert_gemm_w8_packed", "tutel_amd_expert_gemm_w8_glu_packed"


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _plain(L, E=1, rows=1, tiles=1, N=32, K=64, dtype=None, act=0, lda=None, ldd=None, w_stride=None, bias_stride=0):
    from tutel_amd import _lib
    dtype = _lib.BF16 if dtype is None else dtype
    return L.tutel_amd_expert_gemm_w8_packed(None, K if lda is None else lda, None, 0, None, None, N * K if w_stride is None else w_stride,
                                             None, None, bias_stride, None, N if ldd is None else ldd, E, rows, N, K, dtype, act,
                                             None, None, None, tiles, None)


def _glu(L, E=1, rows=1, tiles=1, H=16, K=64, dtype=None, act=3, lda=None, ldd=None, w_stride=None):
    from tutel_amd import _lib
    dtype = _lib.BF16 if dtype is None else dtype
    return L.tutel_amd_expert_gemm_w8_glu_packed(None, K if lda is None else lda, None, 0, None, None,
                                                 2 * H * K if w_stride is None else w_stride, None, None, H if ldd is None else ldd,
                                                 E, rows, H, K, dtype, act, None, None, None, tiles, None)


def test_header_declares_and_signatures_bind_both_entry_points(L):
    from tutel_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in (PLAIN, GLU):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " is not declared"
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert len(_lib.SIGNATURES[PLAIN][1]) == 23 and len(_lib.SIGNATURES[GLU][1]) == 21


def test_plain_refusals_name_their_reason_and_enqueue_nothing(L):
    from tutel_amd import _lib
    for kw, word in ((dict(K=96), b"K must be a multiple of 64"), (dict(K=100), b"K must be"), (dict(N=40), b"N must be a multiple of 32"),
                     (dict(N=8), b"N must be"), (dict(dtype=_lib.F32), b"bf16 or fp16"), (dict(dtype=7), b"bf16 or fp16"),
                     (dict(act=4), b"activation"), (dict(act=-1), b"activation"), (dict(lda=68), b"aligned"), (dict(ldd=34), b"aligned"),
                     (dict(bias_stride=34), b"aligned"), (dict(w_stride=32 * 64 + 8), b"aligned"), (dict(w_stride=1024), b"image"),
                     (dict(tiles=1 << 30), b"2^31"), (dict(tiles=1 << 24, N=32 * 4 * 64), b"2^31")):
        rc = _plain(L, **kw)
        err = L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and PLAIN.encode() in err and b"not covered" in err and word in err, (kw, rc, err)
    # a covered shape with null operands: an error (not ENOTSUP), still in front of any HIP call -- this machine may have no GPU
    rc = _plain(L)
    assert rc not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _plain(L, N=0) not in (0, _lib.ENOTSUP) and b"bad sizes" in L.tutel_amd_last_error()
    assert _plain(L, rows=-1) not in (0, _lib.ENOTSUP) and _plain(L, tiles=-1) not in (0, _lib.ENOTSUP)
    # one below the work item limit is taken as far as the operand check: 2^23 tiles x 2 halves x 64 channel tiles < 2^31
    assert _plain(L, tiles=(1 << 23) - 1, N=128 * 64) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()


def test_glu_refusals_name_their_reason_and_enqueue_nothing(L):
    from tutel_amd import _lib
    for kw, word in ((dict(K=96), b"K must be a multiple of 64"), (dict(H=24), b"H must be a multiple of 16"), (dict(H=8), b"H must be"),
                     (dict(dtype=_lib.F32), b"bf16 or fp16"), (dict(act=4), b"activation"), (dict(lda=68), b"aligned"),
                     (dict(ldd=18), b"aligned"), (dict(w_stride=2 * 16 * 64 + 8), b"aligned"), (dict(w_stride=16 * 64), b"image"),
                     (dict(tiles=1 << 30), b"2^31")):
        rc = _glu(L, **kw)
        err = L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and GLU.encode() in err and b"not covered" in err and word in err, (kw, rc, err)
    rc = _glu(L)
    assert rc not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _glu(L, H=0) not in (0, _lib.ENOTSUP) and b"bad sizes" in L.tutel_amd_last_error()


def test_a_refusal_comes_before_the_empty_problem(L):
    """the checks stand in front of the no-op: an uncovered shape is refused even when nothing would run"""
    from tutel_amd import _lib
    assert _plain(L, E=0, K=96) == _lib.ENOTSUP and _glu(L, rows=0, H=24) == _lib.ENOTSUP


def test_empty_problem_is_a_no_op(L):
    for call in (_plain, _glu):
        assert call(L, E=0) == 0 and call(L, rows=0) == 0 and call(L, tiles=0) == 0 and call(L, E=0, rows=0, tiles=0) == 0


def test_switch_is_off_unless_the_environment_asks():
    code = ("import torch; from tutel_amd.impls.moe_layer import MOELayer; "
            "l = MOELayer({'type': 'top', 'k': 1}, 64, experts={'type': 'ffn', 'num_experts_per_device': 2, 'hidden_size_per_expert': 64}); "
            "print(int(l.dropless_packed_fp8))")
    for value, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "TUTEL_AMD_DROPLESS_PACKED_FP8"}
        if value is not None:
            env["TUTEL_AMD_DROPLESS_PACKED_FP8"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


def test_the_switch_alone_admits_nothing():
    """dropless_packed_fp8 acts only with capacity_factor <= 0, dropless_packed and experts.fp8_weights: each one missing, the
    admission answers None and records no reason (the forward is exactly what it is without the switch)"""
    import torch
    from tutel_amd.impls.moe_layer import MOELayer
    layer = MOELayer({"type": "top", "k": 1}, 64, experts={"type": "ffn", "num_experts_per_device": 2, "hidden_size_per_expert": 64}).eval()
    x = torch.zeros([8, 64])
    logits = torch.empty([8, 2], device="meta")

    def ask(cf):
        layer._dropless_packed_ran = layer._fp8_weights_ran = None
        gate = layer.gates[0]
        plan = layer._packed_fp8_plan(x, logits, (gate, 1, cf, 1, 1, x.shape[-1:], False, 0, x.dtype))
        return plan, layer._dropless_packed_ran, layer._fp8_weights_ran

    for fp8, packed, w8, cf in ((False, True, True, 0.0), (True, False, True, 0.0), (True, True, False, 0.0), (True, True, True, 1.0)):
        layer.dropless_packed_fp8, layer.dropless_packed, layer.experts.fp8_weights = fp8, packed, w8
        assert ask(cf) == (None, None, None), (fp8, packed, w8, cf)
    # all four hold, but the tokens are not on the device: refused with the routing's reason, in _dropless_packed_ran
    layer.dropless_packed_fp8 = layer.dropless_packed = layer.experts.fp8_weights = True
    plan, why, fp8_why = ask(0.0)
    assert plan is None and isinstance(why, str) and "one-call native path" in why and fp8_why is None
