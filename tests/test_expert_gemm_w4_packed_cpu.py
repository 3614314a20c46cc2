"""tutel_amd_expert_gemm_w4_packed / _glu_packed without a GPU: every check precedes the first HIP call, so refusals, no-ops and operand
errors are answered through the C ABI with null pointers, whichever window form is selected; the ctypes table has both names."""
import pytest

NAMES = ("tutel_amd_expert_gemm_w4_packed", "tutel_amd_expert_gemm_w4_glu_packed")


def _call(glu, E=1, rows=1, tiles=1, N=None, K=64, dtype=None, act=0, lda=None, ldd=None, w_stride=None, s_stride=None, bias_stride=0):
    """N: the output channels (H of the GLU form, whose image has 2 H); the defaults are one expert's smallest covered problem"""
    from tutel_amd import _lib
    N = (16 if glu else 32) if N is None else N
    ws = (2 if glu else 1) * N * K // 2 if w_stride is None else w_stride
    ss = (2 if glu else 1) * N * ((K + 127) // 128) * 4 if s_stride is None else s_stride
    head = (None, K if lda is None else lda, None, 0, None, None, ws, None, ss) + (() if glu else (None, bias_stride))
    return getattr(_lib.lib(), NAMES[glu])(*head, None, N if ldd is None else ldd, E, rows, N, K, _lib.BF16 if dtype is None else dtype, act, None, None, None, tiles, None)


@pytest.mark.parametrize("form", ["wide", "halves"])
@pytest.mark.parametrize("glu", [0, 1])
def test_refusals_name_their_reason_and_no_ops_succeed_before_any_hip_call(glu, form, monkeypatch):
    from tutel_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert len(_lib.SIGNATURES[NAMES[glu]][1]) == (22 if glu else 24) and hasattr(L, NAMES[glu])
    monkeypatch.setenv("TUTEL_AMD_W4_PACKED_TILE", form)
    cases = [(dict(K=96), b"K must be a multiple of 64"), (dict(dtype=_lib.F32), b"bf16 or fp16"), (dict(act=4), b"activation"),
             (dict(lda=68), b"aligned"), (dict(ldd=18), b"aligned"), (dict(w_stride=1024 + 8), b"aligned"), (dict(s_stride=128 + 2), b"aligned"),
             (dict(w_stride=512), b"image"), (dict(s_stride=124), b"image"), (dict(tiles=1 << 30), b"2^31"),
             (dict(N=24), b"H must be a multiple of 16") if glu else (dict(N=48), b"N must be a multiple of 32")]
    for kw, word in cases + ([] if glu else [(dict(bias_stride=34), b"aligned")]):
        rc, err = _call(glu, **kw), L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and NAMES[glu].encode() in err and b"not covered" in err and word in err, (kw, rc, err)
    # a covered shape with null operands: an error (not ENOTSUP), still in front of any HIP call -- this machine may have no GPU
    assert _call(glu) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _call(glu, rows=-1) not in (0, _lib.ENOTSUP) and b"bad sizes" in L.tutel_amd_last_error()
    # the checks stand in front of the no-op: an uncovered shape is refused even when nothing would run
    assert _call(glu, E=0, K=96) == _lib.ENOTSUP
    assert _call(glu, E=0) == 0 and _call(glu, rows=0) == 0 and _call(glu, tiles=0) == 0
