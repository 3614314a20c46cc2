"""tutel_amd_expert_gemm_w8a8_packed / _glu_packed without a GPU: the symbols are exported and bound, and since every check precedes the
first HIP call, refusals, no-ops and operand errors are answered with null pointers in either form."""
import pytest

NAMES = ("tutel_amd_expert_gemm_w8a8_packed", "tutel_amd_expert_gemm_w8a8_glu_packed")


def _call(glu, E=1, rows=1, tiles=1, K=64, lda=None, N=None, dtype=None, short=0):
    """one expert's smallest covered problem with null operands; N: output channels (GLU: H); short: bytes missing from w_stride_e"""
    from tutel_amd import _lib
    N = (16 if glu else 32) if N is None else N
    head = (None, None, K if lda is None else lda, None, 0, None, None, (2 if glu else 1) * N * K - short, None) + (() if glu else (None, 0))
    return getattr(_lib.lib(), NAMES[glu])(*head, None, N, E, rows, N, K, _lib.BF16 if dtype is None else dtype, 0, None, None, None,
                                           tiles, None)


@pytest.mark.parametrize("form", ["wide", "halves"])
@pytest.mark.parametrize("glu", [0, 1])
def test_refusals_name_their_reason_and_no_ops_succeed_before_any_hip_call(glu, form, monkeypatch):
    from tutel_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert len(_lib.SIGNATURES[NAMES[glu]][1]) == (22 if glu else 24) and hasattr(L, NAMES[glu])
    monkeypatch.setenv("TUTEL_AMD_W8A8_PACKED_TILE", form)
    for kw, word in ((dict(K=96), b"K must be a multiple of 64"), (dict(N=24 if glu else 48), b"must be a multiple of"),
                     (dict(dtype=_lib.F32), b"bf16 or fp16"), (dict(lda=72), b"aligned"), (dict(short=16), b"smaller than one expert's image"),
                     (dict(tiles=1 << 30), b"2^31")):
        rc, err = _call(glu, **kw), L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and NAMES[glu].encode() in err and b"not covered" in err and word in err, (kw, rc, err)
    # null tables with nonzero bounds: an error (not ENOTSUP), still in front of any HIP call
    assert _call(glu) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _call(glu, E=0, K=96) == _lib.ENOTSUP, "the checks stand in front of the no-op"
    assert _call(glu, E=0) == 0 and _call(glu, rows=0) == 0 and _call(glu, tiles=0) == 0
