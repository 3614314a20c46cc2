"""tutel_amd_expert_gemm_w4a8_packed / _glu_packed and tutel_amd_quantize_rows_a8_bounded without a GPU: the symbols are exported and bound,
and since every check precedes the first HIP call, refusals, no-ops and operand errors are answered with null pointers in either form."""
import pytest

NAMES = ("tutel_amd_expert_gemm_w4a8_packed", "tutel_amd_expert_gemm_w4a8_glu_packed")


def _call(glu, E=1, rows=1, tiles=1, K=64, lda=None):
    """one expert's smallest covered problem with null operands"""
    from tutel_amd import _lib
    N = 16 if glu else 32
    head = (None, None, K if lda is None else lda, None, 0, None, None, 2 * N * K // 2 if glu else N * K // 2, None,
            (2 if glu else 1) * N * ((K + 127) // 128) * 4) + (() if glu else (None, 0))
    return getattr(_lib.lib(), NAMES[glu])(*head, None, N, E, rows, N, K, _lib.BF16, 0, None, None, None, tiles, None)


@pytest.mark.parametrize("form", ["wide", "halves"])
@pytest.mark.parametrize("glu", [0, 1])
def test_refusals_name_their_reason_and_no_ops_succeed_before_any_hip_call(glu, form, monkeypatch):
    from tutel_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert len(_lib.SIGNATURES[NAMES[glu]][1]) == (23 if glu else 25) and hasattr(L, NAMES[glu])
    monkeypatch.setenv("TUTEL_AMD_W4A8_PACKED_TILE", form)
    for kw, word in ((dict(K=96), b"K must be a multiple of 64"), (dict(lda=72), b"aligned"), (dict(tiles=1 << 30), b"2^31")):
        rc, err = _call(glu, **kw), L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and NAMES[glu].encode() in err and b"not covered" in err and word in err, (kw, rc, err)
    # null tables with nonzero bounds: an error (not ENOTSUP), still in front of any HIP call
    assert _call(glu) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _call(glu, E=0, K=96) == _lib.ENOTSUP, "the checks stand in front of the no-op"
    assert _call(glu, E=0) == 0 and _call(glu, rows=0) == 0 and _call(glu, tiles=0) == 0


def test_bounded_quantiser_is_bound_and_refuses_as_the_unbounded_one():
    from tutel_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert len(_lib.SIGNATURES["tutel_amd_quantize_rows_a8_bounded"][1]) == 10
    assert L.tutel_amd_quantize_rows_a8_bounded(None, _lib.BF16, 96, 1, 96, None, 96, None, None, None) == _lib.ENOTSUP
    assert b"tutel_amd_quantize_rows_a8_bounded" in L.tutel_amd_last_error() and b"multiple of 64" in L.tutel_amd_last_error()
    assert L.tutel_amd_quantize_rows_a8_bounded(None, _lib.BF16, 64, 0, 64, None, 64, None, None, None) == 0
    assert L.tutel_amd_quantize_rows_a8_bounded(None, _lib.BF16, 64, 1, 64, None, 64, None, None, None) not in (0, _lib.ENOTSUP)
