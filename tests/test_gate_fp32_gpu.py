"""The projection of an fp32 gate over 16-bit tokens (csrc/gate_proj.hip, tutel_amd_gate_proj_f32w) and its consumer
(tutel_amd_gate_topk_partials with TUTEL_F32): the ordering contract of include/tutel_amd.h checked bit for bit against a sequential
fmaf chain (tests/gate_fp32_ref.c, compiled here with gcc), the fp32 logits the top-k kernel derives from the partial sums, guard
bands around every operand, and the refusals."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 64, 4), (100, 192, 12), (64, 2048, 64), (130, 1024, 68), (257, 2048, 128), (4096, 2048, 64)]
DTYPES = [torch.bfloat16, torch.float16]
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1])


def _ops():
    from tutel_amd import ops
    return ops


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """gate_fp32_chain of tests/gate_fp32_ref.c: (x fp32 [T, M], w fp32 [E, M], m0, m1) -> [T, E] fp32, numpy in and out"""
    so = tmp_path_factory.mktemp("gate_fp32_ref") / "gate_fp32_ref.so"
    r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "gate_fp32_ref.c"), "-o", str(so), "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fn = ctypes.CDLL(str(so)).gate_fp32_chain
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]

    def run(x, w, m0, m1):
        x, w = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(w, dtype=np.float32)
        out = np.empty([x.shape[0], w.shape[0]], dtype=np.float32)
        fn(x.ctypes.data, w.ctypes.data, x.shape[0], x.shape[1], w.shape[0], m0, m1, out.ctypes.data)
        return out
    return run


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """x ~ N(0, 1) rounded to dtype, wg ~ N(0, 1) / sqrt(M) in fp32, seeded (CPU tensors; never modified)"""
    T, M, E = shape
    g = torch.Generator().manual_seed(1000 * T + M + E)
    return torch.randn([T, M], generator=g).to(dtype), torch.randn([E, M], generator=g) / M ** 0.5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_chain(chain, part, x, wg, ranges, rows):
    """every part[s][t][e], t in rows, is the fmaf chain over split s's range, bit for bit; reports the first differing element"""
    xr, w = x[rows].float().numpy(), wg.numpy()
    for s, (m0, m1) in enumerate(ranges):
        want = torch.from_numpy(chain(xr, w, m0, m1))
        got = part[s][rows]
        ne = (_bits(got) != _bits(want)).nonzero()
        assert ne.numel() == 0, (f"split {s} (m in [{m0}, {m1})): {ne.shape[0]} elements differ from the fmaf chain; the first at token "
                                 f"{int(rows[int(ne[0][0])])}, expert {int(ne[0][1])}: kernel {float(got[tuple(ne[0])])!r}, "
                                 f"chain {float(want[tuple(ne[0])])!r}")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_partial_sums_are_the_ascending_fmaf_chain_bit_for_bit(chain, shape, dtype):
    ops = _ops()
    T, M, E = shape
    x, wg = _inputs(shape, dtype)
    S = ops.gate_proj_f32w_splits(T, M, E, dtype)
    ranges = ops.gate_proj_f32w_ranges(T, M, E, dtype)
    assert 1 <= S <= 64 and len(ranges) == S and ranges[0][0] == 0 and ranges[-1][1] == M
    assert all(a < b for a, b in ranges) and all(ranges[i][1] == ranges[i + 1][0] for i in range(S - 1)), "contiguous, ascending, none empty"
    part = ops.gate_proj_f32w(x.cuda(), wg.cuda())
    assert part is not None and tuple(part.shape) == (S, T, E) and part.dtype == torch.float32
    part = part.cpu()
    rows = torch.arange(T) if T <= 257 else torch.randperm(T, generator=torch.Generator().manual_seed(T + M))[:256].sort().values
    _check_chain(chain, part, x, wg, ranges, rows)
    # the project's bound on a split-K projection (test_gate_projection_split_k_vs_fp32_reference), every row
    ref = x.double() @ wg.double().t()
    bound = 2e-5 * (x.double().abs() @ wg.double().abs().t()) + 1e-30
    err = (part.double().sum(0) - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", [(100, 192, 12), (257, 2048, 128), (4096, 2048, 64)], **_ids)
def test_topk_on_fp32_partial_sums(shape, dtype):
    """logits == ((p0 + p1) + p2) ... in fp32; idx / gates / scores / workspace are those of gate_topk on these logits; two runs give
    the same bits; ops.gate_logits returns the same logits"""
    ops = _ops()
    T, M, E = shape
    x, wg = (t.cuda() for t in _inputs(shape, dtype))
    part = ops.gate_proj_f32w(x, wg)
    k = 2
    idx, gates, ws, logits, scores = ops.gate_topk_partials(part, torch.float32, k, want_logits=True, want_scores=True)
    assert logits.dtype == gates.dtype == scores.dtype == torch.float32
    acc = part[0].clone()
    for s in range(1, part.shape[0]):
        acc = acc + part[s]
    assert torch.equal(_bits(logits), _bits(acc)), "the partial sums added in split order, in fp32, not rounded again"
    idx2, gates2, ws2, scores2 = ops.gate_topk(logits, k, apply_softmax=True, want_scores=True)
    assert torch.equal(idx, idx2) and torch.equal(_bits(gates), _bits(gates2)) and torch.equal(_bits(scores), _bits(scores2))
    assert torch.equal(ws, ws2), "per-tile histograms and score column sums"
    part_b = ops.gate_proj_f32w(x, wg)
    assert torch.equal(_bits(part_b), _bits(part))
    again = ops.gate_topk_partials(part_b, torch.float32, k, want_logits=True, want_scores=True)
    assert all(torch.equal(a, b) for a, b in zip((idx, ws), (again[0], again[2])))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((gates, logits, scores), (again[1], again[3], again[4])))
    mine = ops.gate_logits(x, wg)
    assert mine.dtype == torch.float32 and torch.equal(_bits(mine), _bits(logits))


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", [(100, 192, 12), (65, 64, 128)], **_ids)
def test_guard_bands_stay_untouched(chain, shape, dtype):
    """x, wg and the partial sums each sit inside NaN bands: ragged T and E are clamped on the load and masked on the store"""
    from _packed_fuzz import moat_intact, moated
    ops = _ops()
    T, M, E = shape
    x, wg = _inputs(shape, dtype)
    S = ops.gate_proj_f32w_splits(T, M, E, dtype)
    xm, wm = moated(x.cuda()), moated(wg.cuda())
    pm = moated(torch.full([S, T, E], float("nan"), dtype=torch.float32, device="cuda"))
    out = ops.gate_proj_f32w(xm, wm, partials=pm)
    torch.cuda.synchronize()
    assert out.data_ptr() == pm.data_ptr()
    for view, what in ((xm, "x"), (wm, "wg"), (pm, "partials")):
        moat_intact(view, what)
    assert torch.equal(xm.cpu(), x) and torch.equal(wm.cpu(), wg), "the operands themselves"
    part = pm.cpu()
    assert bool(torch.isfinite(part).all()), "a value from a band reached a result"
    _check_chain(chain, part, x, wg, ops.gate_proj_f32w_ranges(T, M, E, dtype), torch.arange(T))


def test_uncovered_shapes_are_refused_before_anything_is_enqueued():
    from tutel_amd import _lib
    ops = _ops()
    L = _lib.lib()
    sentinel = 12345.0
    for T, M, E, dt in [(128, 2048, 256, torch.bfloat16), (128, 2040, 64, torch.bfloat16), (128, 2048, 6, torch.float16),
                        (128, 2048, 64, torch.float32)]:
        assert ops.gate_proj_f32w_splits(T, M, E, dt) == 0
        assert L.tutel_amd_gate_proj_f32w_splits(T, M, E, {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16, torch.float32: _lib.F32}[dt]) == 0
        assert ops.gate_proj_f32w_ranges(T, M, E, dt) == []
        x = torch.zeros([T, M], dtype=dt, device="cuda")
        wg = torch.zeros([E, M], dtype=torch.float32, device="cuda")
        p = torch.full([64 * T * E], sentinel, dtype=torch.float32, device="cuda")
        rc = L.tutel_amd_gate_proj_f32w(x.data_ptr(), wg.data_ptr(), ops._code(x), T, M, E, p.data_ptr(), p.numel() * 4, None)
        assert rc == _lib.ENOTSUP and b"not covered" in L.tutel_amd_last_error()
        torch.cuda.synchronize()
        assert bool((p == sentinel).all()), "nothing was enqueued"
        if dt != torch.float32:
            assert ops.gate_proj_f32w(x, wg) is None
    # the 16-bit kernel's query still names the 16-bit kernel only
    assert ops.gate_proj_splits(128, 2048, 64, torch.float32) == 0 and L.tutel_amd_gate_proj_splits(128, 2048, 64, _lib.F32) == 0
    x = torch.zeros([128, 2048], dtype=torch.bfloat16, device="cuda")
    wg = torch.zeros([64, 2048], dtype=torch.float32, device="cuda")
    p = torch.full([4], sentinel, dtype=torch.float32, device="cuda")
    rc = L.tutel_amd_gate_proj_f32w(x.data_ptr(), wg.data_ptr(), _lib.BF16, 128, 2048, 64, p.data_ptr(), 16, None)
    assert rc != 0 and rc != _lib.ENOTSUP and b"too small" in L.tutel_amd_last_error()
    torch.cuda.synchronize()
    assert bool((p == sentinel).all())
