"""W8A16 (csrc/expert_gemm_w8.hip, tutel_amd_expert_gemm_w8) on the MI355X, against its written contract (include/tutel_amd.h): every
e4m3 code widened exactly at every lane position, operands chosen so that every partial sum is exact in fp32 (the output then equals
the float64 result rounded once, whatever the K order), random operands against float64 of the exact dequantised weights at the
16-bit GEMM's own tolerance, the gathered form against the bucket form, guard bands around every device operand, and the refusals."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _packed_fuzz import moat_intact, moated  # noqa: E402

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
# (E_loc, R, N, K): one row; ragged rows and a ragged channel tile, an odd number of K-tiles; one row past a row tile, two channel
# tiles; three row tiles and three channel tiles with slivers, K longer than the weight ring; the tuned case, 128 rows, a long K
SHAPES = [(3, 1, 32, 64), (2, 127, 96, 192), (2, 129, 160, 64), (1, 300, 288, 1024), (5, 128, 256, 2048)]
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
OUT_FILL = 1234.0


def _mods():
    from tutel_amd import ops
    from tutel_amd.experts import w8
    return ops, w8


# the project's 16-bit GEMM bar (tests/test_ops_gpu.py::_gemm_tol), restated: operands scaled by 1 / sqrt(K).  This kernel differs from
# the 16-bit one by a single fp32 multiply per output, so no new constant
def _gemm_tol(dtype):
    return dict(rtol=2.0 ** -7, atol=2e-3) if dtype == torch.bfloat16 else dict(rtol=2.0 ** -10, atol=3e-4)


def _act64(v, act):
    if act == "relu":
        return v.clamp_min(0)
    if act == "gelu":
        return torch.nn.functional.gelu(v)
    if act == "silu":
        return torch.nn.functional.silu(v)
    return v


def _run(a, q, scale, bias, act, slot_map=None, R=None):
    """one launch with every device operand inside guard bands (NaN around the inputs, an in-range index around the slot map, a
    sentinel in and around the output); the bands are checked after the launch"""
    ops, w8 = _mods()
    E, N, K = q.shape
    dev = torch.device("cuda")
    ad = moated(a, device=dev)
    img = moated(w8.pack(q), fill=0x7F, device=dev)   # the NaN code around the image
    sd = moated(scale, device=dev)
    bd = moated(bias, device=dev) if bias is not None else None
    sm = moated(slot_map, fill=0, device=dev) if slot_map is not None else None
    rows = a.shape[1] if slot_map is None else R
    out = moated(torch.full([E, rows, N], OUT_FILL, dtype=a.dtype), fill=OUT_FILL, device=dev)
    got = ops.expert_gemm_w8(ad, img, sd, bd, N, K, act=act, slot_map=sm, R=R, out=out)
    assert got is out
    torch.cuda.synchronize()
    for t, what in ((ad, "A"), (img, "the image"), (sd, "scale"), (bd, "bias"), (sm, "the slot map"), (out, "D")):
        if t is not None:
            moat_intact(t, what)
    return out.cpu()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    ne = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert ne.numel() == 0, (f"{what}: {ne.shape[0]} of {got.numel()} elements differ; the first at {tuple(int(v) for v in ne[0])}: "
                             f"{float(got[tuple(ne[0])])!r} against {float(want[tuple(ne[0])])!r}")


# ---- every code -------------------------------------------------------------------------------------------------------------------
def _all_codes():
    """[1, 32, 256] codes: column k of channel n holds code (k + n) mod 256 -- every channel holds every code once, and over the 32
    channels every position k mod 8 of a lane's operand bytes (and both lane halves, both K-steps) sees every code"""
    n = torch.arange(32).view(32, 1)
    k = torch.arange(256).view(1, 256)
    return ((k + n) % 256).to(torch.uint8).view(1, 32, 256)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_every_code_is_widened_exactly(dtype):
    codes = _all_codes()
    nan = (codes & 0x7F) == 0x7F
    eye = torch.eye(256, dtype=dtype).view(1, 256, 256)
    one = torch.ones([1, 32])
    # the 254 finite codes (the two NaN codes replaced by code 0: 0 * NaN would spread over their whole channel): D[r, n] = dq(code[n, r])
    finite = torch.where(nan, torch.zeros_like(codes), codes).view(F8)
    out = _run(eye, finite, one, None, "none")
    want = finite.float()[0].t().contiguous()   # [k, n]
    assert torch.isfinite(want).all() and want.unique().numel() == 253   # 254 finite codes, +0 and -0 one value
    assert torch.equal(out[0].float(), want), "a finite code is not widened to its exact value"   # +-0 by value
    assert bool((want.to(dtype).float() == want).all()), "every finite code is a value of the dtype"
    # all 256 codes: the NaN codes come out as NaN where they stand
    out = _run(eye, codes.view(F8), one, None, "none")
    assert bool(torch.isnan(out[0].float())[nan[0].t()].all())
    # and NaN propagates through the sum of ITS channel only: channel 5 holds 0x7F, channel 20 holds 0xFF, once each
    poisoned = finite.view(torch.uint8).clone()
    poisoned[0, 5, 9], poisoned[0, 20, 200] = 0x7F, 0xFF
    out = _run(eye, poisoned.view(F8), one, None, "none")[0].float()
    bad = torch.zeros([256, 32], dtype=torch.bool)
    bad[:, 5] = bad[:, 20] = True
    assert bool(torch.isnan(out[bad]).all()) and torch.equal(out[~bad], want[~bad])


# ---- exact arithmetic -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_inputs(shape):
    """A in {-3 .. 3}, q the e4m3 integers {-4 .. 4}, scales 2^-3 .. 2^3, bias from a dyadic set: every product, every partial sum in
    any order (|sum| <= 12 K <= 24576 < 2^24) and the scaled, biased result (a multiple of 2^-3 below 2^18) are exact in fp32"""
    E, R, N, K = shape
    g = torch.Generator().manual_seed(4099 * E + 17 * R + 3 * N + K)
    a = torch.randint(-3, 4, [E, R, K], generator=g).float()
    q = torch.randint(-4, 5, [E, N, K], generator=g).float().to(F8)
    scale = torch.pow(2.0, torch.randint(-3, 4, [E, N], generator=g).float())
    bias = torch.tensor([-2.0, -0.5, -0.25, 0.0, 0.25, 1.0, 3.0])[torch.randint(0, 7, [E, N], generator=g)]
    T = max(R, 8) + 3
    smap = torch.randint(0, 4 * T, [E * R], generator=g, dtype=torch.int32)
    smap[torch.rand([E * R], generator=g) < 0.25] = -1
    smap[0] = -1
    smap[-1] = 4 * T - 1
    x = torch.randint(-3, 4, [T, K], generator=g).float()
    return a, q, scale, bias, smap, x


@functools.lru_cache(maxsize=None)
def _exact_want(shape, gathered):
    """float64 acc * scale [+ bias is added by the caller]: [E, R, N] float64, computed once, never modified"""
    a, q, scale, bias, smap, x = _exact_inputs(shape)
    if gathered:
        a = _encode(x, smap, shape[0], shape[1])
    return torch.einsum("erk,enk->ern", a.double(), q.double()) * scale.double().unsqueeze(1)


def _encode(x, smap, E, R):
    """the materialised fast_encode with unit gates: row (e, r) = x[smap % T], zeros where smap < 0"""
    rows = x[(smap.long() % x.shape[0])].clone()
    rows[smap < 0] = 0
    return rows.view(E, R, x.shape[1]).contiguous()


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_exact_operands_equal_float64_rounded_once(shape, dtype, has_bias, act):
    ops, _ = _mods()
    a, q, scale, bias, smap, x = _exact_inputs(shape)
    assert ops.gemm_w8_supported(dtype, shape[2], shape[3])
    b = bias.to(dtype) if has_bias else None
    for gathered in (False, True):
        v = _exact_want(shape, gathered)
        if has_bias:
            v = v + bias.double().unsqueeze(1)
        want = _act64(v, act)
        assert torch.equal(want.float().double(), want), "the reference is exact in fp32: one rounding to the dtype follows"
        want = want.float().to(dtype)
        if gathered:
            out = _run(x.to(dtype), q, scale, b, act, slot_map=smap, R=shape[1])
            again = _run(x.to(dtype), q, scale, b, act, slot_map=smap, R=shape[1])
            bucket = _run(_encode(x, smap, shape[0], shape[1]).to(dtype), q, scale, b, act)
            _same(out, bucket, "gathered form against bucket form")
        else:
            out = _run(a.to(dtype), q, scale, b, act)
            again = _run(a.to(dtype), q, scale, b, act)
        _same(out, want, "kernel against float64 rounded once" + (" (gathered)" if gathered else ""))
        _same(again, out, "a second run")


# ---- random operands --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_inputs(shape, dtype):
    """a ~ N(0, 1), w ~ N(0, 1) / sqrt(K) quantised by the module's own quantiser, bias ~ N(0, 1), all rounded to the dtype first;
    float64 pre-activations over the EXACT dequantised weights q * scale (computed once, never modified)"""
    _, w8 = _mods()
    E, R, N, K = shape
    g = torch.Generator().manual_seed(7919 * E + 31 * R + N + 3 * K)
    a = torch.randn([E, R, K], generator=g).to(dtype)
    w = (torch.randn([E, N, K], generator=g) / K ** 0.5).to(dtype)
    bias = torch.randn([E, N], generator=g).to(dtype)
    q, scale = w8.quantize_e4m3(w, True)
    pre = torch.einsum("erk,enk->ern", a.double(), q.double() * scale.double().unsqueeze(2)) + bias.double().unsqueeze(1)
    return a, q, scale, bias, pre


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape,act", [(s, "relu") for s in SHAPES] + [(SHAPES[1], "gelu"), (SHAPES[1], "silu"), (SHAPES[1], "none")], **_ids)
def test_random_operands_against_float64_of_the_dequantised_weights(shape, act, dtype):
    a, q, scale, bias, pre = _random_inputs(shape, dtype)
    out = _run(a, q, scale, bias, act)
    want = _act64(pre, act)
    err = (out.double() - want).abs()
    tol = _gemm_tol(dtype)
    print(f"w8 {shape} {act} {dtype}: max abs error {float(err.max()):.3e}, max of |want| {float(want.abs().max()):.3f}")
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), want, **tol)


# ---- the quantiser on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32] + DTYPES, **_ids)
@pytest.mark.parametrize("w_kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_quantiser_gives_the_same_bits_on_the_device_as_on_the_cpu(dtype, w_kmajor):
    """the layer quantises where its parameters live: codes and scales must not depend on the device (a division by 448 that the
    device turns into a multiplication by 1 / 448 moves scales by an ulp and flips codes on rounding ties)"""
    _, w8 = _mods()
    w = (torch.randn([8, 256, 256], generator=torch.Generator().manual_seed(12)) / 16).to(dtype)
    w[0, 3] = 0
    q, scale = w8.quantize_e4m3(w, w_kmajor)
    qd, sd = w8.quantize_e4m3(w.cuda(), w_kmajor)
    assert torch.equal(sd.cpu().view(torch.int32), scale.view(torch.int32)), "scales"
    assert torch.equal(qd.cpu().view(torch.uint8), q.view(torch.uint8)), "codes"
    assert torch.equal(w8.pack(qd).cpu(), w8.pack(q)) and torch.equal(w8.unpack(w8.pack(qd), 256, 256).cpu().view(torch.uint8), q.view(torch.uint8))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    ops, w8 = _mods()
    dev = torch.device("cuda")

    def attempt(dtype, N, K, **kw):
        E, R = 2, 5
        a = moated(torch.ones([E, R, K], dtype=dtype), device=dev)
        img = w8.pack(torch.zeros([E, N, K]).to(F8)).to(dev)
        scale = torch.ones([E, N], device=dev)
        out = moated(torch.full([E, R, N], OUT_FILL, dtype=dtype), fill=OUT_FILL, device=dev)
        got = ops.expert_gemm_w8(a, img, scale, None, N, K, out=out, **kw)
        torch.cuda.synchronize()
        moat_intact(out, "D")
        return got, bool((out == torch.full([1], OUT_FILL, dtype=dtype).item()).all())

    got, untouched = attempt(torch.bfloat16, 64, 128)
    assert got is not None and not untouched and bool((got == 0).all()), "the covered case, so that each refusal below shows"
    counts = torch.full([2], 3, dtype=torch.int32, device=dev)
    for dtype, N, K, kw in ((torch.bfloat16, 64, 128, dict(row_counts=counts)), (torch.bfloat16, 48, 128, {}), (torch.bfloat16, 64, 96, {}),
                            (torch.float16, 40, 64, {}), (torch.float32, 64, 128, {})):
        got, untouched = attempt(dtype, N, K, **kw)
        assert got is None and untouched, (dtype, N, K, kw)
