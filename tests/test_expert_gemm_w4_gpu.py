"""W4A16 (csrc/expert_gemm_w4.hip, tutel_amd_expert_gemm_w4 / _w4_glu) on the MI355X, against its written contract
(include/tutel_amd.h): every e2m1 code under every admitted scale byte widened exactly, operands chosen so that every partial sum is
exact in fp32 (the output then equals the float64 result rounded once, whatever the K order), random operands against float64 of the
exact dequantised weights at the 16-bit GEMM's own tolerance, the gathered form against the bucket form, the GLU launch against two
plain launches, and guard bands around every device operand."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _packed_fuzz import moat_intact, moated  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# (E_loc, R, N, K): one K-tile (shorter than the weight ring), one live wave, one row; a ragged channel tile and K no multiple of 128
# (the last scale dword is half pad); two row tiles, two channel tiles, five K-tiles (odd, no multiple of the ring depth); three row
# tiles and three channel tiles with slivers; the tuned case, 128 rows, a long K
SHAPES = [(3, 1, 32, 64), (2, 127, 96, 192), (2, 129, 160, 320), (1, 300, 288, 1024), (5, 128, 256, 2048)]
GLU_SHAPES = [(3, 1, 16, 64), (2, 127, 48, 192), (2, 129, 80, 320), (1, 200, 144, 1024)]   # (E_loc, R, H, K)
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
OUT_FILL = 1234.0


def _mods():
    from tutel_amd import ops
    from tutel_amd.experts import w4, w8
    return ops, w4, w8


# the W8A16 GPU test's own bar (the project's 16-bit GEMM bar): the accumulator and the single rounding are the same
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


def _run(a, codes, scales, bias, act, slot_map=None, R=None, glu=False):
    """one launch with every device operand inside guard bands (NaN around the inputs, the largest scale byte and code 0x77 = 6.0 around
    the image, an in-range index around the slot map, a sentinel in and around the output); the bands are checked after the launch.
    codes / scales: the standard layout [E, N, K / 2] / [E, N, K / 32] (for glu: the interleaved 2 H channels)"""
    ops, w4, _ = _mods()
    E, N, K = codes.shape[0], codes.shape[1], 2 * codes.shape[2]
    dev = torch.device("cuda")
    ci, si = w4.pack(codes, scales)
    ad = moated(a, device=dev)
    cd = moated(ci, fill=0x77, device=dev)
    sd = moated(si, fill=252, device=dev)
    bd = moated(bias, device=dev) if bias is not None else None
    sm = moated(slot_map, fill=0, device=dev) if slot_map is not None else None
    rows = a.shape[1] if slot_map is None else R
    cols = N // 2 if glu else N
    out = moated(torch.full([E, rows, cols], OUT_FILL, dtype=a.dtype), fill=OUT_FILL, device=dev)
    if glu:
        got = ops.expert_gemm_w4_glu(ad, cd, sd, cols, K, act=act, slot_map=sm, R=R, out=out)
    else:
        got = ops.expert_gemm_w4(ad, cd, sd, bd, N, K, act=act, slot_map=sm, R=R, out=out)
    assert got is out
    torch.cuda.synchronize()
    for t, what in ((ad, "A"), (cd, "the codes"), (sd, "the scales"), (bd, "bias"), (sm, "the slot map"), (out, "D")):
        if t is not None:
            moat_intact(t, what)
    return out.cpu()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    ne = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert ne.numel() == 0, (f"{what}: {ne.shape[0]} of {got.numel()} elements differ; the first at {tuple(int(v) for v in ne[0])}: "
                             f"{float(got[tuple(ne[0])])!r} against {float(want[tuple(ne[0])])!r}")


def _pack_nibbles(c):
    """one code per element [..., K] -> the standard layout [..., K / 2]"""
    c = c.to(torch.uint8).view(*c.shape[:-1], c.shape[-1] // 2, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous()


# ---- every code under every admitted scale ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_every_code_under_every_admitted_scale_is_widened_exactly(dtype):
    """one expert, 32 channels, K = 256: the 8 blocks of each of the 32 channels are 256 (channel, block) pairs with one scale byte
    each -- all 251 admitted bytes for bf16, the 27 of fp16 repeated; every block holds all 16 codes twice, rotated by channel and
    block so that every nibble position of a lane's dwords sees every code.  A is the identity: D[k, n] = w[n, k]."""
    _, w4, _ = _mods()
    lo, hi = w4.SCALE_RANGE[dtype]
    pair = torch.arange(256).view(32, 8)                       # (channel, block) -> 0 .. 255
    scales = (lo + pair % (hi - lo + 1)).to(torch.uint8).view(1, 32, 8)
    assert set(scales.flatten().tolist()) == set(range(lo, hi + 1))
    n = torch.arange(32).view(32, 1, 1)
    b = torch.arange(8).view(1, 8, 1)
    i = torch.arange(32).view(1, 1, 32)
    codes = _pack_nibbles(((i + n + 3 * b) % 16).view(1, 32, 256))
    w4.check_scales(scales, dtype)
    want = w4.dequantize(codes, scales, dtype)
    assert torch.equal(want.double(), w4.dequantize(codes, scales, torch.float32).double()), "every value is a value of the dtype"
    out = _run(torch.eye(256, dtype=dtype).view(1, 256, 256), codes, scales, None, "none")
    got, ref = out[0].float(), want[0].t().contiguous().float()
    ne = (got != ref).nonzero()
    assert ne.numel() == 0, (f"{ne.shape[0]} weights are not widened exactly; the first: k {int(ne[0][0])}, channel {int(ne[0][1])}, scale byte "
                             f"{int(scales[0, ne[0][1], ne[0][0] // 32])}: {float(got[tuple(ne[0])])!r} against {float(ref[tuple(ne[0])])!r}")


# ---- exact arithmetic -------------------------------------------------------------------------------------------------------------
def _encode(x, smap, E, R):
    """the materialised fast_encode with unit gates: row (e, r) = x[smap % T], zeros where smap < 0"""
    rows = x[(smap.long() % x.shape[0])].clone()
    rows[smap < 0] = 0
    return rows.view(E, R, x.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def _exact_inputs(shape):
    """A in {-3 .. 3}, random codes, block scales 2^-3 .. 2^3, bias from the W8 test's dyadic set: every product is a multiple of
    2^-4 and |sum| <= 3 * 48 * K = 144 K < 2^19 for K <= 2048, so every partial sum in any order is exact in fp32"""
    E, R, N, K = shape
    g = torch.Generator().manual_seed(4099 * E + 17 * R + 3 * N + K)
    a = torch.randint(-3, 4, [E, R, K], generator=g).float()
    codes = _pack_nibbles(torch.randint(0, 16, [E, N, K], generator=g))
    scales = torch.randint(124, 131, [E, N, K // 32], generator=g).to(torch.uint8)
    bias = torch.tensor([-2.0, -0.5, -0.25, 0.0, 0.25, 1.0, 3.0])[torch.randint(0, 7, [E, N], generator=g)]
    T = max(R, 8) + 3
    smap = torch.randint(0, 4 * T, [E * R], generator=g, dtype=torch.int32)
    smap[torch.rand([E * R], generator=g) < 0.25] = -1
    smap[0] = -1
    smap[-1] = 4 * T - 1
    x = torch.randint(-3, 4, [T, K], generator=g).float()
    return a, codes, scales, bias, smap, x


@functools.lru_cache(maxsize=None)
def _exact_acc(shape, gathered):
    """float64 accumulators [E, R, N], computed once, never modified"""
    _, w4, _ = _mods()
    a, codes, scales, bias, smap, x = _exact_inputs(shape)
    if gathered:
        a = _encode(x, smap, shape[0], shape[1])
    acc = torch.einsum("erk,enk->ern", a.double(), w4.dequantize(codes, scales).double())
    assert torch.equal(acc.float().double(), acc)
    return acc


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_exact_operands_equal_float64_rounded_once(shape, dtype, has_bias, act):
    ops, _, _ = _mods()
    a, codes, scales, bias, smap, x = _exact_inputs(shape)
    assert ops.gemm_w4_supported(dtype, shape[2], shape[3])
    b = bias.to(dtype) if has_bias else None
    for gathered in (False, True):
        v = _exact_acc(shape, gathered)
        if has_bias:
            v = v + bias.double().unsqueeze(1)
        want = _act64(v, act)
        assert torch.equal(want.float().double(), want), "the reference is exact in fp32: one rounding to the dtype follows"
        want = want.float().to(dtype)
        if gathered:
            out = _run(x.to(dtype), codes, scales, b, act, slot_map=smap, R=shape[1])
            again = _run(x.to(dtype), codes, scales, b, act, slot_map=smap, R=shape[1])
            bucket = _run(_encode(x, smap, shape[0], shape[1]).to(dtype), codes, scales, b, act)
            _same(out, bucket, "gathered form against bucket form")
        else:
            out = _run(a.to(dtype), codes, scales, b, act)
            again = _run(a.to(dtype), codes, scales, b, act)
        _same(out, want, "kernel against float64 rounded once" + (" (gathered)" if gathered else ""))
        _same(again, out, "a second run")


# ---- random operands --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_inputs(shape, dtype):
    """a ~ N(0, 1), w ~ N(0, 1) / sqrt(K) quantised by quantize_mxfp4, bias ~ N(0, 1), all rounded to the dtype first; float64
    pre-activations over the EXACT dequantised weights (computed once, never modified)"""
    _, w4, _ = _mods()
    E, R, N, K = shape
    g = torch.Generator().manual_seed(7919 * E + 31 * R + N + 3 * K)
    a = torch.randn([E, R, K], generator=g).to(dtype)
    w = (torch.randn([E, N, K], generator=g) / K ** 0.5).to(dtype)
    bias = torch.randn([E, N], generator=g).to(dtype)
    codes, scales = w4.quantize_mxfp4(w, True, dtype)
    w4.check_scales(scales, dtype)
    pre = torch.einsum("erk,enk->ern", a.double(), w4.dequantize(codes, scales).double()) + bias.double().unsqueeze(1)
    return a, codes, scales, bias, pre


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape,act", [(s, "relu") for s in SHAPES] + [(SHAPES[1], "gelu"), (SHAPES[1], "silu"), (SHAPES[1], "none")], **_ids)
def test_random_operands_against_float64_of_the_dequantised_weights(shape, act, dtype):
    a, codes, scales, bias, pre = _random_inputs(shape, dtype)
    out = _run(a, codes, scales, bias, act)
    want = _act64(pre, act)
    err = (out.double() - want).abs()
    print(f"w4 {shape} {act} {dtype}: max abs error {float(err.max()):.3e}, max of |want| {float(want.abs().max()):.3f}")
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), want, **_gemm_tol(dtype))


# ---- the GLU kernel -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _glu_exact_inputs(shape):
    """gate and up operands of _exact_inputs' kind: (a, codes_gate, scales_gate, codes_up, scales_up, smap, x)"""
    E, R, H, K = shape
    a, cg, sg, _, smap, x = _exact_inputs((E, R, 2 * H, K))
    return a, cg[:, :H].contiguous(), sg[:, :H].contiguous(), cg[:, H:].contiguous(), sg[:, H:].contiguous(), smap, x


def _glu_contract(gacc, uacc, act, dtype):
    """D = round_T( float(round_T(act(gacc))) * uacc ) from float64 accumulators: the activation in float64, the gate rounded to the
    dtype, the product in float64, one rounding"""
    g = _act64(gacc, act).to(dtype)
    return g.double() * uacc


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", GLU_SHAPES, **_ids)
def test_glu_exact_operands_equal_the_contract_and_two_plain_launches(shape, dtype):
    ops, w4, w8 = _mods()
    E, R, H, K = shape
    a, cg, sg, cu, su, smap, x = _glu_exact_inputs(shape)
    assert ops.gemm_w4_glu_supported(dtype, H, K)
    both_c, both_s = w8.interleave_gate_up(cg, cu), w8.interleave_gate_up(sg, su)
    for gathered in (False, True):
        rows = _encode(x, smap, E, R) if gathered else a
        gacc = torch.einsum("erk,ehk->erh", rows.double(), w4.dequantize(cg, sg).double())
        uacc = torch.einsum("erk,ehk->erh", rows.double(), w4.dequantize(cu, su).double())
        assert torch.equal(gacc.float().double(), gacc) and torch.equal(uacc.float().double(), uacc)
        g = gacc.float().clamp_min(0).to(dtype)          # exact accumulators: the activation in fp32, ONE rounding of the gate
        want = (g.float() * uacc.float()).to(dtype)      # one fp32 multiply with its own rounding, one rounding to the dtype
        if gathered:
            out = _run(x.to(dtype), both_c, both_s, None, "relu", slot_map=smap, R=R, glu=True)
            again = _run(x.to(dtype), both_c, both_s, None, "relu", slot_map=smap, R=R, glu=True)
            _same(out, _run(rows.to(dtype), both_c, both_s, None, "relu", glu=True), "gathered form against bucket form")
        else:
            out = _run(a.to(dtype), both_c, both_s, None, "relu", glu=True)
            again = _run(a.to(dtype), both_c, both_s, None, "relu", glu=True)
        _same(out, want, "kernel against the contract on the CPU" + (" (gathered)" if gathered else ""))
        _same(again, out, "a second run")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", [(1, 40, 32, 64), (2, 129, 96, 320)], **_ids)
def test_glu_launch_equals_two_plain_launches(shape, dtype):
    """the GLU launch against two plain W4 launches on the separate gate and up images (H % 32 == 0: the plain kernel's channel
    groups), combined in torch by the contract's formula, bit for bit.  The plain launch rounds uacc to the dtype where the GLU
    launch keeps it in fp32, so the rows are scaled one-hot vectors: every accumulator is ONE product a * w, a in {+-1, +-2}, a value
    of the dtype -- the comparison is about which register meets which, the sums are the other tests'."""
    _, _, w8 = _mods()
    E, R, H, K = shape
    _, cg, sg, cu, su, _, _ = _glu_exact_inputs(shape)
    g = torch.Generator().manual_seed(R + K)
    a = torch.zeros([E * R, K])
    a[torch.arange(E * R), torch.randint(0, K, [E * R], generator=g)] = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, [E * R], generator=g)]
    a = a.view(E, R, K).to(dtype)
    out = _run(a, w8.interleave_gate_up(cg, cu), w8.interleave_gate_up(sg, su), None, "silu", glu=True)
    gate = _run(a, cg, sg, None, "silu")
    up = _run(a, cu, su, None, "none")
    assert int((up.float() != 0).sum()) * 2 >= up.numel()
    _same(out, (gate.float() * up.float()).to(dtype), "the GLU launch against two plain launches")


@functools.lru_cache(maxsize=None)
def _glu_random_inputs(shape, dtype):
    _, w4, _ = _mods()
    E, R, H, K = shape
    g = torch.Generator().manual_seed(7919 * E + 31 * R + H + 3 * K)
    a = torch.randn([E, R, K], generator=g).to(dtype)
    wg = (torch.randn([E, H, K], generator=g) / K ** 0.5).to(dtype)
    wu = (torch.randn([E, H, K], generator=g) / K ** 0.5).to(dtype)
    cg, sg = w4.quantize_mxfp4(wg, True, dtype)
    cu, su = w4.quantize_mxfp4(wu, True, dtype)
    gacc = torch.einsum("erk,ehk->erh", a.double(), w4.dequantize(cg, sg).double())
    uacc = torch.einsum("erk,ehk->erh", a.double(), w4.dequantize(cu, su).double())
    return a, cg, sg, cu, su, gacc, uacc


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", GLU_SHAPES, **_ids)
def test_glu_random_operands_against_the_two_rounding_formula(shape, dtype):
    _, _, w8 = _mods()
    a, cg, sg, cu, su, gacc, uacc = _glu_random_inputs(shape, dtype)
    out = _run(a, w8.interleave_gate_up(cg, cu), w8.interleave_gate_up(sg, su), None, "silu", glu=True)
    want = _glu_contract(gacc, uacc, "silu", dtype)
    err = (out.double() - want).abs()
    print(f"w4 glu {shape} silu {dtype}: max abs error {float(err.max()):.3e}, max of |want| {float(want.abs().max()):.3f}")
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), want, **_gemm_tol(dtype))
