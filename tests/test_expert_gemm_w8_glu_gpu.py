"""The W8A16 gate / up GEMM of SwiGLU experts (csrc/expert_gemm_w8.hip, tutel_amd_expert_gemm_w8_glu) on the MI355X, against its written
contract (include/tutel_amd.h): every e4m3 code through the up half and through the gate half, operands chosen so that every partial
sum and both scaled values are exact in fp32 (the output then equals the contract done step by step on the CPU, whatever the K order),
random operands against float64 of the exact dequantised weights at the 16-bit gated kernels' own bar, the gathered form against the
bucket form, guard bands around every device operand, and the refusals."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _gemm_fuzz as GF                            # noqa: E402
from _packed_fuzz import moat_intact, moated       # noqa: E402

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
# (E_loc, R, H, K): one row, one channel group, one K-tile; ragged rows, a ragged channel tile, an odd number of K-tiles; one row past
# a row tile, two channel tiles; three row and three channel tiles with slivers, K longer than the weight ring; the tuned case
SHAPES = [(3, 1, 16, 64), (2, 127, 48, 192), (2, 129, 80, 64), (1, 300, 144, 1024), (4, 128, 128, 512)]
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
OUT_FILL = 1234.0
ONE = 0x38   # the code of 1.0
SALT = 1     # of the exact operands' seeds: chosen so that every reference is at least a quarter finite and non-zero (asserted below)


def _mods():
    from tutel_amd import ops
    from tutel_amd.experts import w8
    return ops, w8


def _run(a, q_gate, q_up, s_gate, s_up, act, slot_map=None, R=None):
    """one launch with every device operand inside guard bands (NaN around A and the scales, the NaN code around the image, an in-range
    index around the slot map, a sentinel in and around the output); the bands are checked after the launch"""
    ops, w8 = _mods()
    E, H, K = q_gate.shape
    dev = torch.device("cuda")
    ad = moated(a, device=dev)
    img = moated(w8.pack(w8.interleave_gate_up(q_gate, q_up)), fill=0x7F, device=dev)
    sd = moated(w8.interleave_gate_up(s_gate, s_up).contiguous(), device=dev)
    sm = moated(slot_map, fill=0, device=dev) if slot_map is not None else None
    rows = a.shape[1] if slot_map is None else R
    out = moated(torch.full([E, rows, H], OUT_FILL, dtype=a.dtype), fill=OUT_FILL, device=dev)
    got = ops.expert_gemm_w8_glu(ad, img, sd, H, K, act=act, slot_map=sm, R=R, out=out)
    assert got is out
    torch.cuda.synchronize()
    for t, what in ((ad, "A"), (img, "the image"), (sd, "the scales"), (sm, "the slot map"), (out, "D")):
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
    channels (two 16-channel groups: both halves of an image group, every register of a lane) every byte position sees every code"""
    n = torch.arange(32).view(32, 1)
    k = torch.arange(256).view(1, 256)
    return ((k + n) % 256).to(torch.uint8).view(1, 32, 256)


@pytest.mark.parametrize("half", ["up", "gate"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_every_code_is_widened_exactly_through_either_half(dtype, half):
    """A the identity, the other half all 1.0, scales 1, no activation: D[r, n] = dq(code[n, r]) * 1 exactly"""
    codes = _all_codes()
    nan = (codes & 0x7F) == 0x7F
    eye = torch.eye(256, dtype=dtype).view(1, 256, 256)
    one = torch.ones([1, 32])
    ones = torch.full_like(codes, ONE).view(F8)
    finite = torch.where(nan, torch.zeros_like(codes), codes).view(F8)   # (0 * NaN would spread over a NaN code's whole channel)

    def run(q):
        return _run(eye, q, ones, one, one, "none") if half == "gate" else _run(eye, ones, q, one, one, "none")

    out = run(finite)
    want = finite.float()[0].t().contiguous()   # [k, n]
    assert torch.isfinite(want).all() and want.unique().numel() == 253   # 254 finite codes, +0 and -0 one value
    assert bool((want.to(dtype).float() == want).all()), "every finite code is a value of the dtype"
    assert torch.equal(out[0].float(), want), "a finite code is not widened to its exact value"   # +-0 by value
    # all 256 codes: the NaN codes come out as NaN where they stand
    out = run(codes.view(F8))
    assert bool(torch.isnan(out[0].float())[nan[0].t()].all())


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_nan_codes_poison_their_own_output_channel_only(dtype):
    """0x7F in gate channel 5 and 0xFF in up channel 20 make exactly output channels 5 and 20 NaN"""
    codes = _all_codes()
    finite = torch.where((codes & 0x7F) == 0x7F, torch.zeros_like(codes), codes)
    eye = torch.eye(256, dtype=dtype).view(1, 256, 256)
    one = torch.ones([1, 32])
    gate, up = torch.full_like(codes, ONE), finite.clone()
    gate[0, 5, 9], up[0, 20, 200] = 0x7F, 0xFF
    out = _run(eye, gate.view(F8), up.view(F8), one, one, "none")[0].float()
    want = finite.view(F8).float()[0].t().contiguous()
    bad = torch.zeros([256, 32], dtype=torch.bool)
    bad[:, 5] = bad[:, 20] = True
    assert bool(torch.isnan(out[bad]).all()) and torch.equal(out[~bad], want[~bad])


# ---- exact arithmetic -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_inputs(shape):
    """A in {-1, 0, 1}, the e4m3 integers {-2 .. 2} as codes, scales 2^-3 .. 1: every product, every partial sum in any order
    (|sum| <= 2 K <= 2048 < 2^24) and both scaled values (multiples of 2^-3 below 2^11) are exact in fp32"""
    E, R, H, K = shape
    g = torch.Generator().manual_seed(4099 * E + 17 * R + 3 * H + K + SALT)
    a = torch.randint(-1, 2, [E, R, K], generator=g).float()
    qg = torch.randint(-2, 3, [E, H, K], generator=g).float().to(F8)
    qu = torch.randint(-2, 3, [E, H, K], generator=g).float().to(F8)
    sg = torch.pow(2.0, torch.randint(-3, 1, [E, H], generator=g).float())
    su = torch.pow(2.0, torch.randint(-3, 1, [E, H], generator=g).float())
    T = max(R, 8) + 3
    smap = torch.randint(0, 4 * T, [E * R], generator=g, dtype=torch.int32)
    smap[torch.rand([E * R], generator=g) < 0.25] = -1
    smap[0] = -1
    smap[-1] = 4 * T - 1
    x = torch.randint(-1, 2, [T, K], generator=g).float()
    return a, qg, qu, sg, su, smap, x


def _encode(x, smap, E, R):
    """the materialised fast_encode with unit gates: row (e, r) = x[smap % T], zeros where smap < 0"""
    rows = x[(smap.long() % x.shape[0])].clone()
    rows[smap < 0] = 0
    return rows.view(E, R, x.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def _exact_want(shape, gathered, act, dtype):
    """the contract step by step on the CPU in fp32: [E, R, H] in the dtype, computed once, never modified"""
    a, qg, qu, sg, su, smap, x = _exact_inputs(shape)
    if gathered:
        a = _encode(x, smap, shape[0], shape[1])
    gacc = torch.einsum("erk,ehk->erh", a.double(), qg.double())
    uacc = torch.einsum("erk,ehk->erh", a.double(), qu.double())
    assert torch.equal(gacc.float().double(), gacc) and torch.equal(uacc.float().double(), uacc)
    gs, us = gacc.float() * sg.unsqueeze(1), uacc.float() * su.unsqueeze(1)          # one fp32 multiply each
    assert torch.equal(gs.double(), gacc * sg.double().unsqueeze(1)) and torch.equal(us.double(), uacc * su.double().unsqueeze(1)), "exact in fp32"
    g = (gs.clamp_min(0) if act == "relu" else gs).to(dtype)                         # the activation in fp32, ONE rounding of the gate
    return (g.float() * us).to(dtype)                                                # one fp32 multiply, one rounding


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_exact_operands_equal_the_contract_step_by_step(shape, dtype, act):
    ops, _ = _mods()
    a, qg, qu, sg, su, smap, x = _exact_inputs(shape)
    assert ops.gemm_w8_glu_supported(dtype, shape[2], shape[3])
    for gathered in (False, True):
        want = _exact_want(shape, gathered, act, dtype)
        assert not torch.isnan(want.float()).any(), "the reference holds no NaN"
        live = torch.isfinite(want.float()) & (want.float() != 0)
        assert int(live.sum()) * 4 >= want.numel(), f"only {int(live.sum())} of {want.numel()} reference elements are finite and non-zero"
        if gathered:
            out = _run(x.to(dtype), qg, qu, sg, su, act, slot_map=smap, R=shape[1])
            again = _run(x.to(dtype), qg, qu, sg, su, act, slot_map=smap, R=shape[1])
            bucket = _run(_encode(x, smap, shape[0], shape[1]).to(dtype), qg, qu, sg, su, act)
            _same(out, bucket, "gathered form against bucket form")
        else:
            out = _run(a.to(dtype), qg, qu, sg, su, act)
            again = _run(a.to(dtype), qg, qu, sg, su, act)
        _same(out, want, "kernel against the contract on the CPU" + (" (gathered)" if gathered else ""))
        _same(again, out, "a second run")


# ---- random operands --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_inputs(shape, dtype):
    """The operands the bar is held at: drawn by the gated GEMM fuzz's own generator for its gate_up form (tests/_gemm_fuzz.py::
    make_glu_inputs: a ~ N(0, 1), both weights ~ U(-1, 1) / sqrt(K), every product of standard deviation 0.58), rounded to the dtype,
    the weights then quantised by the module's own quantiser; the EXACT dequantised weights q * scale in float64 (computed once,
    never modified).  The bar is held on these operands, as the 16-bit gate_up kernel's is, because it is not a bound of the contract
    for every input: the gate is rounded from an fp32 activation, which falls on the other side of a rounding tie than the float64
    gate about once in 2^12 elements (fp16), and where such a flip meets a gate just above a power of two (ulp(g) = eps g), an
    unfavourable rounding of the output and |ref| > floor / (eps / 2) = 0.61, the element is at up to 1.5 eps |ref| -- past
    eps |ref| + floor.  A first draw of this test with wider weights (N(0, 1) / sqrt(K)) had one such element in 12192 at
    (2, 127, 48, 192), gelu, fp16: g = 0.25098 against G = 0.25073, ref = 0.625, error / bound = 1.07; the contract replayed on the
    CPU gives the same figure."""
    _, w8 = _mods()
    E, R, H, K = shape
    a, wg, _, _, wu = GF.make_glu_inputs(dict(dtype={torch.bfloat16: "bf16", torch.float16: "f16"}[dtype], E=E, R=R, N=H, K=K, kmajor=True,
                                              bias=False, form="gate_up", act="silu", seed=7919 * E + 31 * R + H + 3 * K))
    qg, sg = w8.quantize_e4m3(wg, True)
    qu, su = w8.quantize_e4m3(wu, True)
    return a, qg, qu, sg, su, qg.double() * sg.double().unsqueeze(2), qu.double() * su.double().unsqueeze(2)


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape,act", [(s, "silu") for s in SHAPES] + [(SHAPES[1], "gelu"), (SHAPES[1], "relu"), (SHAPES[1], "none")], **_ids)
def test_random_operands_against_float64_of_the_dequantised_weights(shape, act, dtype):
    """the bar the 16-bit gated kernels are held to (tests/_gemm_fuzz.py::glu_bound), G the float64 gate rounded to the dtype"""
    a, qg, qu, sg, su, dg, du = _random_inputs(shape, dtype)
    out = _run(a, qg, qu, sg, su, act)
    G = GF.ref_gate(a, dg, act, dtype)
    ref, _ = GF.ref_glu(a, du, None, True, "none", G, dtype)
    bound = GF.glu_bound(ref, G, dtype)
    err = (out.double() - ref).abs()
    print(f"w8 glu {shape} {act} {dtype}: max abs error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}, "
          f"max of |ref| {float(ref.abs().max()):.3f}")
    assert torch.isfinite(out.float()).all()
    assert bool((err <= bound).all()), float((err / bound).max())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    ops, w8 = _mods()
    dev = torch.device("cuda")

    def attempt(dtype, H, K, **kw):
        E, R = 2, 5
        a = moated(torch.ones([E, R, K], dtype=dtype), device=dev)
        img = w8.pack(torch.zeros([E, 2 * H, K]).to(F8)).to(dev)
        scale = torch.ones([E, 2 * H], device=dev)
        out = moated(torch.full([E, R, H], OUT_FILL, dtype=dtype), fill=OUT_FILL, device=dev)
        got = ops.expert_gemm_w8_glu(a, img, scale, H, K, out=out, **kw)
        torch.cuda.synchronize()
        moat_intact(out, "D")
        return got, bool((out == torch.full([1], OUT_FILL, dtype=dtype).item()).all())

    got, untouched = attempt(torch.bfloat16, 32, 128)
    assert got is not None and not untouched and bool((got == 0).all()), "the covered case, so that each refusal below shows"
    counts = torch.full([2], 3, dtype=torch.int32, device=dev)
    for dtype, H, K, kw in ((torch.bfloat16, 32, 128, dict(row_counts=counts)), (torch.bfloat16, 24, 128, {}), (torch.bfloat16, 32, 96, {}),
                            (torch.float16, 40, 64, {}), (torch.float32, 32, 128, {})):
        got, untouched = attempt(dtype, H, K, **kw)
        assert got is None and untouched, (dtype, H, K, kw)
