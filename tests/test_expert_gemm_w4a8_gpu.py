"""W4A8 (csrc/expert_gemm_w4a8.hip) on the MI355X against its contract (include/tutel_amd.h): every e2m1 code under every admitted scale
byte in every position (this pins the operand order, the lane swap and the scale-byte selection), exact operands against float64
through the epilogue once, random operands against float64 of both dequantised operands, refusals.  Inputs: the W4A16 test's."""
import pytest
import torch
from _packed_fuzz import moat_intact, moated
from test_expert_gemm_w4_gpu import DTYPES, OUT_FILL, _act64, _encode, _exact_inputs, _gemm_tol, _ids, _mods, _pack_nibbles, _same

pytestmark = pytest.mark.gpu

# (E_loc, R, N, K): one tile; an odd count of K-tiles (a half-used scale dword); ragged rows / channels, two row tiles; K-tiles > the ring
SHAPES = [(3, 1, 32, 64), (2, 127, 96, 192), (2, 129, 160, 64), (1, 300, 288, 1024)]
F8, ONE, NAN = torch.float8_e4m3fn, 0x38, 0x7F   # e4m3, its codes of 1.0 and of NaN


def _run(aq, a_scale, codes, scales, bias, act, dtype, slot_map=None, R=None, glu=False):
    # one launch with every device operand inside guard bands; aq: e4m3 [E, R, K] or [T, K]; codes / scales: the standard layout
    ops, w4, _ = _mods()
    E, N, K = codes.shape[0], codes.shape[1] // (2 if glu else 1), 2 * codes.shape[2]
    out = torch.full([E, aq.shape[1] if slot_map is None else R, N], OUT_FILL, dtype=dtype)
    fills = zip((aq.view(torch.uint8), a_scale.reshape(-1), *w4.pack(codes, scales), bias, slot_map, out), (NAN, None, 0x77, 252, None, 0, OUT_FILL))
    ad, asd, cd, sd, bd, sm, out = moats = [None if t is None else moated(t, fill=f, device=torch.device("cuda")) for t, f in fills]
    got = (ops.expert_gemm_w4a8_glu(ad, asd, cd, sd, N, K, dtype, act=act, slot_map=sm, R=R, out=out) if glu else
           ops.expert_gemm_w4a8(ad, asd, cd, sd, bd, N, K, dtype, act=act, slot_map=sm, R=R, out=out))
    torch.cuda.synchronize()
    assert got is out and all(moat_intact(t) is None for t in moats if t is not None)
    return out.cpu()


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_every_code_under_every_admitted_scale_byte_in_every_position(dtype):
    """32 channels, K = 256 (two scale dwords, four K-tiles): 256 (channel, block) pairs with one scale byte each -- all 251 admitted
    bytes for bf16, the 27 of fp16 repeated, over all four byte positions and both lane halves; every block holds all 16 codes twice,
    rotated so that every nibble position sees every code.  Aq is the e4m3 identity with row scales 1: D[k, n] = w[n, k]."""
    _, w4, _ = _mods()
    lo, hi = w4.SCALE_RANGE[dtype]
    scales = (lo + torch.arange(256).view(32, 8) % (hi - lo + 1)).to(torch.uint8).view(1, 32, 8)
    assert set(scales.flatten().tolist()) == set(range(lo, hi + 1))
    n, b, i = torch.arange(32).view(32, 1, 1), torch.arange(8).view(1, 8, 1), torch.arange(32).view(1, 1, 32)
    codes = _pack_nibbles(((i + n + 3 * b) % 16).view(1, 32, 256))
    w4.check_scales(scales, dtype)
    ref = w4.dequantize(codes, scales, dtype)[0].t().contiguous()
    eye = (torch.eye(256) * ONE).to(torch.uint8).view(1, 256, 256)
    got = _run(eye, torch.ones([256]), codes, scales, None, "none", dtype)[0]
    assert torch.equal(got, ref), f"{int((got != ref).sum())} weights do not come out as their value (by value: the code of -0 gives a zero)"
    if dtype == torch.bfloat16:   # once: the fp8 NaN code as an activation comes out NaN where it stands
        eye[0, 70, 70] = NAN
        got = _run(eye, torch.ones([256]), codes, scales, None, "none", dtype)[0]
        assert bool(torch.isnan(got[70]).all()) and torch.equal(got[:70], ref[:70]) and torch.equal(got[71:], ref[71:])


def _rows(shape, gathered):
    # _exact_inputs' rows ({-3 .. 3}: e4m3 values), row scales 2^-2 .. 2^1 -> (kernel rows, scales, slot map, the rows the GEMM sees, their scales)
    E, R = shape[:2]
    a, _, _, _, smap, x = _exact_inputs(shape)
    st = torch.pow(2.0, (torch.arange(x.shape[0] if gathered else E * R) % 4 - 2.0))
    if not gathered:
        return a.to(F8), st, None, a, st.view(E, R)
    rs = st[smap.long() % x.shape[0]].clone()
    rs[smap < 0] = 1.0
    return x.to(F8), st, smap, _encode(x, smap, E, R), rs.view(E, R)


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_exact_operands_equal_float64_through_the_epilogue_once(shape, dtype, has_bias, act):
    ops, w4, _ = _mods()
    _, codes, scales, bias, _, _ = _exact_inputs(shape)   # block scales 2^-3 .. 2^3
    assert ops.gemm_w4a8_supported(dtype, shape[2], shape[3])
    for gathered in (False, True):
        ka, ks, smap, rows, rs = _rows(shape, gathered)
        acc = torch.einsum("erk,enk->ern", rows.double(), w4.dequantize(codes, scales).double())
        want = _act64(acc * rs.double().unsqueeze(2) + (bias.double().unsqueeze(1) if has_bias else 0), act)
        assert torch.equal(acc.float().double(), acc) and torch.equal(want.float().double(), want), "the reference is exact in fp32"
        out, again = (_run(ka, ks, codes, scales, bias.to(dtype) if has_bias else None, act, dtype, smap, shape[1] if gathered else None) for _ in "12")
        _same(out, want.float().to(dtype), "kernel against float64 through the epilogue once" + (" (gathered)" if gathered else ""))
        _same(again, out, "a second run")


@pytest.mark.parametrize("gathered", [False, True], ids=["plain", "gathered"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("H", [16, 80])
def test_glu_exact_operands(H, dtype, gathered):
    _, w4, w8 = _mods()
    shape = (2, 127, 2 * H, 192)
    _, c, s, _, _, _ = _exact_inputs(shape)
    ka, ks, smap, rows, rs = _rows(shape, gathered)
    gate, up = (torch.einsum("erk,enk->ern", rows.double(), w4.dequantize(c[:, h], s[:, h]).double()) * rs.double().unsqueeze(2)
                for h in (slice(0, H), slice(H, 2 * H)))
    assert torch.equal(gate.float().double(), gate) and torch.equal(up.float().double(), up), "both products are exact in fp32"
    # the gate rounded once; the exact product rounded to fp32 as __fmul_rn does, then once
    want = (gate.clamp_min(0).float().to(dtype).double() * up).float().to(dtype)
    out = _run(ka, ks, w8.interleave_gate_up(c[:, :H], c[:, H:]), w8.interleave_gate_up(s[:, :H], s[:, H:]), None, "relu", dtype,
               smap, shape[1] if gathered else None, glu=True)
    _same(out, want, "the gate / up kernel against float64 through the epilogue once")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape,act", [(SHAPES[1], a) for a in ("gelu", "silu", "relu", "none")] + [((5, 128, 256, 2048), "relu")], **_ids)
def test_random_operands_against_float64_of_both_dequantised_operands(shape, act, dtype):
    _, w4, w8 = _mods()
    E, R, N, K = shape
    g = torch.Generator().manual_seed(7919 * E + 31 * R + N + 3 * K)
    a, w, bias = (torch.randn(s, generator=g).to(dtype) for s in ([E, R, K], [E, N, K], [E, N]))
    qa, sa = w8.quantize_e4m3(a, True)
    codes, scales = w4.quantize_mxfp4((w.float() / K ** 0.5).to(dtype), True, dtype)
    want = _act64(torch.einsum("erk,enk->ern", qa.double() * sa.double().unsqueeze(2), w4.dequantize(codes, scales).double())
                  + bias.double().unsqueeze(1), act)
    out = _run(qa, sa, codes, scales, bias, act, dtype)
    print(f"w4a8 {shape} {act} {dtype}: max abs error {float((out.double() - want).abs().max()):.3e}, max of |want| {float(want.abs().max()):.3f}")
    torch.testing.assert_close(out.double(), want, **_gemm_tol(dtype))


def test_refusals_leave_the_output_untouched():
    ops, w4, _ = _mods()
    dev = torch.device("cuda")

    def attempt(dtype, N, K, E=2, R=5, small_image=False, **kw):
        Ni = 32 if small_image else 64   # 64 channels of K = 128: an image that would do for every case below, but for small_image
        ci, si = w4.pack(torch.zeros([E, Ni, 64], dtype=torch.uint8), torch.full([E, Ni, 4], 127, dtype=torch.uint8))
        out = moated(torch.full([E, R, N], OUT_FILL, dtype=dtype), fill=OUT_FILL, device=dev)
        got = ops.expert_gemm_w4a8(torch.full([E, R, K], ONE, dtype=torch.uint8, device=dev), torch.ones([E * R], device=dev), ci.to(dev),
                                   si.to(dev), None, N, K, dtype, out=out, **kw)
        torch.cuda.synchronize()
        moat_intact(out, "D")
        return got, bool((out == torch.full([], OUT_FILL, dtype=dtype, device=dev)).all())

    got, untouched = attempt(torch.bfloat16, 64, 128)
    assert got is not None and not untouched and bool((got == 0).all()), "the covered case, so that each refusal below shows"
    counts = torch.full([2], 3, dtype=torch.int32, device=dev)
    for dtype, N, K, kw in ((torch.float32, 64, 128, {}), (torch.bfloat16, 64, 96, {}), (torch.float16, 48, 128, {}),
                            (torch.bfloat16, 64, 128, dict(row_counts=counts)), (torch.bfloat16, 64, 128, dict(small_image=True))):
        assert attempt(dtype, N, K, **kw) == (None, True), (dtype, N, K, kw)
        assert "not covered" in ops._lib.lib().tutel_amd_last_error().decode(), "a refusal carries its reason"
