"""W8A8 (csrc/expert_gemm_w8a8.hip, tutel_amd_expert_gemm_w8a8 / _glu) on the MI355X, against its written contract
(include/tutel_amd.h): every e4m3 code through the fp8 matrix instruction as a weight and as an activation, operands whose every
partial sum is exact in fp32 (the output then equals the float64 result pushed through the epilogue once, whatever the order inside
an instruction), random operands against float64 of both dequantised operands at the 16-bit GEMM's own tolerance, and the refusals.
Helpers and inputs are the W8A16 test's, with a row scale added."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _packed_fuzz import moat_intact, moated  # noqa: E402
from test_expert_gemm_w8_gpu import DTYPES, F8, OUT_FILL, _act64, _all_codes, _encode, _exact_inputs, _gemm_tol, _ids, _same  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 32, 64), (2, 127, 96, 192), (2, 129, 160, 64), (1, 300, 288, 1024)]
ONE = 0x38   # the e4m3 code of 1.0


def _mods():
    from tutel_amd import ops
    from tutel_amd.experts import w8
    return ops, w8


def _run(aq, a_scale, q, scale, bias, act, dtype, slot_map=None, R=None, glu=False):
    """one launch with every device operand inside guard bands (the NaN code around both code arrays); aq: e4m3 [E, R, K] or [T, K],
    q: e4m3 [E, N, K] (glu: the interleaved gate / up codes, scale [E, 2 H])"""
    ops, w8 = _mods()
    E, N, K = q.shape
    dev = torch.device("cuda")
    ad = moated(aq.view(torch.uint8), fill=0x7F, device=dev)
    asd = moated(a_scale.reshape(-1), device=dev)
    img = moated(w8.pack(q), fill=0x7F, device=dev)
    sd = moated(scale, device=dev)
    bd = moated(bias, device=dev) if bias is not None else None
    sm = moated(slot_map, fill=0, device=dev) if slot_map is not None else None
    rows = aq.shape[1] if slot_map is None else R
    out = moated(torch.full([E, rows, N // 2 if glu else N], OUT_FILL, dtype=dtype), fill=OUT_FILL, device=dev)
    if glu:
        got = ops.expert_gemm_w8a8_glu(ad, asd, img, sd, N // 2, K, dtype, act=act, slot_map=sm, R=R, out=out)
    else:
        got = ops.expert_gemm_w8a8(ad, asd, img, sd, bd, N, K, dtype, act=act, slot_map=sm, R=R, out=out)
    assert got is out
    torch.cuda.synchronize()
    for t, what in ((ad, "Aq"), (asd, "a_scale"), (img, "the image"), (sd, "scale"), (bd, "bias"), (sm, "the slot map"), (out, "D")):
        if t is not None:
            moat_intact(t, what)
    return out.cpu()


# ---- every code through the instruction ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_every_code_is_multiplied_exactly_as_weight_and_as_activation(dtype):
    codes = _all_codes()   # [1, 32, 256]: column k of channel n holds code (k + n) mod 256
    nan = (codes & 0x7F) == 0x7F
    finite = torch.where(nan, torch.zeros_like(codes), codes)
    want = finite.view(F8).float()[0]   # [32, 256]
    assert bool((want.to(dtype).float() == want).all()), "every finite code is a value of the dtype"
    eye = (torch.eye(256) * ONE).to(torch.uint8).view(1, 256, 256)
    # as weights: token row r holds the single code 1.0 at k = r, D[r, n] = val(code[n, r])
    out = _run(eye.view(F8), torch.ones([256]), finite.view(F8), torch.ones([1, 32]), None, "none", dtype)
    assert torch.equal(out[0].float(), want.t()), "a weight code's product with 1.0 is not its value"
    # as activations: the 32 code rows are the token rows, channel n holds 1.0 at k = n, D[r, n] = val(code[r, n])
    out = _run(finite.view(F8), torch.ones([32]), eye.view(F8), torch.ones([1, 256]), None, "none", dtype)
    assert torch.equal(out[0].float(), want), "an activation code's product with 1.0 is not its value"
    # the NaN codes come out as NaN where they stand, in either role
    out = _run(eye.view(F8), torch.ones([256]), codes.view(F8), torch.ones([1, 32]), None, "none", dtype)
    assert bool(torch.isnan(out[0].float())[nan[0].t()].all())
    out = _run(codes.view(F8), torch.ones([32]), eye.view(F8), torch.ones([1, 256]), None, "none", dtype)
    assert bool(torch.isnan(out[0].float())[nan[0]].all())


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _row_scales(shape):
    """power-of-two row scales 2^-2 .. 2^1 for the bucket rows [E, R] and the tokens [T] of _exact_inputs(shape): with |acc| <= 12 K
    < 2^14 and channel scales 2^-3 .. 2^3 every scaled, biased result is a multiple of 2^-5 below 2^18 -- exact in fp32"""
    E, R, N, K = shape
    T = _exact_inputs(shape)[5].shape[0]
    g = torch.Generator().manual_seed(977 * E + R + K)
    return (torch.pow(2.0, torch.randint(-2, 2, [E, R], generator=g).float()), torch.pow(2.0, torch.randint(-2, 2, [T], generator=g).float()))


def _gathered_scales(sa_tok, smap, E, R):
    s = sa_tok[smap.long() % sa_tok.numel()].clone()
    s[smap < 0] = 1.0
    return s.view(E, R)


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_exact_operands_equal_float64_through_the_epilogue_once(shape, dtype, has_bias, act):
    ops, _ = _mods()
    E, R, N, K = shape
    a, q, scale, bias, smap, x = _exact_inputs(shape)   # small integers: every one an e4m3 value
    sa, sa_tok = _row_scales(shape)
    assert ops.gemm_w8a8_supported(dtype, N, K)
    b = bias.to(dtype) if has_bias else None
    for gathered in (False, True):
        rows, rs = (_encode(x, smap, E, R), _gathered_scales(sa_tok, smap, E, R)) if gathered else (a, sa)
        v = torch.einsum("erk,enk->ern", rows.double(), q.double()) * rs.double().unsqueeze(2) * scale.double().unsqueeze(1)
        if has_bias:
            v = v + bias.double().unsqueeze(1)
        want = _act64(v, act)
        assert torch.equal(want.float().double(), want), "the reference is exact in fp32: one rounding to the dtype follows"
        want = want.float().to(dtype)
        if gathered:
            out = _run(x.to(F8), sa_tok, q, scale, b, act, dtype, slot_map=smap, R=R)
            again = _run(x.to(F8), sa_tok, q, scale, b, act, dtype, slot_map=smap, R=R)
        else:
            out = _run(a.to(F8), sa, q, scale, b, act, dtype)
            again = _run(a.to(F8), sa, q, scale, b, act, dtype)
        _same(out, want, "kernel against float64 through the epilogue once" + (" (gathered)" if gathered else ""))
        _same(again, out, "a second run")


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("H", [16, 80])
def test_glu_exact_operands(H, dtype):
    _, w8 = _mods()
    E, R, K = 2, 127, 192
    a, qg, sg, _, smap, x = _exact_inputs((E, R, H, K))
    _, qu, su, _, _, _ = _exact_inputs((E, R + 1, H, K))   # (another seed: the up matrix)
    qu, su = qu[:, :H], su[:, :H]
    sa, sa_tok = _row_scales((E, R, H, K))
    q, scale = w8.interleave_gate_up(qg, qu), w8.interleave_gate_up(sg, su)
    for gathered in (False, True):
        rows, rs = (_encode(x, smap, E, R), _gathered_scales(sa_tok, smap, E, R)) if gathered else (a, sa)
        pre = [torch.einsum("erk,enk->ern", rows.double(), m.double()) * rs.double().unsqueeze(2) * s.double().unsqueeze(1)
               for m, s in ((qg, sg), (qu, su))]
        gate = pre[0].clamp_min(0).float().to(dtype)                  # exact in fp32, rounded once
        want = (gate.double() * pre[1]).float().to(dtype)              # the exact product rounded to fp32 as __fmul_rn does, then once
        if gathered:
            out = _run(x.to(F8), sa_tok, q, scale, None, "relu", dtype, slot_map=smap, R=R, glu=True)
        else:
            out = _run(a.to(F8), sa, q, scale, None, "relu", dtype, glu=True)
        _same(out, want, "the gate / up kernel against float64 through the epilogue once" + (" (gathered)" if gathered else ""))


# ---- random operands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape,act", [(SHAPES[1], a) for a in ("gelu", "silu", "relu", "none")] + [((5, 128, 256, 2048), "relu")], **_ids)
def test_random_operands_against_float64_of_both_dequantised_operands(shape, act, dtype):
    _, w8 = _mods()
    E, R, N, K = shape
    g = torch.Generator().manual_seed(7919 * E + 31 * R + N + 3 * K)
    a = torch.randn([E, R, K], generator=g).to(dtype)
    w = (torch.randn([E, N, K], generator=g) / K ** 0.5).to(dtype)
    bias = torch.randn([E, N], generator=g).to(dtype)
    qa, sa = w8.quantize_e4m3(a, True)
    qw, sw = w8.quantize_e4m3(w, True)
    want = _act64(torch.einsum("erk,enk->ern", qa.double() * sa.double().unsqueeze(2), qw.double() * sw.double().unsqueeze(2))
                  + bias.double().unsqueeze(1), act)
    out = _run(qa, sa, qw, sw, bias, act, dtype)
    print(f"w8a8 {shape} {act} {dtype}: max abs error {float((out.double() - want).abs().max()):.3e}, max of |want| {float(want.abs().max()):.3f}")
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), want, **_gemm_tol(dtype))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    ops, w8 = _mods()
    dev = torch.device("cuda")

    def attempt(dtype, N, K, small_image=False, **kw):
        E, R = 2, 5
        aq = torch.full([E, R, K], ONE, dtype=torch.uint8, device=dev)
        img = w8.pack(torch.zeros([E, N - (32 if small_image else 0), K]).to(F8)).to(dev)
        out = moated(torch.full([E, R, N], OUT_FILL, dtype=dtype), fill=OUT_FILL, device=dev)
        got = ops.expert_gemm_w8a8(aq, torch.ones([E * R], device=dev), img, torch.ones([E, N], device=dev), None, N, K, dtype, out=out, **kw)
        torch.cuda.synchronize()
        moat_intact(out, "D")
        return got, bool((out == torch.full([1], OUT_FILL, dtype=dtype).item()).all())

    got, untouched = attempt(torch.bfloat16, 64, 128)
    assert got is not None and not untouched and bool((got == 0).all()), "the covered case, so that each refusal below shows"
    counts = torch.full([2], 3, dtype=torch.int32, device=dev)
    for dtype, N, K, kw in ((torch.float32, 64, 128, {}), (torch.bfloat16, 64, 96, {}), (torch.float16, 48, 128, {}),
                            (torch.bfloat16, 64, 128, dict(row_counts=counts)), (torch.bfloat16, 64, 128, dict(small_image=True))):
        got, untouched = attempt(dtype, N, K, **kw)
        assert got is None and untouched, (dtype, N, K, kw)
        assert "not covered" in ops._lib.lib().tutel_amd_last_error().decode(), "a refusal carries its reason"
