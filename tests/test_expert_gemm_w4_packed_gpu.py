"""tutel_amd_expert_gemm_w4_packed / _glu_packed on the MI355X.  The contract (include/tutel_amd.h): a packed row's output is BIT-IDENTICAL
to the padded W4 entry point's for the same input row and expert, whichever window form computed it.  Checked with no tolerance against
the padded kernel on the bucket form of the same rows; against float64 rounded once, on operands whose arithmetic is exact in fp32 (A
and tokens in {-3 .. 3}, all sixteen e2m1 codes, scale bytes 124 .. 130, a dyadic bias: products are multiples of 2^-4 and |sum| <=
144 K < 2^16, 20 significant bits); and the wide form against the halves form (TUTEL_AMD_W4_PACKED_TILE, which the library reads at
every call: both run in this process).  Every device operand and the five layout tables lie in guard bands (0xFF codes and scale bytes
around the images, NaN around A and in its dead rows); D rows at and past offsets[E] keep a sentinel."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _packed_fuzz import gathered, layout_from_rows, moat_intact, moated  # noqa: E402

pytestmark = pytest.mark.gpu

OUT_FILL = 1234.0
TABLES = ("offsets", "tiles", "ntiles", "capacity", "slot_map")
CASES = {   # (rows per expert, alignment, N, K)
    "every_group_count": ([32, 33, 96, 128, 129, 161, 193, 225, 256, 257], 1, 96, 64),   # live groups 1 .. 8, a second table tile of one
                                                                                        # row, a clamped wave, half a scale dword
    "empty_experts_three_ktiles": ([0, 1, 127, 0, 300, 5], 1, 160, 192),   # the scale image's padded dword, K loop shorter than the ring
    "pad_rows_five_ktiles": ([3, 0, 130, 0], 4, 160, 320),                 # -1 pad rows, an empty last expert, a second trip round the ring
    "one_expert_holds_all": ([0, 600, 0], 1, 256, 128),
    "nothing_live": ([0, 0, 0, 0], 1, 32, 64),                             # D keeps its sentinel everywhere
}
# (gathered (fc1) form, bias, activation), the cross product thinned; the GLU form has no bias
COMBOS = [(True, True, "relu"), (False, False, "none"), (True, False, "none"), (False, True, "relu"), (True, True, "gelu"),
          (False, True, "silu"), (True, False, "silu"), (False, False, "gelu")]
GLU_COMBOS = [(True, False, "silu"), (False, False, "silu"), (True, False, "relu"), (False, False, "none"), (True, False, "gelu")]


def _same(got, want, what):
    ne = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert got.shape == want.shape and ne.numel() == 0, f"{what}: {ne.shape[0]} of {got.numel()} elements differ, the first at {ne[:1].tolist()}"


@functools.lru_cache(maxsize=None)
def _layout(name):
    """(layout whose tables are moated copies of the library's, offsets on the host, slot map on the host, T)"""
    rows, align = CASES[name][:2]
    lay, idx, _ = layout_from_rows(rows, align)
    off, slot = lay.offsets.cpu(), lay.slot_map.cpu()
    assert (off[1:] - off[:-1]).tolist() == [(r + align - 1) // align * align for r in rows], "the layout is the one the rows describe"
    for t in TABLES:
        setattr(lay, t, moated(getattr(lay, t).cpu(), fill=0, device=torch.device("cuda")))
    return lay, off, slot, idx.shape[1]


@functools.lru_cache(maxsize=None)
def _inputs(name, channels, amax):
    """A [rows_bound, K] (NaN at and past offsets[E]) and the tokens [T, K] in {-amax .. amax}, codes, scale bytes, bias"""
    rows, _, _, K = CASES[name]
    lay, off, _, T = _layout(name)
    E = len(rows)
    g = torch.Generator().manual_seed(8191 * E + 3 * channels + K)
    a = torch.randint(-amax, amax + 1, [lay.rows_bound, K], generator=g).float()
    a[int(off[-1]):] = float("nan")
    x = torch.randint(-amax, amax + 1, [T, K], generator=g).float()
    codes = torch.randint(0, 256, [E, channels, K // 2], generator=g).to(torch.uint8)
    scales = torch.randint(124, 131, [E, channels, K // 32], generator=g).to(torch.uint8)
    bias = torch.tensor([-2.0, -0.5, -0.25, 0.0, 0.25, 1.0, 3.0])[torch.randint(0, 7, [E, channels], generator=g)]
    return a, x, codes, scales, bias


@functools.lru_cache(maxsize=None)
def _acc64(name, channels, amax, gather):
    """float64 sums of the live packed rows [used, channels] plus the expert of every row, computed once, never modified"""
    from tutel_amd.experts import w4
    a, x, codes, scales, _ = _inputs(name, channels, amax)
    _, off, slot, _ = _layout(name)
    used = int(off[-1])
    expert = torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])
    src = (gathered(x, slot[:used]) if gather else a[:used]).double()
    out = torch.einsum("rk,rnk->rn", src, w4.dequantize(codes, scales).double()[expert])
    assert torch.equal(out.float().double(), out), "the sums are exact in fp32: one rounding to the dtype follows"
    return out, expert


def _bucket(rows_2d, off):
    """[used, K] packed rows -> the bucket form [E, C, K] (rows an expert does not own: zeros)"""
    E, C = off.numel() - 1, max(int((off[1:] - off[:-1]).max()), 1)
    out = torch.zeros([E, C, rows_2d.shape[1]], dtype=rows_2d.dtype)
    for e in range(E):
        out[e, :int(off[e + 1] - off[e])] = rows_2d[int(off[e]):int(off[e + 1])]
    return out


def _packed(name, form, H, a, image, bias, act, gather):
    """one packed launch in the window form `form`, every operand in guard bands -> D on the host"""
    from tutel_amd import ops
    lay, off = _layout(name)[:2]
    dev, K, N = torch.device("cuda"), a.shape[1], CASES[name][2]
    ad, ci, si = moated(a, device=dev), moated(image[0], fill=0xFF, device=dev), moated(image[1], fill=0xFF, device=dev)
    bd = moated(bias, device=dev) if bias is not None else None
    zr = moated(torch.zeros([K], dtype=a.dtype), device=dev) if gather else None
    out = moated(torch.full([lay.rows_bound, H or N], OUT_FILL, dtype=a.dtype), fill=OUT_FILL, device=dev)
    os.environ["TUTEL_AMD_W4_PACKED_TILE"] = form
    try:
        if H:
            got = ops.expert_gemm_w4_glu_packed(ad, ci, si, H, K, lay, act=act, gather=gather, zero_row=zr, out=out)
        else:
            got = ops.expert_gemm_w4_packed(ad, ci, si, bd, N, K, lay, act=act, gather=gather, zero_row=zr, out=out)
    finally:
        del os.environ["TUTEL_AMD_W4_PACKED_TILE"]
    assert got is out
    torch.cuda.synchronize()
    for t in [ad, ci, si, bd, zr, out] + [getattr(lay, n) for n in TABLES]:
        if t is not None:
            moat_intact(t)
    out = out.cpu()
    assert bool((out[int(off[-1]):] == torch.full([1], OUT_FILL, dtype=a.dtype)).all()), "a row at or past offsets[E] was written"
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("H", [None, 48, 128], ids=["plain", "glu48", "glu128"])
@pytest.mark.parametrize("name", list(CASES))
def test_packed_rows_equal_the_padded_kernel_the_other_form_and_float64_rounded_once(name, H, dtype):
    from tutel_amd import ops
    from tutel_amd.experts import w4, w8
    rows, align, N, K = CASES[name]
    channels, amax = (2 * H, 1) if H else (N, 3)   # GLU: channels [0, H) are the gate, [H, 2 H) the up
    a, x, codes, scales, bias = _inputs(name, channels, amax)
    w4.check_scales(scales, dtype)
    _, off, slot, _ = _layout(name)
    used = int(off[-1])
    if H:
        codes, scales = w8.interleave_gate_up(codes[:, :H], codes[:, H:]), w8.interleave_gate_up(scales[:, :H], scales[:, H:])
    image = w4.pack(codes, scales)
    for gather, has_bias, act in (GLU_COMBOS if H else COMBOS):
        what = f"{name} H={H} gather={gather} bias={has_bias} {act}"
        b = bias.to(dtype) if has_bias else None
        out = _packed(name, "wide", H, (x if gather else a).to(dtype), image, b, act, gather)
        _same(out, _packed(name, "halves", H, (x if gather else a).to(dtype), image, b, act, gather), what + ": wide against halves")
        if used == 0:
            continue
        ab = _bucket((gathered(x, slot[:used]) if gather else a[:used]).to(dtype), off).cuda()
        if H:
            padded = ops.expert_gemm_w4_glu(ab, image[0].cuda(), image[1].cuda(), H, K, act=act)
        else:
            padded = ops.expert_gemm_w4(ab, image[0].cuda(), image[1].cuda(), b.cuda() if has_bias else None, N, K, act=act)
        padded = torch.cat([padded.cpu()[e, :int(off[e + 1] - off[e])] for e in range(len(rows))], 0)
        _same(out[:used], padded, what + ": packed rows against the padded kernel")
        if act in ("none", "relu"):   # (the transcendental activations have no exact reference)
            acc, expert = _acc64(name, channels, amax, gather)
            f = (lambda v: v.clamp_min(0)) if act == "relu" else (lambda v: v)
            if H:   # the contract step by step: g = round(act(gacc)), D = round(float(g) * uacc)
                want = (f(acc[:, :H].float()).to(dtype).float() * acc[:, H:].float()).to(dtype)
            else:
                want = f(acc + bias[expert].double() if has_bias else acc)
                assert torch.equal(want.float().double(), want), "exact in fp32"
                want = want.float().to(dtype)
            _same(out[:used], want, what + ": packed rows against float64 rounded once")


def test_refusals_leave_d_untouched():
    """refused shapes: None comes back and D keeps its sentinel (nothing was enqueued)"""
    from tutel_amd import ops
    from tutel_amd.experts import w4
    lay = _layout("every_group_count")[0]
    E, dev = lay.E, torch.device("cuda")
    for dt, N, K, cut in ((torch.bfloat16, 48, 64, 0), (torch.bfloat16, 96, 96, 0), (torch.float32, 96, 64, 0), (torch.bfloat16, 96, 64, 4)):
        Ni, Ki = (N + 31) // 32 * 32, (K + 63) // 64 * 64   # an image of the next covered shape: the call's own N, K and strides refuse
        ci, si = w4.pack(torch.zeros([E, Ni, Ki // 2], dtype=torch.uint8), torch.full([E, Ni, Ki // 32], 127, dtype=torch.uint8))
        si = si.view(E, -1)[:, :si[0].numel() - cut].contiguous()   # cut: an expert's scale image is that many bytes short
        out = moated(torch.full([lay.rows_bound, N], OUT_FILL, dtype=dt), fill=OUT_FILL, device=dev)
        got = ops.expert_gemm_w4_packed(torch.ones([lay.rows_bound, K], dtype=dt, device=dev), ci.to(dev), si.to(dev), None, N, K, lay, out=out)
        torch.cuda.synchronize()
        moat_intact(out, "D")
        assert got is None and bool((out == OUT_FILL).all()), (dt, N, K, cut)
