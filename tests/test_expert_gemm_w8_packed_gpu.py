"""The W8A16 grouped GEMMs over the packed dropless layout (tutel_amd_expert_gemm_w8_packed / _glu_packed) on the MI355X.

The contract (include/tutel_amd.h): a packed row's output is BIT-IDENTICAL to what tutel_amd_expert_gemm_w8 / _glu writes for the same
input row and expert, wherever the row lies.  Checked twice, with no tolerance either time:
  * against the padded kernel on the bucket form of the same rows (pad rows are the zero row);
  * independently of both kernels, on operands whose arithmetic is exact in fp32 (small integers, power-of-two scales, a dyadic bias:
    the restated inputs of tests/test_expert_gemm_w8_gpu.py::_exact_inputs and of the GLU file) -- the result is then the float64
    value rounded once, whatever the order of the sum.
Every device operand, the layout's tables included, lies in guard bands; D holds a sentinel: rows at and past offsets[E] keep it."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _packed_fuzz import gathered, layout_from_rows, moat_intact, moated  # noqa: E402

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
OUT_FILL = 1234.0
# (rows per expert, alignment, N, K)
CASES = {
    "halves_tiles_clamped_wave": ([0, 1, 127, 128, 129, 0, 256, 257, 300, 5], 1, 96, 64),   # empty experts, both halves, a second table
                                                                                            # tile, a clamped wave (N = 96), one K-tile
    "pad_rows_odd_ktiles": ([3, 0, 130, 0], 4, 160, 320),   # -1 pad rows inside ranges, an empty last expert, 5 K-tiles (ring depth 4)
    "one_expert_holds_all": ([0, 600, 0], 1, 256, 128),
    "nothing_live": ([0, 0, 0, 0], 1, 32, 64),               # D keeps its sentinel everywhere
}
# (gathered (fc1) form, bias, activation): both forms, bias on and off, the four activations -- the cross product thinned
COMBOS = [(True, True, "relu"), (False, False, "none"), (True, False, "none"), (False, True, "relu"), (True, True, "gelu"),
          (False, True, "silu"), (True, False, "silu"), (False, False, "gelu")]
GLU_H = [48, 128]
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))


def _mods():
    from tutel_amd import ops
    from tutel_amd.experts import w8
    return ops, w8


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ne = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert ne.numel() == 0, (f"{what}: {ne.shape[0]} of {got.numel()} elements differ; the first at {tuple(int(v) for v in ne[0])}: "
                             f"{float(got[tuple(ne[0])])!r} against {float(want[tuple(ne[0])])!r}")


# ---- the layout, its tables inside guard bands ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout(name):
    """(layout whose five tables are moated copies of the library's, offsets on the host, slot map on the host, T)"""
    rows, align = CASES[name][:2]
    lay, idx, _ = layout_from_rows(rows, align)
    torch.cuda.synchronize()
    off, slot = lay.offsets.cpu(), lay.slot_map.cpu()
    want = [0]
    for r in rows:
        want.append(want[-1] + (r + align - 1) // align * align)
    assert off.tolist() == want, "the layout is the one the rows describe"
    live = int(lay.ntiles.cpu())
    tiles = lay.tiles.cpu()[:2 * live].view(-1, 2).tolist()
    assert tiles == [[e, want[e] + j] for e in range(len(rows)) for j in range(0, want[e + 1] - want[e], 256)], "the tile table"
    # an in-range index around every table: a kernel that reads past one must not get a wild address out of it
    for name_ in ("offsets", "tiles", "ntiles", "capacity", "slot_map"):
        setattr(lay, name_, moated(getattr(lay, name_).cpu(), fill=0, device=torch.device("cuda")))
    return lay, off, slot, idx.shape[1]


def _tables_intact(lay):
    for name_ in ("offsets", "tiles", "ntiles", "capacity", "slot_map"):
        moat_intact(getattr(lay, name_), "the table " + name_)


def _bucket(rows_2d, off, C):
    """[used, K] packed rows -> the bucket form [E, C, K] (rows an expert does not own: zeros)"""
    E = off.numel() - 1
    out = torch.zeros([E, C, rows_2d.shape[1]], dtype=rows_2d.dtype)
    for e in range(E):
        n = int(off[e + 1] - off[e])
        out[e, :n] = rows_2d[int(off[e]):int(off[e + 1])]
    return out


def _unbucket(b, off):
    return torch.cat([b[e, :int(off[e + 1] - off[e])] for e in range(off.numel() - 1)], 0)


# ---- exact operands (tests/test_expert_gemm_w8_gpu.py::_exact_inputs, restated for packed rows) -----------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_inputs(name):
    """A and the tokens in {-3 .. 3}, q the e4m3 integers {-4 .. 4}, scales 2^-3 .. 2^3, bias from a dyadic set: every product, every
    partial sum in any order (|sum| <= 12 K < 2^24) and the scaled, biased result (a multiple of 2^-3 below 2^18) are exact in fp32.
    Rows of A at and past offsets[E] are NaN: they are never read"""
    rows, align, N, K = CASES[name]
    lay, off, slot, T = _layout(name)
    E, used = len(rows), int(off[-1])
    g = torch.Generator().manual_seed(8191 * E + 3 * N + K + used)
    a = torch.randint(-3, 4, [lay.rows_bound, K], generator=g).float()
    a[used:] = float("nan")
    x = torch.randint(-3, 4, [T, K], generator=g).float()
    q = torch.randint(-4, 5, [E, N, K], generator=g).float().to(F8)
    scale = torch.pow(2.0, torch.randint(-3, 4, [E, N], generator=g).float())
    bias = torch.tensor([-2.0, -0.5, -0.25, 0.0, 0.25, 1.0, 3.0])[torch.randint(0, 7, [E, N], generator=g)]
    return a, x, q, scale, bias


@functools.lru_cache(maxsize=None)
def _exact_pre(name, gather):
    """float64 acc * scale of the live packed rows [used, N], computed once, never modified (the bias is added by the caller)"""
    a, x, q, scale, _ = _exact_inputs(name)
    _, off, slot, _ = _layout(name)
    used = int(off[-1])
    src = (gathered(x, slot[:used]) if gather else a[:used]).double()
    out = torch.empty([used, q.shape[1]], dtype=torch.float64)
    for e in range(off.numel() - 1):
        lo, hi = int(off[e]), int(off[e + 1])
        out[lo:hi] = src[lo:hi] @ q[e].double().t() * scale[e].double()
    return out


def _act64(v, act):
    return v.clamp_min(0) if act == "relu" else v


def _run_packed(name, a, q, scale, bias, act, gather):
    ops, w8 = _mods()
    lay = _layout(name)[0]
    dev = torch.device("cuda")
    E, N, K = q.shape
    ad = moated(a, device=dev)
    img = moated(w8.pack(q), fill=0x7F, device=dev)   # the NaN code around the image
    sd = moated(scale, device=dev)
    bd = moated(bias, device=dev) if bias is not None else None
    zr = moated(torch.zeros([K], dtype=a.dtype), device=dev) if gather else None
    out = moated(torch.full([lay.rows_bound, N], OUT_FILL, dtype=a.dtype), fill=OUT_FILL, device=dev)
    got = ops.expert_gemm_w8_packed(ad, img, sd, bd, N, K, lay, act=act, gather=gather, zero_row=zr, out=out)
    assert got is out
    torch.cuda.synchronize()
    for t, what in ((ad, "A"), (img, "the image"), (sd, "scale"), (bd, "bias"), (zr, "the zero row"), (out, "D")):
        if t is not None:
            moat_intact(t, what)
    _tables_intact(lay)
    return out.cpu()


def _run_padded(a_bucket, q, scale, bias, act):
    ops, w8 = _mods()
    E, N, K = q.shape
    out = ops.expert_gemm_w8(a_bucket.cuda(), w8.pack(q).cuda(), scale.cuda(), bias.cuda() if bias is not None else None, N, K, act=act)
    assert out is not None
    return out.cpu()


def _sentinel_kept(out, used, dtype):
    fill = torch.full([1], OUT_FILL, dtype=dtype)
    assert bool((out[used:] == fill).all()), "a row at or past offsets[E] was written"


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("name", list(CASES))
def test_packed_rows_equal_the_padded_kernel_and_float64_rounded_once(name, dtype):
    rows, align, N, K = CASES[name]
    a, x, q, scale, bias = _exact_inputs(name)
    _, off, slot, _ = _layout(name)
    used = int(off[-1])
    C = int((off[1:] - off[:-1]).max())
    for gather, has_bias, act in COMBOS:
        what = f"{name} {'gathered' if gather else 'plain'} {'bias' if has_bias else 'nobias'} {act}"
        b = bias.to(dtype) if has_bias else None
        out = _run_packed(name, (x if gather else a).to(dtype), q, scale, b, act, gather)
        _sentinel_kept(out, used, dtype)
        if used == 0:
            continue
        # against the padded kernel on the bucket form of the same rows: the contract, no tolerance
        src = (gathered(x, slot[:used]) if gather else a[:used]).to(dtype)
        padded = _run_padded(_bucket(src, off, C), q, scale, b, act)
        _same(out[:used], _unbucket(padded, off), what + ": packed rows against the padded kernel")
        # independent of both kernels: float64 rounded once (the transcendental activations have no exact reference)
        if act in ("none", "relu"):
            v = _exact_pre(name, gather)
            if has_bias:
                v = v + torch.cat([bias[e].double().expand(int(off[e + 1] - off[e]), N) for e in range(len(rows))], 0)
            want = _act64(v, act)
            assert torch.equal(want.float().double(), want), "the reference is exact in fp32: one rounding to the dtype follows"
            _same(out[:used], want.float().to(dtype), what + ": packed rows against float64 rounded once")


# ---- the GLU form -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _glu_inputs(name, H):
    """A and the tokens in {-1, 0, 1}, the e4m3 integers {-2 .. 2}, scales 2^-3 .. 1 (tests/test_expert_gemm_w8_glu_gpu.py): every
    partial sum and both scaled values are exact in fp32"""
    rows, align, _, K = CASES[name]
    lay, off, slot, T = _layout(name)
    E, used = len(rows), int(off[-1])
    g = torch.Generator().manual_seed(131 * E + 7 * H + K + used)
    a = torch.randint(-1, 2, [lay.rows_bound, K], generator=g).float()
    a[used:] = float("nan")
    x = torch.randint(-1, 2, [T, K], generator=g).float()
    qg = torch.randint(-2, 3, [E, H, K], generator=g).float().to(F8)
    qu = torch.randint(-2, 3, [E, H, K], generator=g).float().to(F8)
    sg = torch.pow(2.0, torch.randint(-3, 1, [E, H], generator=g).float())
    su = torch.pow(2.0, torch.randint(-3, 1, [E, H], generator=g).float())
    return a, x, qg, qu, sg, su


def _glu_want(name, H, gather, act, dtype):
    """the contract step by step on the CPU: g = round(act(gacc * sg)), u = uacc * su, D = round(float(g) * u) -- [used, H]"""
    a, x, qg, qu, sg, su = _glu_inputs(name, H)
    _, off, slot, _ = _layout(name)
    used = int(off[-1])
    src = (gathered(x, slot[:used]) if gather else a[:used]).double()
    out = torch.empty([used, H], dtype=dtype)
    for e in range(off.numel() - 1):
        lo, hi = int(off[e]), int(off[e + 1])
        gacc, uacc = src[lo:hi] @ qg[e].double().t(), src[lo:hi] @ qu[e].double().t()
        gs, us = gacc.float() * sg[e], uacc.float() * su[e]
        assert torch.equal(gs.double(), gacc * sg[e].double()) and torch.equal(us.double(), uacc * su[e].double()), "exact in fp32"
        g = (gs.clamp_min(0) if act == "relu" else gs).to(dtype)
        out[lo:hi] = (g.float() * us).to(dtype)
    return out


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("H", GLU_H)
@pytest.mark.parametrize("name", list(CASES))
def test_glu_packed_rows_equal_the_padded_kernel_and_the_contract(name, H, dtype):
    ops, w8 = _mods()
    rows, align, _, K = CASES[name]
    a, x, qg, qu, sg, su = _glu_inputs(name, H)
    lay, off, slot, _ = _layout(name)
    used = int(off[-1])
    C = int((off[1:] - off[:-1]).max())
    dev = torch.device("cuda")
    image, scale = w8.pack(w8.interleave_gate_up(qg, qu)), w8.interleave_gate_up(sg, su).contiguous()
    for gather, act in ((True, "silu"), (False, "silu"), (True, "relu"), (False, "none"), (True, "gelu")):
        what = f"{name} H={H} {'gathered' if gather else 'plain'} {act}"
        ad = moated((x if gather else a).to(dtype), device=dev)
        img = moated(image, fill=0x7F, device=dev)
        sd = moated(scale, device=dev)
        zr = moated(torch.zeros([K], dtype=dtype), device=dev) if gather else None
        out = moated(torch.full([lay.rows_bound, H], OUT_FILL, dtype=dtype), fill=OUT_FILL, device=dev)
        got = ops.expert_gemm_w8_glu_packed(ad, img, sd, H, K, lay, act=act, gather=gather, zero_row=zr, out=out)
        assert got is out
        torch.cuda.synchronize()
        for t, w in ((ad, "A"), (img, "the image"), (sd, "scale"), (zr, "the zero row"), (out, "D")):
            if t is not None:
                moat_intact(t, w)
        _tables_intact(lay)
        out = out.cpu()
        _sentinel_kept(out, used, dtype)
        if used == 0:
            continue
        src = (gathered(x, slot[:used]) if gather else a[:used]).to(dtype)
        padded = ops.expert_gemm_w8_glu(_bucket(src, off, C).cuda(), image.cuda(), scale.cuda(), H, K, act=act)
        assert padded is not None
        _same(out[:used], _unbucket(padded.cpu(), off), what + ": packed rows against the padded kernel")
        if act in ("none", "relu"):
            _same(out[:used], _glu_want(name, H, gather, act, dtype), what + ": packed rows against the contract step by step")


def test_a_second_run_gives_the_same_bits_and_refusals_leave_d_untouched():
    ops, w8 = _mods()
    name = "halves_tiles_clamped_wave"
    rows, align, N, K = CASES[name]
    a, x, q, scale, bias = _exact_inputs(name)
    dtype = torch.bfloat16
    one = _run_packed(name, x.to(dtype), q, scale, bias.to(dtype), "relu", True)
    two = _run_packed(name, x.to(dtype), q, scale, bias.to(dtype), "relu", True)
    _same(one, two, "a second run")
    # refused shapes: None comes back and D keeps its sentinel (nothing was enqueued)
    lay = _layout(name)[0]
    dev = torch.device("cuda")
    for dt, N_, K_ in ((torch.bfloat16, 48, 64), (torch.bfloat16, 96, 96), (torch.float32, 96, 64)):
        ad = torch.ones([lay.rows_bound, K_], dtype=dt, device=dev)
        img = w8.pack(torch.zeros([len(rows), N_, K_]).to(F8)).to(dev)
        out = moated(torch.full([lay.rows_bound, N_], OUT_FILL, dtype=dt), fill=OUT_FILL, device=dev)
        got = ops.expert_gemm_w8_packed(ad, img, torch.ones([len(rows), N_], device=dev), None, N_, K_, lay, out=out)
        torch.cuda.synchronize()
        moat_intact(out, "D")
        assert got is None and bool((out == OUT_FILL).all()), (dt, N_, K_)
