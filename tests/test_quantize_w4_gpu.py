"""The HIP MXFP4 quantiser (ops.quantize_w4) against w4.prepare / w4.prepare_gate_up ON THE CPU, bit for bit.  The kernel's K chunk is
256 (four 64-k code tiles, two 128-k scale dwords per workgroup): K = 64 is a quarter chunk with three pad scale bytes, K = 192 a
ragged scale dword, K = 256 a full chunk and K = 384 two workgroups along K, the second half full."""
import functools

import pytest
import torch

from tutel_amd import ops
from tutel_amd.experts import w4, w8

pytestmark = pytest.mark.gpu
ACT = [torch.bfloat16, torch.float16]
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))
src = pytest.mark.parametrize("dtype", ACT + [torch.float32], **_ids)
act = pytest.mark.parametrize("act", ACT, **_ids)
layout = pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
POISON = 0xA5


def _same(got, want, what=""):
    for g, w, part in zip(got, want, ("codes", "scales")):
        assert g.dtype == torch.uint8 and g.shape == w.shape, f"{what}: {part} {tuple(g.shape)} {g.dtype}"
        ne = (g.cpu() != w).nonzero()
        assert ne.numel() == 0, f"{what}: {ne.shape[0]} of {w.numel()} {part} bytes differ, the first at {tuple(int(v) for v in ne[0])}"


def _weights(E, N, K, dtype, seed, kmajor=True):
    """the parameter as stored: block magnitudes over many binades, an all-zero block, a tiny channel"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn([E, N, K // 32, 32], generator=g) * torch.exp2(torch.randint(-20, 12, [E, N, K // 32, 1], generator=g).float())
    w[0, 1, 0] = 0
    w[E - 1, N - 1] *= 1e-6
    w = w.view(E, N, K).to(dtype)
    return w if kmajor else w.transpose(1, 2).contiguous()


@act
@src
@layout
def test_smallest_shapes_that_reach_every_index_path(kmajor, dtype, act):
    for N in (32, 96):
        for K in (64, 192, 256, 384):
            w = _weights(2, N, K, dtype, N + K, kmajor)
            _same(ops.quantize_w4(w.cuda(), kmajor, act), w4.prepare(w, kmajor, act), f"N={N} K={K}")


@src
@layout
def test_strided_source_in_nan_padding_and_outputs_in_guard_bands(kmajor, dtype):
    """every element that is not a weight is a NaN: no ValueError means no padding was read; the images sit inside poisoned bands"""
    E, band = 3, 4096
    src = _weights(E, 64, 192, dtype, 7, kmajor)
    rows, cols = src.shape[1:]
    ldw, stride_e = cols + 8, rows * (cols + 8) + 16
    store = torch.full([E * stride_e + 64], float("nan"), dtype=dtype)
    store.as_strided([E, rows, cols], [stride_e, ldw, 1], 0).copy_(src)
    w = store.cuda().as_strided([E, rows, cols], [stride_e, ldw, 1], 0)
    want = w4.prepare(src, kmajor, torch.bfloat16)
    bufs = [torch.full([t.numel() + 2 * band], POISON, dtype=torch.uint8, device="cuda") for t in want]
    codes, scales = (b[band:-band].view(t.shape) for b, t in zip(bufs, want))
    got = ops.quantize_w4(w, kmajor, torch.bfloat16, codes=codes, scales=scales)
    assert got[0] is codes and got[1] is scales
    _same(got, want, "strided")
    assert all(bool((b[:band] == POISON).all()) and bool((b[-band:] == POISON).all()) for b in bufs), "a guard band was written"


@functools.lru_cache(maxsize=None)
def _every_finite(dtype, permuted):
    """[1, 32, 2048]: every pattern of the dtype, the non-finite ones replaced by 0; permuted: small values sit under a large amax"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    v = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    if permuted:
        v = v[torch.randperm(65536, generator=torch.Generator().manual_seed(11))]
    return v.view(1, 32, 2048)


@act
@pytest.mark.parametrize("permuted", [False, True], ids=["natural", "permuted"])
@pytest.mark.parametrize("dtype", ACT, **_ids)
def test_every_finite_16_bit_pattern(dtype, permuted, act):
    w = _every_finite(dtype, permuted)
    want = w4.prepare(w, True, act)
    _same(ops.quantize_w4(w.cuda(), True, act), want, "k-major")
    _same(ops.quantize_w4(w.transpose(1, 2).contiguous().cuda(), False, act), want, "n-major")
    assert not permuted or bool(((w < 0) & (w4.unpack_nibbles(w4.unpack(*want, 32, 2048)[0]) == 0)).any()), "negative values round to 0"


def _crafted():
    """[1, 32, 512] fp32, one case per block of 32; every row also runs negated in the next channel"""
    grid = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 7.0] * 2)
    tiny, huge = 2.0 ** -140, 2.0 ** 126
    blocks = [grid * 2.0 ** e for e in (-126, -100, -14, -13, 0, 13, 14, 100, 120)]     # the midpoints under s = 127 + e (where admitted)
    blocks += [torch.tensor(b * 8) for b in (
        [0.0, -0.0, 0.0, -0.0],
        [tiny, -tiny, tiny / 4, tiny * 0.75],                                   # amax an fp32 subnormal: below every range
        [2.0 ** -149, -(2.0 ** -127), 2.0 ** -128 * 1.5, 2.0 ** -127 * 1.25],
        [2.0 ** -20, 2.0 ** -22, -(2.0 ** -21), 0.75 * 2.0 ** -20],             # below fp16's range: rounding to 0 under s = 114
        [huge, -huge, huge / 3, 1.0],                                           # above both ranges: saturation at +-6
        [60000.0, -65504.0, 30000.0, 40960.0],                                  # above fp16's range only
        [3.0e38, -3.4e38, 1.0e38, 1.0])]
    row = torch.cat(blocks)
    w = torch.zeros(1, 32, row.numel())
    w[0, 0::2], w[0, 1::2] = row, -row
    return w


@act
@layout
def test_crafted_blocks(kmajor, act):
    w = _crafted() if kmajor else _crafted().transpose(1, 2).contiguous()
    want = w4.prepare(w, kmajor, act)
    _same(ops.quantize_w4(w.cuda(), kmajor, act), want, "crafted")
    codes, scales = w4.unpack(*want, 32, 512)
    assert (int(scales.min()), int(scales.max())) == w4.SCALE_RANGE[act] and bool((w4.unpack_nibbles(codes) == 0xf).any())


@pytest.mark.parametrize("dtype", ACT, **_ids)
@pytest.mark.parametrize("H", [48, 64])
def test_swiglu_map_two_calls_into_one_image(H, dtype):
    gate, up = (_weights(2, H, 192, dtype, s, False) for s in (3, 4))
    want = w4.prepare_gate_up(gate, up, False, dtype)
    got = tuple(torch.full(t.shape, POISON, dtype=torch.uint8, device="cuda") for t in want)
    for w, is_up in ((gate, False), (up, True)):
        assert ops.quantize_w4(w.cuda(), False, dtype, *got, channel_map=w8.glu_channel_map(H, is_up)) is not None
    _same(got, want, "gate / up")


@layout
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_input_raises_the_torch_quantisers_error(bad, kmajor):
    w = _weights(2, 64, 384, torch.bfloat16, 9)
    w[1, 37, 300] = bad
    w = w if kmajor else w.transpose(1, 2).contiguous()
    with pytest.raises(ValueError, match=r"\(expert 1, output 37\)") as ref:
        w4.prepare(w, kmajor)
    got = tuple(torch.full(s, POISON, dtype=torch.uint8, device="cuda") for s in ([2, 2, 6, 64, 16], [2, 2, 3, 32, 4]))
    for check_only in (True, False):
        with pytest.raises(ValueError) as err:
            ops.quantize_w4(w.cuda(), kmajor, None, *got, check_only=check_only)
        assert str(err.value) == str(ref.value)
        assert not check_only or all(bool((t == POISON).all()) for t in got), "check_only writes nothing"


@pytest.mark.parametrize("dtype", ACT, **_ids)
def test_gemm_round_trip(dtype):
    E, R, N, K = 2, 40, 96, 192
    w = _weights(E, N, K, torch.float32, 13).clamp(-4, 4).to(dtype)
    a = (torch.randn([E, R, K], generator=torch.Generator().manual_seed(14)) * 0.25).to(dtype).cuda()
    want = ops.expert_gemm_w4(a, *(t.cuda() for t in w4.prepare(w, True)), None, N, K)
    got = ops.expert_gemm_w4(a, *ops.quantize_w4(w.cuda(), True), None, N, K)
    assert float(want.abs().max()) > 0 and torch.equal(got.view(torch.int16), want.view(torch.int16))
