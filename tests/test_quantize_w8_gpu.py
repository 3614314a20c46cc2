"""The HIP quantiser (csrc/quantize_w8.hip, ops.quantize_w8) against the torch quantiser ON THE CPU, bit for bit: image bytes and
scales `torch.equal` to w8.prepare(w.cpu(), kmajor) / w8.prepare_gate_up(...).  Both source layouts and all three dtypes, strided
sources and outputs inside poisoned guard bands, the gate / up channel map one launch at a time, every 16-bit value up to 448 (every
rounding tie and every e4m3 subnormal) under a unit scale and under scales that are no powers of two, all-zero and denormal
channels, quotients that round past 448 into the clamp, and non-finite weights."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))
POISON, SENTINEL = 0xA5, 12345.0


def _same(got, want, what=""):
    image, scale = got
    ref_image, ref_scale = want
    assert image.dtype == torch.uint8 and scale.dtype == torch.float32 and image.shape == ref_image.shape and scale.shape == ref_scale.shape, what
    assert torch.equal(scale.cpu().view(torch.int32), ref_scale.view(torch.int32)), what + ": scales"
    ne = (image.cpu() != ref_image).nonzero()
    assert ne.numel() == 0, f"{what}: {ne.shape[0]} of {ref_image.numel()} image bytes differ, the first at {tuple(int(v) for v in ne[0])}"


def _weights(E, N, K, dtype, seed):
    """[E, N, K] with channel magnitudes spread over many binades, one all-zero channel and one tiny one"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn([E, N, K], generator=g) * torch.exp2(torch.randint(-12, 6, [E, N, 1], generator=g).float())
    w[0, 1] = 0
    w[E - 1, N - 1] *= 1e-4
    return w.to(dtype)


def _stored(w_nk, kmajor):
    """the parameter as stored on the device: [E, N, K] or [E, K, N] contiguous"""
    return (w_nk if kmajor else w_nk.transpose(1, 2)).contiguous().cuda()


# ---- basic shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_basic_shapes_equal_the_cpu_quantiser(dtype, kmajor):
    """E = 3, N = 64, K = 96: three k-groups (a partial 128-k tile), two channel groups, more than one expert"""
    from tutel_amd import ops
    from tutel_amd.experts import w8
    w = _stored(_weights(3, 64, 96, dtype, 5), kmajor)
    want = w8.prepare(w.cpu(), kmajor)
    _same(ops.quantize_w8(w, kmajor), want, "ops.quantize_w8")
    _same(w8.prepare_native(w, kmajor), want, "w8.prepare_native")
    assert want[0].shape == (3, 2, 3, 64, 16) and float(want[1][0, 1]) == 1.0


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_more_than_one_tile_and_a_ragged_channel_block(dtype, kmajor):
    """K = 288 (two full 128-k tiles and a 32-k rest), N = 80 with the plain map into 96 image channels: the last workgroup of an
    expert holds 16 channels; the 16 image channels nobody maps to stay as they were"""
    from tutel_amd import ops
    from tutel_amd.experts import w8
    E, N, K, C = 2, 80, 288, 96
    w = _stored(_weights(E, N, K, dtype, 6), kmajor)
    image = torch.full([E, C // 32, K // 32, 64, 16], POISON, dtype=torch.uint8, device="cuda")
    scale = torch.full([E, C], SENTINEL, device="cuda")
    got = ops.quantize_w8(w, kmajor, image=image, scale=scale, channel_map=(C, N, N, 0))
    assert got[0] is image and got[1] is scale
    q, s = w8.quantize_e4m3(w.cpu(), kmajor)
    codes = w8.unpack(image.cpu(), C, K).view(torch.uint8)
    assert torch.equal(codes[:, :N], q.view(torch.uint8)) and bool((codes[:, N:] == POISON).all())
    assert torch.equal(scale.cpu()[:, :N], s) and bool((scale.cpu()[:, N:] == SENTINEL).all())


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_strided_source_in_nan_padding_and_outputs_in_guard_bands(dtype, kmajor):
    """ldw and w_stride_e larger than the data, every element that is not a weight a NaN: no ValueError means the status word stayed
    INT32_MAX, i.e. no padding was read as a weight.  Image and scales sit inside poisoned bands that come back intact"""
    from tutel_amd import ops
    from tutel_amd.experts import w8
    E, N, K = 3, 64, 96
    w_nk = _weights(E, N, K, dtype, 7)
    src = w_nk if kmajor else w_nk.transpose(1, 2).contiguous()     # [E, rows, cols]
    rows, cols = src.shape[1:]
    ldw, stride_e = cols + 8, rows * (cols + 8) + 16                # rows and experts stay 16-byte aligned in every dtype
    store = torch.full([E * stride_e + 64], float("nan"), dtype=dtype)
    view = store.as_strided([E, rows, cols], [stride_e, ldw, 1], 0)
    view.copy_(src)
    dev = store.cuda()
    w = dev.as_strided([E, rows, cols], [stride_e, ldw, 1], 0)
    assert bool(torch.isnan(dev).any()) and bool(torch.isfinite(w).all()) and not w.is_contiguous()
    G = 256
    ibuf = torch.full([G + E * N * K + G], POISON, dtype=torch.uint8, device="cuda")
    sbuf = torch.full([G + E * N + G], SENTINEL, device="cuda")
    image = ibuf[G:G + E * N * K].view(E, N // 32, K // 32, 64, 16)
    scale = sbuf[G:G + E * N].view(E, N)
    got = ops.quantize_w8(w, kmajor, image=image, scale=scale)
    assert got is not None, "the strided call is covered"
    _same(got, w8.prepare(src, kmajor), "strided")
    for band in (ibuf[:G], ibuf[-G:]):
        assert bool((band == POISON).all()), "the image's guard band was written"
    for band in (sbuf[:G], sbuf[-G:]):
        assert bool((band == SENTINEL).all()), "the scales' guard band was written"


# ---- the gate / up map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], **_ids)
@pytest.mark.parametrize("H", [48, 64])
def test_glu_map_one_launch_at_a_time(H, dtype):
    """n-major [E, K, H] parameters, K = 64.  After the gate launch alone the up half of a pre-poisoned image (and of the scales) is
    untouched; after both the image is prepare_gate_up's"""
    from tutel_amd import ops
    from tutel_amd.experts import w8
    E, K = 2, 64
    gate = _stored(_weights(E, H, K, dtype, 8), False)
    up = _stored(_weights(E, H, K, dtype, 9), False)
    want = w8.prepare_gate_up(gate.cpu(), up.cpu(), False)
    image = torch.full([E, 2 * H // 32, K // 32, 64, 16], POISON, dtype=torch.uint8, device="cuda")
    scale = torch.full([E, 2 * H], SENTINEL, device="cuda")
    assert ops.quantize_w8(gate, False, image=image, scale=scale, channel_map=w8.glu_channel_map(H, False)) is not None
    half_g, half_u = w8.deinterleave_gate_up(w8.unpack(image.cpu(), 2 * H, K))
    want_g, want_u = w8.deinterleave_gate_up(w8.unpack(want[0], 2 * H, K))
    assert torch.equal(half_g.view(torch.uint8), want_g.view(torch.uint8)), "the gate's codes"
    assert bool((half_u.view(torch.uint8) == POISON).all()), "the gate launch wrote into the up half"
    sg, su = w8.deinterleave_gate_up(scale.cpu())
    assert torch.equal(sg, w8.deinterleave_gate_up(want[1])[0]) and bool((su == SENTINEL).all())
    assert ops.quantize_w8(up, False, image=image, scale=scale, channel_map=w8.glu_channel_map(H, True)) is not None
    _same((image, scale), want, "gate + up")
    _same(w8.prepare_gate_up_native(gate, up, False), want, "w8.prepare_gate_up_native")


# ---- every value ---------------------------------------------------------------------------------------------------------------------
def _every_value(dtype):
    """every finite value of `dtype` with |v| <= 448, both signs (and both zeros), as fp32"""
    v = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(dtype).float()
    return v[torch.isfinite(v) & (v.abs() <= 448)]


def _channels_with_amax(values, amax, K=64):
    """[1, N, K] fp32: the values spread over channels of K - 1, each channel's last element `amax` itself; N padded up to a multiple
    of 32 with channels of zeros (and their amax)"""
    per = K - 1
    n = (values.numel() + per - 1) // per
    N = (n + 31) // 32 * 32
    body = torch.zeros([N * per])
    body[:values.numel()] = values
    w = torch.cat([body.view(N, per), torch.full([N, 1], float(amax))], dim=1)
    return w.view(1, N, K)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], **_ids)
@pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_every_value_up_to_448(dtype, kmajor):
    """under amax = 448 the scale is exactly 1 and the code is the value's own rounding: every tie, every subnormal code.  Scaled into
    channels of amax 3.0 and 0.1 the scales are no powers of two and the quotients carry the division's rounding"""
    from tutel_amd import ops
    from tutel_amd.experts import w8
    vals = _every_value(dtype)
    assert vals.numel() > 30000 and float(vals.abs().max()) == 448.0
    unit = _channels_with_amax(vals, 448.0).to(dtype)
    assert torch.equal(unit.float().view(-1)[:5], _channels_with_amax(vals, 448.0).view(-1)[:5])
    src = _stored(unit, kmajor)
    want = w8.prepare(src.cpu(), kmajor)
    assert bool((want[1] == 1.0).all()), "amax 448: the scale is exactly 1"
    assert len(set(want[0].view(-1).tolist())) >= 254, "every finite code appears"
    _same(ops.quantize_w8(src, kmajor), want, "unit scale")
    for amax in (3.0, 0.1):
        top = float(torch.tensor(amax).to(dtype))
        for dt in (dtype, torch.float32):   # rounded to the dtype, and exact in fp32
            scaled = _channels_with_amax(vals * (top / 448.0), top).to(dt)
            src = _stored(scaled, kmajor)
            want = w8.prepare(src.cpu(), kmajor)
            s = float(want[1][0, 0])
            assert s != 1.0 and s != 2.0 ** round(torch.log2(torch.tensor(s)).item()), "not a power of two"
            _same(ops.quantize_w8(src, kmajor), want, f"amax {amax} in {dt}")


# ---- edge channels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_zero_channels_keep_the_sign_and_denormal_channels_are_not_flushed(kmajor):
    from tutel_amd import ops
    from tutel_amd.experts import w8
    g = torch.Generator().manual_seed(11)
    E, N, K = 1, 32, 64
    # bf16: channel 0 all zero with -0 entries; channels 1..7 hold bf16 SUBNORMALS only (bit patterns 1..0x7f, both signs): the amax and
    # with it the scale are fp32 denormals; the rest ordinary
    bits = torch.randint(1, 0x80, [8, K], generator=g, dtype=torch.int32) | (torch.randint(0, 2, [8, K], generator=g, dtype=torch.int32) << 15)
    w = (torch.randn([E, N, K], generator=g)).bfloat16()
    w[0, :8] = bits.to(torch.int16).view(torch.bfloat16)
    w[0, 0] = 0.0
    w[0, 0, ::3] = -0.0
    src = _stored(w, kmajor)
    want = w8.prepare(src.cpu(), kmajor)
    q = w8.unpack(want[0], N, K).view(torch.uint8)
    assert float(want[1][0, 0]) == 1.0 and set(q[0, 0].tolist()) == {0x00, 0x80}, "-0 keeps its sign in the reference"
    assert bool((want[1][0, 1:8] < 2.0 ** -126).all()) and bool((want[1][0, 1:8] > 0).all()), "denormal scales in the reference"
    assert int((q[0, 1:8] & 0x7F).max()) == 0x7E, "the denormal channels use the whole code range"
    _same(ops.quantize_w8(src, kmajor), want, "bf16 edge channels")
    # fp32: denormal weights, amax around 1e-40
    wf = torch.randn([E, N, K], generator=g)
    wf[0, :8] *= 1e-40
    wf[0, 8] = 0.0
    wf[0, 8, 1::2] = -0.0
    src = _stored(wf, kmajor)
    want = w8.prepare(src.cpu(), kmajor)
    assert bool((want[1][0, :8] < 1e-41).all()) and bool((want[1][0, :8] > 0).all())
    _same(ops.quantize_w8(src, kmajor), want, "fp32 denormal channels")


# ---- rounding past the clamp ---------------------------------------------------------------------------------------------------------
CLAMP_SEED = 2024


def _clamp_sweep():
    """4096 fp32 channels of K = 32, amax drawn over 60 binades; every channel holds +amax and -amax"""
    g = torch.Generator().manual_seed(CLAMP_SEED)
    N, K = 4096, 32
    amax = (1.0 + torch.rand([N], generator=g)) * torch.exp2(torch.randint(-30, 30, [N], generator=g).float())
    w = (torch.rand([1, N, K], generator=g) * 2 - 1) * amax.view(1, N, 1)
    w[0, :, 0], w[0, :, 1] = amax, -amax
    return w


@pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_quotients_that_round_above_448_are_clamped(kmajor):
    from tutel_amd import ops
    from tutel_amd.experts import w8
    w = _clamp_sweep()
    amax = w.abs().amax(dim=2)
    scale = amax / torch.full_like(amax, 448.0)
    over = (amax / scale) > 448.0
    assert int(over.sum()) >= 1, "the sweep holds a channel whose own amax / scale rounds above 448: the clamp acts in the reference"
    assert float(torch.log2(amax.max() / amax.min())) > 55, "amax over 60 binades"
    src = _stored(w, kmajor)
    want = w8.prepare(src.cpu(), kmajor)
    q = w8.unpack(want[0], 4096, 32).view(torch.uint8)
    assert bool((q[0, :, 0] == 0x7E).all()) and bool((q[0, :, 1] == 0xFE).all())
    _same(ops.quantize_w8(src, kmajor), want, "clamp sweep")


# ---- non-finite weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_non_finite_weights_raise_the_torch_quantisers_error(dtype, kmajor):
    from tutel_amd import ops
    from tutel_amd.experts import w8
    for first, second in ((float("inf"), float("nan")), (float("nan"), -float("inf"))):
        w = _weights(3, 64, 96, dtype, 13)
        w[1, 40, 17] = first      # the lower channel: lowest expert first, then lowest output
        w[1, 57, 3] = second
        w[2, 5, 90] = second
        src = _stored(w, kmajor)
        with pytest.raises(ValueError) as ref:
            w8.prepare(src.cpu(), kmajor)
        assert "(expert 1, output 40)" in str(ref.value)
        with pytest.raises(ValueError) as got:
            ops.quantize_w8(src, kmajor)
        assert str(got.value) == str(ref.value)
        with pytest.raises(ValueError) as got:
            ops.quantize_w8(src, kmajor, check_only=True)
        assert str(got.value) == str(ref.value)
    clean = _stored(_weights(3, 64, 96, dtype, 13), kmajor)
    assert ops.quantize_w8(clean, kmajor, check_only=True) == (None, None)
