"""MXFP4-resident experts in the layer (experts.fp4_freeze()), `ffn` and SwiGLU, bf16 and fp16 at M = H = 128, E = 4, 64 tokens: same
bits as the fp4_weights forwards before the freeze, exact memory, MXFP4 state dicts both ways, refusals with their reason."""
import gc
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL                                     # noqa: E402
from test_swiglu_packed_gpu import make_layer as make_swiglu    # noqa: E402

pytestmark = pytest.mark.gpu

T, E, K, M, H = 64, 4, 2, 128, 128
FP4_KEYS = {"ffn": ["fc1_w4", "fc1_w4_scale", "fc2_w4", "fc2_w4_scale"], "llama_ffn": ["fc12_w4", "fc12_w4_scale", "fc3_w4", "fc3_w4_scale"]}
W16_KEYS = {"ffn": ["batched_fc1_w", "batched_fc2_w"], "llama_ffn": ["W_fc1", "W_fc2", "W_fc3"]}
BIASES = {"ffn": ["batched_fc1_bias", "batched_fc2_bias"], "llama_ffn": []}
IMAGES = {"ffn": [(H, M), (M, H)], "llama_ffn": [(2 * H, M), (M, H)]}      # (channels, K) of the images, in FP4_KEYS' order
both = pytest.mark.parametrize("kind, dtype", [(k, d) for k in FP4_KEYS for d in (torch.bfloat16, torch.float16)],
                               ids=lambda v: str(v).replace("torch.", ""))


@pytest.fixture(autouse=True)
def leave_no_garbage():
    yield
    gc.collect()


def _layer(oracle, kind, dtype, seed=21, hidden=H, fp4=True):
    x, wg, w1, b1, w2, b2 = oracle.make_problem(T, M, hidden, E, dtype=dtype, seed=seed)
    if kind == "ffn":
        layer = TL.make_layer(M, hidden, E, K, 1.0, dtype, (wg, w1, b1, w2, b2), gate={"fp32_gate": True}).eval()
    else:
        g = torch.Generator().manual_seed(77 + seed)
        weights = [wg] + [(torch.randn(s, generator=g) / s[1] ** 0.5).to(dtype) for s in ([E, M, hidden], [E, M, hidden], [E, hidden, M])]
        layer = make_swiglu(M, hidden, E, K, 1.0, dtype, "top", weights=tuple(weights), gate={"fp32_gate": True}).eval()
        x = x * 0.5
    for p in layer.parameters():
        p.requires_grad_(False)
    layer.experts.fp4_weights = fp4
    return layer, x.cuda()


def _run(layer, x, cf):   # cf: the gate's capacity_factor for this call (0: dropless)
    layer.gates[0].capacity_factor = cf
    with torch.no_grad():
        y = layer(x)
    assert layer._fp4_weights_ran is True, layer._fp4_weights_ran
    return y.detach().clone()


def _same(a, b, what):
    assert a.dtype == b.dtype and torch.equal(a.view(torch.int16), b.view(torch.int16)), what


@both
def test_same_bits_after_the_freeze_and_memory_peaks_at_the_images(oracle, kind, dtype):
    """The peak bound: memory before the freeze + every image + ONE 512-byte allocator block, the status word of the quantiser call in
    flight.  The parameters are contiguous and 16-byte aligned, so _quantise clones nothing; every image is a multiple of 512 bytes"""
    from tutel_amd.impls.graph import GraphedForward
    layer, x = _layer(oracle, kind, dtype)
    ex = layer.experts
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dtype).cuda() * 0.5
    before = {cf: _run(layer, x, cf) for cf in (1.0, 0.0)}
    before_other = _run(layer, other, 1.0)
    assert float(before[1.0].abs().max()) > 0 and bool(torch.isfinite(before[0.0].float()).all())
    ex.invalidate_prepacked()                                   # (the derived images: the freeze is measured against the parameters alone)
    released = sum(getattr(ex, n).numel() * 2 for n in W16_KEYS[kind])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    assert ex.fp4_freeze() is ex and ex.fp4_frozen is True and ex.fp4_weights is True and ex.fp8_frozen is False
    torch.cuda.synchronize()
    after, peak = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
    sizes = [getattr(ex, k).numel() for k in FP4_KEYS[kind]]
    assert sizes == [n for C, Kd in IMAGES[kind] for n in (E * C * Kd // 2, E * C * ((Kd + 127) // 128) * 4)], sizes
    print(f"\n{kind} {dtype}: released {released} B, images {sum(sizes)} B, allocated {base} -> {after} B, peak {peak} B")
    assert base - after == released - sum(sizes) and peak <= base + sum(sizes) + 512, (base, after, peak, released, sizes)
    assert [n for n, _ in ex.named_parameters()] == BIASES[kind]
    for t in (getattr(ex, n) for n in W16_KEYS[kind]):
        assert t.device.type == "meta" and t.dtype == dtype and not isinstance(t, torch.nn.Parameter)
    assert [id(b) for pair in ex.w4_params() for b in pair] == [id(getattr(ex, k)) for k in FP4_KEYS[kind]]
    for cf in (1.0, 0.0):
        _same(_run(layer, x, cf), before[cf], f"capacity_factor {cf}")
    layer.gates[0].capacity_factor = 1.0
    g = GraphedForward(layer, x)
    for _ in range(3):
        _same(g(other), before_other, "a replay on the second batch")


@both
def test_state_dict_holds_the_fp4_form_and_round_trips(oracle, kind, dtype):
    layer, x = _layer(oracle, kind, dtype)
    sd16 = {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}
    layer.experts.fp4_freeze()
    want = _run(layer, x, 1.0)
    sd = layer.experts.state_dict()
    assert sorted(sd) == sorted(FP4_KEYS[kind] + BIASES[kind]), list(sd)
    fresh, _ = _layer(oracle, kind, dtype, seed=34, fp4=False)     # unfrozen, other weights: the state dict freezes it
    res = fresh.load_state_dict({k: v.clone() for k, v in layer.state_dict().items()})
    assert not res.missing_keys and not res.unexpected_keys, res
    assert fresh.experts.fp4_frozen is True and fresh.experts.fp8_frozen is False and [n for n, _ in fresh.experts.named_parameters()] == BIASES[kind]
    _same(_run(fresh, x, 1.0), want, "after load_state_dict")
    frozen2, _ = _layer(oracle, kind, dtype, seed=33)              # frozen from other weights: the 16-bit checkpoint is quantised on arrival
    frozen2.experts.fp4_freeze()
    assert not torch.equal(getattr(frozen2.experts, FP4_KEYS[kind][0]), sd[FP4_KEYS[kind][0]])
    res = frozen2.load_state_dict(sd16)
    assert not res.missing_keys and not res.unexpected_keys, res
    assert all(torch.equal(getattr(frozen2.experts, k), sd[k]) for k in FP4_KEYS[kind])


@both
def test_refusals_raise_with_their_reason(oracle, kind, dtype):
    layer, x = _layer(oracle, kind, dtype)
    ex = layer.experts.fp4_freeze()
    want = _run(layer, x, 1.0)
    for mod in (ex, layer):
        with pytest.raises(RuntimeError, match="FP4-resident.*training mode"):
            mod.train()
    for move in (ex.half if dtype == torch.bfloat16 else ex.bfloat16, ex.cpu):
        with pytest.raises(RuntimeError, match="FP4-resident experts .fp4_freeze. cannot be cast or moved"):
            move()
    with pytest.raises(RuntimeError, match="FP4-resident.*autocast is on"):
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            layer(x)
    with pytest.raises(ValueError, match="fp8_freeze: the module is FP4-resident"):
        ex.fp8_freeze()
    layer.dropless_packed = True
    layer.gates[0].capacity_factor = 0.0
    with pytest.raises(RuntimeError, match="FP4-resident.*the packed dropless forward has no FP4 GEMM"):
        with torch.no_grad():
            layer(x)
    layer.dropless_packed = False
    _same(_run(layer, x, 1.0), want, "after the refusals")
    other, _ = _layer(oracle, kind, dtype, fp4=False)
    other.experts.fp8_freeze()
    with pytest.raises(ValueError, match="fp4_freeze: the module is FP8-resident"):
        other.experts.fp4_freeze()
    if kind == "ffn":                                              # an uncovered shape: ValueError, and the parameters are still there
        small, _ = _layer(oracle, kind, dtype, hidden=48)
        keys = list(small.experts.state_dict())
        with pytest.raises(ValueError, match="fp4_freeze: the shape is not covered"):
            small.experts.fp4_freeze()
        assert list(small.experts.state_dict()) == keys and small.experts.fp4_frozen is False and small.experts.batched_fc1_w.is_cuda
