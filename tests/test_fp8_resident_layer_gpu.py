"""FP8-resident experts in the layer (experts.fp8_freeze(); experts/fp8_resident.py), `ffn` and SwiGLU, bf16 and fp16: the forwards
after the freeze -- padded, dropless, packed FP8 eager and under a HIP graph -- are bit for bit the FP8 forwards before it; memory
falls by exactly the 16-bit weights minus images and scales and never peaks above the images; no expert weight stays a parameter;
the state dict holds the FP8 form and round-trips, a 16-bit checkpoint is quantised on arrival; and every forward that would have
read the 16-bit weights raises with the ladder's reason and launches no 16-bit GEMM."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL                                     # noqa: E402
from test_swiglu_packed_gpu import make_layer as make_swiglu    # noqa: E402

pytestmark = pytest.mark.gpu

T, E, K, M = 96, 4, 2, 128
DTYPES = [torch.bfloat16, torch.float16]
# (ffn_128: the packed dropless layout takes H >= 128 only, so the packed FP8 forward of `ffn` experts needs a wider layer than H = 64)
LAYERS = {"ffn": ("ffn", 64), "ffn_128": ("ffn", 128), "swiglu_64": ("llama_ffn", 64), "swiglu_192": ("llama_ffn", 192)}
FP8_KEYS = {"ffn": ["fc1_w8", "fc1_w8_scale", "fc2_w8", "fc2_w8_scale"], "llama_ffn": ["fc12_w8", "fc12_w8_scale", "fc3_w8", "fc3_w8_scale"]}
W16_KEYS = {"ffn": ["batched_fc1_w", "batched_fc2_w"], "llama_ffn": ["W_fc1", "W_fc2", "W_fc3"]}
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))


class Spy:
    """in front of the loaded library (as tests/test_fp8_weights_layer_gpu.py::Spy): counts the calls by name"""

    def __init__(self, real):
        self._real, self.counts = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args):
            self.counts[name] += 1
            return fn(*args)
        return counted

    def gemms_16bit(self):
        """the one-call pipelines and every grouped GEMM that reads 16-bit (or fp32) weights"""
        return {n: c for n, c in self.counts.items()
                if n.startswith("tutel_amd_moe_forward") or n == "tutel_amd_expert_ffn" or
                (n.startswith("tutel_amd_expert_gemm") and "_w8" not in n and not n.endswith("_supported"))}

    def gemms_fp8(self):
        return sum(c for n, c in self.counts.items() if n.startswith("tutel_amd_expert_gemm_w8") and not n.endswith("_supported"))


@pytest.fixture
def spy(monkeypatch):
    from tutel_amd import _lib
    s = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", s)
    return s


def _layer(oracle, name, dtype, seed=21):
    kind, hidden = LAYERS[name]
    x, wg, w1, b1, w2, b2 = oracle.make_problem(T, M, hidden, E, dtype=dtype, seed=seed)
    gate = {"fp32_gate": True}
    if kind == "ffn":
        layer = TL.make_layer(M, hidden, E, K, 1.0, dtype, (wg, w1, b1, w2, b2), gate=gate).eval()
    else:
        g = torch.Generator().manual_seed(77 + hidden + seed)
        weights = (wg, (torch.randn([E, M, hidden], generator=g) / M ** 0.5).to(dtype), (torch.randn([E, M, hidden], generator=g) / M ** 0.5).to(dtype),
                   (torch.randn([E, hidden, M], generator=g) / hidden ** 0.5).to(dtype))
        layer = make_swiglu(M, hidden, E, K, 1.0, dtype, "top", weights=weights, gate=gate)
        x = x * 0.5
    for p in layer.parameters():
        p.requires_grad_(False)
    layer.experts.fp8_weights = True
    return layer, x.cuda()


def _second_batch(x, dtype):
    return torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dtype).cuda() * 0.5


def _run(layer, x, cf, packed_fp8=False, **kw):
    """one forward -> (y, l_aux); cf: the gate's capacity_factor for this call (0: dropless)"""
    layer.gates[0].capacity_factor = cf
    layer.dropless_packed = layer.dropless_packed_fp8 = packed_fp8
    with torch.no_grad():
        y = layer(x, **kw)
    return y.detach().clone(), layer.l_aux.detach().clone()


def _equal(a, b, what):
    assert a[0].dtype == b[0].dtype and torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)), what + ": output bits"
    assert torch.equal(a[1], b[1]), what + ": l_aux"


# ---- the forwards, before and after ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("name", list(LAYERS))
def test_forwards_after_the_freeze_are_the_fp8_forwards_before_it(oracle, spy, name, dtype):
    from tutel_amd.impls.graph import GraphedForward
    layer, x = _layer(oracle, name, dtype)
    other = _second_batch(x, dtype)
    before = {}
    for what, cf in (("padded", 1.0), ("dropless", 0.0)):
        before[what] = _run(layer, x, cf)
        assert layer._fp8_weights_ran is True, (what, layer._fp8_weights_ran)
    before["dropless_other"] = _run(layer, other, 0.0)
    assert not spy.gemms_16bit(), spy.gemms_16bit()
    assert float(before["padded"][0].abs().max()) > 0 and bool(torch.isfinite(before["dropless"][0].float()).all())

    assert layer.experts.fp8_freeze() is layer.experts and layer.experts.fp8_frozen is True and layer.experts.fp8_weights is True
    spy.counts.clear()
    for what, cf in (("padded", 1.0), ("dropless", 0.0)):
        after = _run(layer, x, cf)
        assert layer._fp8_weights_ran is True, (what, layer._fp8_weights_ran)
        _equal(after, before[what], what)
    assert spy.gemms_fp8() == 4 and not spy.gemms_16bit(), spy.counts
    assert spy.counts["tutel_amd_quantize_w8"] == 0, "a frozen module quantises nothing in a forward"

    # the packed FP8 forward, eager and under a graph, against the padded dropless FP8 forward
    if LAYERS[name][1] < 128:   # the packed layout refuses H < 128; unfrozen that forward is the 16-bit packed one: here it raises
        spy.counts.clear()
        with pytest.raises(RuntimeError, match="hold no 16-bit weights.*tutel_amd_packed_plan: not covered"):
            _run(layer, x, 0.0, packed_fp8=True)
        assert not spy.gemms_16bit() and spy.gemms_fp8() == 0, spy.counts
        return
    packed = _run(layer, x, 0.0, packed_fp8=True)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True, (layer._dropless_packed_ran, layer._fp8_weights_ran)
    _equal(packed, before["dropless"], "packed FP8, eager")
    layer.dropless_packed = layer.dropless_packed_fp8 = True
    g = GraphedForward(layer, x, dropless_packed=True)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True, "the capture took the packed FP8 route"
    calls = dict(spy.counts)
    for _ in range(3):
        y = g(other)
        assert torch.equal(y.view(torch.int16), before["dropless_other"][0].view(torch.int16)), "a replay on the second batch"
    assert dict(spy.counts) == calls and not spy.gemms_16bit(), "replays make no library call"


# ---- memory, parameters ------------------------------------------------------------------------------------------------------------
def _bytes(t):
    return t.numel() * t.element_size()


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("name", list(LAYERS))
def test_memory_falls_by_the_weights_minus_the_images_and_peaks_at_the_images(oracle, name, dtype):
    """every tensor involved is a multiple of 512 bytes, so the allocator's rounding does not enter.  The peak bound -- memory before
    the freeze plus ALL images and scales plus 4 KiB for the status words -- follows from quantising one parameter at a time with
    nothing but image and scales allocated; the torch quantiser's fp32 copy of one parameter alone is larger than that margin"""
    from tutel_amd import ops
    kind, _ = LAYERS[name]
    layer, _x = _layer(oracle, name, dtype)
    ex = layer.experts
    ops.quantize_w8(torch.zeros([1, 32, 32], dtype=dtype, device="cuda"), True, check_only=True)   # (the library is loaded and warm)
    weights = [getattr(ex, n) for n in W16_KEYS[kind]]
    released = sum(_bytes(w) for w in weights)
    largest_fp32_copy = max(w.numel() for w in weights) * 4
    assert all(_bytes(w) % 512 == 0 for w in weights)
    del weights
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ex.fp8_freeze()
    torch.cuda.synchronize()
    after, peak = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
    bufs = [getattr(ex, n) for n in FP8_KEYS[kind]]
    images = sum(_bytes(b) for b in bufs)
    assert all(_bytes(b) % 512 == 0 for b in bufs)
    print(f"\n{name} {dtype}: released {released} B, images + scales {images} B, allocated {base} -> {after} B, peak {peak} B")
    assert base - after == released - images, (base, after, released, images)
    assert peak <= base + images + 4096, (peak, base, images)
    assert largest_fp32_copy > images + 4096, "the torch quantiser's fp32 copy of one parameter alone exceeds the bound's margin"
    # no expert weight is left among the parameters
    names = [n for n, _ in ex.named_parameters()]
    assert names == (["batched_fc1_bias", "batched_fc2_bias"] if kind == "ffn" else []), names
    for n in W16_KEYS[kind]:
        t = getattr(ex, n)
        assert t.device.type == "meta" and not isinstance(t, torch.nn.Parameter), "shape and dtype stay answerable, nothing else"


# ---- state dict --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("name", ["ffn", "swiglu_64"])
def test_state_dict_holds_the_fp8_form_and_round_trips(oracle, name, dtype):
    kind, _ = LAYERS[name]
    layer, x = _layer(oracle, name, dtype)
    sd16 = {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}      # the 16-bit checkpoint, held on the CPU
    layer.experts.fp8_freeze()
    want = _run(layer, x, 1.0)
    sd = layer.experts.state_dict()
    biases = ["batched_fc1_bias", "batched_fc2_bias"] if kind == "ffn" else []
    assert sorted(sd) == sorted(FP8_KEYS[kind] + biases), list(sd)
    assert not any(k in sd for k in W16_KEYS[kind])
    assert all(sd[k].dtype == (torch.float32 if k.endswith("_scale") else torch.uint8) for k in FP8_KEYS[kind])
    full = {k: v.clone() for k, v in layer.state_dict().items()}

    # into a second frozen module (other weights), and into an unfrozen one, which becomes frozen
    frozen2, _ = _layer(oracle, name, dtype, seed=33)
    frozen2.experts.fp8_freeze()
    assert not torch.equal(frozen2.experts.state_dict()[FP8_KEYS[kind][0]], sd[FP8_KEYS[kind][0]])
    unfrozen, _ = _layer(oracle, name, dtype, seed=34)
    for other in (frozen2, unfrozen):
        res = other.load_state_dict(full)
        assert not res.missing_keys and not res.unexpected_keys, res
        assert other.experts.fp8_frozen is True and other.experts.fp8_weights is True
        assert [n for n, _ in other.experts.named_parameters()] == biases
        for k in FP8_KEYS[kind]:
            assert torch.equal(other.experts.state_dict()[k], sd[k]), k
        _equal(_run(other, x, 1.0), want, "after load_state_dict")
        assert other._fp8_weights_ran is True

    # the 16-bit checkpoint into the frozen module whose buffers were zeroed: quantised on arrival, the first freeze's bits
    for k in FP8_KEYS[kind]:
        getattr(layer.experts, k).zero_()
    res = layer.load_state_dict(sd16)
    assert not res.missing_keys and not res.unexpected_keys, res
    for k in FP8_KEYS[kind]:
        assert torch.equal(getattr(layer.experts, k), sd[k]), k
    _equal(_run(layer, x, 1.0), want, "after the 16-bit checkpoint")

    # mismatches are load_state_dict's errors
    bad = dict(sd16)
    key = "experts." + W16_KEYS[kind][0]
    bad[key] = bad[key].reshape(-1)[:-64].clone()
    with pytest.raises(RuntimeError, match="size mismatch for " + key):
        layer.load_state_dict(bad)
    bad[key] = sd16[key].to(torch.float32)
    with pytest.raises(RuntimeError, match="dtype mismatch for " + key):
        layer.load_state_dict(bad)
    bad = dict(full)
    bad["experts." + FP8_KEYS[kind][0]] = full["experts." + FP8_KEYS[kind][0]][:, :1].clone()
    with pytest.raises(RuntimeError, match="size mismatch"):
        layer.load_state_dict(bad)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("name", ["ffn", "swiglu_64"])
def test_forwards_that_would_read_16_bit_weights_raise_with_the_reason(oracle, spy, name, dtype):
    layer, x = _layer(oracle, name, dtype)
    layer.experts.fp8_freeze()
    want = _run(layer, x, 1.0)
    spy.counts.clear()
    layer.gates[0].capacity_factor = 1.0

    with pytest.raises(RuntimeError, match="autocast is on"):
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            layer(x)
    with pytest.raises(RuntimeError, match="not bf16 / fp16 in the experts' own dtype"):     # the experts themselves: the layer casts its input
        with torch.no_grad():
            layer.experts(torch.zeros([E, 8, M], dtype=torch.float32, device="cuda"), layer)
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    with pytest.raises(RuntimeError, match="not bf16 / fp16 in the experts' own dtype"):
        with torch.no_grad():
            layer.experts(torch.zeros([E, 8, M], dtype=other, device="cuda"), layer)
    with pytest.raises(RuntimeError, match="autograd is live"):
        with torch.enable_grad():
            layer(x.clone().requires_grad_(True))
    if name == "ffn":   # (SwiGLU experts' ladder has no megablocks rung: they take any)
        with pytest.raises(RuntimeError, match="megablocks row counts are not covered"):
            with torch.no_grad():
                layer(x, megablocks_size=4)
    for mod in (layer.experts, layer):
        with pytest.raises(RuntimeError, match="training mode"):
            mod.train()
    layer.eval()
    with pytest.raises(RuntimeError, match="cannot be cast or moved"):
        layer.experts.float()
    assert not spy.gemms_16bit() and spy.gemms_fp8() == 0, spy.counts
    # ... and the module is what it was
    _equal(_run(layer, x, 1.0), want, "after the refusals")
    assert layer._fp8_weights_ran is True


def test_fp8_freeze_refuses_what_the_ladder_refuses_and_leaves_the_module_untouched(oracle):
    for name, change, word in (("ffn", lambda ex: ex.float(), "not bf16 / fp16"), ("swiglu_64", lambda ex: ex.train(), "training mode"),
                               ("ffn", lambda ex: setattr(ex, "activation_fn", lambda t: t.clamp(0, 6)) or ex._act_cache.clear(), "activation")):
        layer, _x = _layer(oracle, name, torch.bfloat16)
        change(layer.experts)
        keys = list(layer.experts.state_dict())
        with pytest.raises(ValueError, match=word):
            layer.experts.fp8_freeze()
        assert list(layer.experts.state_dict()) == keys and layer.experts.fp8_frozen is False
    # a non-finite weight: found before anything is released
    layer, _x = _layer(oracle, "swiglu_64", torch.bfloat16)
    with torch.no_grad():
        layer.experts.W_fc3.view(layer.experts.W_fc3_full_shape)[2, 5, 7] = float("inf")
    keys = list(layer.experts.state_dict())
    with pytest.raises(ValueError, match=r"channel \(expert 2, output 7\) holds a non-finite weight"):
        layer.experts.fp8_freeze()
    assert list(layer.experts.state_dict()) == keys and layer.experts.fp8_frozen is False
    assert isinstance(layer.experts.W_fc1, torch.nn.Parameter) and layer.experts.W_fc1.is_cuda
