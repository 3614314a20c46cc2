"""FP8 (e4m3) expert weights in a SwiGLU (llama_ffn) layer (switch experts.fp8_weights, off by default): the switched-on forward makes
exactly one call of tutel_amd_expert_gemm_w8_glu and one of tutel_amd_expert_gemm_w8 and none of the 16-bit GEMMs or the one-call
pipelines, routes as the switched-off forward does, and agrees with the oracle layer run over the dequantised weights q * scale with
the gate rounded; an in-place update of any of the three weights re-quantises; every forward that must keep the 16-bit weights does,
bit for bit, with its reason; graph replays."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL                     # noqa: E402
from test_swiglu_packed_gpu import make_layer   # noqa: E402

pytestmark = pytest.mark.gpu

GLU, FC3 = "tutel_amd_expert_gemm_w8_glu", "tutel_amd_expert_gemm_w8"
T, M, H, E, K = 300, 256, 256, 8, 2
DTYPES = [torch.bfloat16, torch.float16]
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

    def fp8(self):
        return (self.counts[GLU], self.counts[FC3])

    def other_gemms(self):
        return {n: c for n, c in self.counts.items()
                if n not in (GLU, FC3) and (n.startswith("tutel_amd_moe_forward") or
                                            (n.startswith("tutel_amd_expert_gemm") and not n.endswith("_supported")))}


@pytest.fixture
def spy(monkeypatch):
    from tutel_amd import _lib
    s = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", s)
    return s


def _problem(oracle, dtype, hidden=H):
    """x and the gate from the oracle's generator (x halved: |y| stays below 1, the fp16 bar is absolute), SwiGLU weights spread as
    tests/test_swiglu_packed_gpu.py spreads them; everything rounded to the dtype"""
    x, wg, *_ = oracle.make_problem(T, M, hidden, E, dtype=dtype, seed=21)
    g = torch.Generator().manual_seed(77 + hidden)
    w1 = (torch.randn([E, M, hidden], generator=g) / M ** 0.5).to(dtype)
    w2 = (torch.randn([E, M, hidden], generator=g) / M ** 0.5).to(dtype)
    w3 = (torch.randn([E, hidden, M], generator=g) / hidden ** 0.5).to(dtype)
    return x * 0.5, (wg, w1, w2, w3)


def _layer(oracle, dtype, hidden=H, cf=1.0, **kw):
    x, weights = _problem(oracle, dtype, hidden)
    layer = make_layer(M, hidden, E, K, cf, dtype, "top", weights=weights, gate={"fp32_gate": True}, **kw)   # (the oracle's routing: fp32 scores)
    layer._keep_routing = True
    return layer, x.cuda(), weights


def _run(layer, x, on, autocast=False, **kw):
    layer.experts.fp8_weights = on
    layer.last_routing = ()
    with torch.no_grad(), torch.autocast("cuda", dtype=x.dtype, enabled=autocast):
        y = layer(x, **kw)
    return (y.detach().clone(), layer.l_aux.detach().clone(), layer.dispatch_count.clone(), tuple(t.clone() for t in layer.last_routing))


def _same_routing(a, b):
    assert torch.equal(a[2], b[2]) and len(a[3]) == len(b[3]) and all(torch.equal(p, q) for p, q in zip(a[3], b[3])), "routing bits"
    assert torch.equal(a[1], b[1]), "l_aux"


def _dequantised_expert_fn(weights, dtype):
    """the kernels' contract over the EXACT dequantised weights q * scale in fp32: the gate rounded to the dtype before the product,
    the product rounded once, the output rounded once"""
    from tutel_amd.experts import w8
    _, w1, w2, w3 = weights
    d1, d2, d3 = (w8.dequantize(*w8.quantize_e4m3(w, False)) for w in (w1, w2, w3))   # [E, H, M], [E, H, M], [E, M, H] fp32

    def fn(enc):
        ef = enc.float()
        g = torch.nn.functional.silu(torch.matmul(ef, d1.permute(0, 2, 1))).to(dtype).float()
        h = (g * torch.matmul(ef, d2.permute(0, 2, 1))).to(dtype).float()
        return torch.matmul(h, d3.permute(0, 2, 1)).to(dtype)
    return fn


def _oracle(oracle, x, weights, dtype, cf=1.0):
    wg, w1, _, _ = weights
    return oracle.moe_forward(x.cpu(), wg, w1, None, None, None, top_k=K, capacity_factor=cf, fp32_gate=True,
                              expert_fn=_dequantised_expert_fn(weights, dtype))


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_switch_on_two_calls_same_routing_and_the_oracle_over_dequantised_weights(oracle, spy, dtype):
    layer, x, weights = _layer(oracle, dtype)
    off = _run(layer, x, False)
    assert spy.fp8() == (0, 0) and layer._fp8_weights_ran is None, "switch off: no new call"
    assert spy.counts[GLU + "_supported"] == 0 and spy.counts[FC3 + "_supported"] == 0
    spy.counts.clear()
    on = _run(layer, x, True)
    assert spy.fp8() == (1, 1) and layer._fp8_weights_ran is True, (spy.counts, layer._fp8_weights_ran)
    assert not spy.other_gemms(), spy.other_gemms()
    _same_routing(on, off)
    yo, lo, crit, _ = _oracle(oracle, x, weights, dtype)
    assert torch.equal(on[3][0].cpu(), torch.stack(crit[1]).to(torch.int32)) and torch.equal(on[3][1].cpu(), torch.stack(crit[2]).to(torch.int32))
    TL._close(on[0], yo, dtype)
    # what quantising the weights does to this layer: reported, not asserted
    d = (on[0].double() - off[0].double()).abs()
    print(f"\nfp8 weights, SwiGLU, {dtype}: |y_fp8 - y_16bit| max {float(d.max()):.4e} mean {float(d.mean()):.4e}; |y_16bit| max "
          f"{float(off[0].abs().max()):.4f} mean {float(off[0].double().abs().mean()):.4e}")
    assert bool(torch.isfinite(on[0].float()).all()) and float(on[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_switch_off_is_the_parent_forward(oracle, spy, dtype):
    layer, x, _ = _layer(oracle, dtype)
    off = _run(layer, x, False)
    assert layer._fp8_weights_ran is None and spy.fp8() == (0, 0)
    assert spy.counts[GLU + "_supported"] == 0 and spy.counts[FC3 + "_supported"] == 0
    assert "off" in layer.experts.w8_refusal(x, layer)
    assert not layer.experts.w8_cached(), "nothing was quantised"
    again = _run(layer, x, False)
    assert torch.equal(off[0], again[0])


@pytest.mark.parametrize("param,factor", [("W_fc1", 0.5), ("W_fc2", 2.0), ("W_fc3", 2.0)])
def test_in_place_weight_update_requantises(oracle, spy, param, factor):
    """a power of two in place (exact in bf16: the codes stay, the scales move): the next forward equals the oracle over the NEW
    dequantised weights and differs from the stale output"""
    dtype = torch.bfloat16
    layer, x, weights = _layer(oracle, dtype)
    before = _run(layer, x, True)
    assert layer._fp8_weights_ran is True
    with torch.no_grad():
        getattr(layer.experts, param).mul_(factor)
    after = _run(layer, x, True)
    assert layer._fp8_weights_ran is True and spy.fp8() == (2, 2)
    wg, w1, w2, w3 = weights
    new = (wg, w1 * factor if param == "W_fc1" else w1, w2 * factor if param == "W_fc2" else w2, w3 * factor if param == "W_fc3" else w3)
    yo, *_ = _oracle(oracle, x, new, dtype)
    TL._close(after[0], yo, dtype)
    assert not torch.equal(after[0], before[0]), "the cached images were not rebuilt"
    _same_routing(after, before)


FALLBACKS = {   # name -> (layer kwargs, attributes set on the layer, run kwargs, a word of the reason)
    "training_mode": ({}, {}, dict(train=True), "training mode"),
    "autocast": ({}, {}, dict(autocast=True), "autocast"),
    "hidden_size_96": (dict(hidden=96), {}, {}, "shape"),
    "dropless_packed": (dict(cf=0.0), dict(dropless_packed=True), {}, "the packed dropless forward has no FP8 GEMM"),
}


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_keep_the_16_bit_weights_bit_for_bit(oracle, spy, case, dtype):
    layer_kw, attrs, run_kw, word = FALLBACKS[case]
    layer, x, _ = _layer(oracle, dtype, **layer_kw)
    for name, value in attrs.items():
        setattr(layer, name, value)
    run_kw = dict(run_kw)
    if run_kw.pop("train", False):
        layer.train()
        for p in layer.parameters():
            p.requires_grad_(False)
    off = _run(layer, x, False, **run_kw)
    assert layer._fp8_weights_ran is None
    on = _run(layer, x, True, **run_kw)
    assert spy.fp8() == (0, 0), "a new entry point was called"
    assert isinstance(layer._fp8_weights_ran, str) and word in layer._fp8_weights_ran, layer._fp8_weights_ran
    if case == "dropless_packed":
        assert layer._dropless_packed_ran is True and spy.counts["tutel_amd_moe_forward_packed_glu"] == 2, "it keeps its one-call path"
    _same_routing(on, off)
    assert on[0].dtype == off[0].dtype and torch.equal(on[0], off[0]), "bit-equal to switch-off"
    assert bool(torch.isfinite(on[0].float()).all()) and float(on[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_graph_capture_replays_the_eager_forward(oracle, spy, dtype):
    from tutel_amd.impls.graph import GraphedForward
    layer, x, _ = _layer(oracle, dtype)
    layer._keep_routing = False
    layer.experts.fp8_weights = True
    with torch.no_grad():
        eager = layer(x).clone()
    assert layer._fp8_weights_ran is True and spy.fp8() == (1, 1)
    other = (torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) * 0.5).to(dtype).cuda()
    with torch.no_grad():
        eager_other = layer(other).clone()
    g = GraphedForward(layer, x)
    assert layer._fp8_weights_ran is True
    calls = spy.fp8()
    for _ in range(3):
        assert torch.equal(g(other), eager_other), "a replay on the second batch"
        assert torch.equal(g(x), eager), "a replay against the eager forward"
    assert spy.fp8() == calls, "replays make no library call"


def test_first_use_inside_a_capture_keeps_the_16_bit_weights_with_a_reason(oracle):
    """with nothing cached, a forward under stream capture must not quantise (that would allocate the images in the graph's pool):
    the predicate names the reason and the 16-bit weights are read"""
    layer, x, _ = _layer(oracle, torch.bfloat16)
    layer.experts.fp8_weights = True
    with torch.no_grad():
        assert layer.experts.fused_activation() == "silu" and layer.experts.w8_refusal(x, layer) is None, "admitted outside a capture"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.no_grad():
        with torch.cuda.graph(g, stream=s):
            why = layer.experts.w8_refusal(x, layer)
    torch.cuda.current_stream().wait_stream(s)
    assert isinstance(why, str) and "eager forward" in why
    assert not layer.experts.w8_cached()
