"""FP8 (e4m3) expert weights in the layer (switch experts.fp8_weights, off by default): the switched-on forward makes exactly two calls of
tutel_amd_expert_gemm_w8 and none of the 16-bit GEMMs or the one-call pipeline, routes as the switched-off forward does, and agrees
with the oracle layer run over the dequantised weights q * scale; the gathered form equals the bucket form bit for bit; an in-place
weight update re-quantises; every forward that must keep the 16-bit weights does, bit for bit, with its reason; graph replays."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL            # noqa: E402

pytestmark = pytest.mark.gpu

ENTRY = "tutel_amd_expert_gemm_w8"
T, M, H, E, K = 300, 256, 256, 8, 2
DTYPES = [torch.bfloat16, torch.float16]
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))


class Spy:
    """in front of the loaded library (as tests/test_fp32_experts_layer_gpu.py::Spy): counts the calls by name and keeps, per call of
    the W8A16 grouped GEMM, whether it gathered (slot_map, argument 22)"""

    def __init__(self, real):
        self._real, self.counts, self.gathered = real, collections.Counter(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args):
            self.counts[name] += 1
            if name == ENTRY:
                self.gathered.append(bool(args[22]))
            return fn(*args)
        return counted

    def other_gemms(self):
        return {n: c for n, c in self.counts.items()
                if n != ENTRY and (n == "tutel_amd_moe_forward" or (n.startswith("tutel_amd_expert_gemm") and not n.endswith("_supported")))}


@pytest.fixture
def spy(monkeypatch):
    from tutel_amd import _lib
    s = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", s)
    return s


def _layer(oracle, dtype, hidden=H, cf=1.0, **kw):
    x, *weights = oracle.make_problem(T, M, hidden, E, dtype=dtype, seed=21)
    layer = TL.make_layer(M, hidden, E, K, cf, dtype, weights, gate={"fp32_gate": True}, **kw).eval()   # (the oracle's routing: fp32 scores)
    layer._keep_routing = True
    return layer, x.cuda(), weights


def _run(layer, x, on, grad=False, autocast=False, **kw):
    layer.experts.fp8_weights = on
    with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=x.dtype, enabled=autocast):
        y = layer(x, **kw)
    return (y.detach().clone(), layer.l_aux.detach().clone(), layer.dispatch_count.clone(),
            tuple(t.clone() for t in layer.last_routing))


def _same_routing(a, b):
    assert torch.equal(a[2], b[2]) and torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1]), "routing bits"
    assert torch.equal(a[1], b[1]), "l_aux"


def _dequantised_expert_fn(weights, dtype):
    """the oracle's fp32-accumulating FFN (oracle.expert_ffn, accum_fp32) over the EXACT dequantised weights q * scale in fp32"""
    from tutel_amd.experts import w8
    _, w1, b1, w2, b2 = weights
    q1, s1 = w8.quantize_e4m3(w1, True)
    q2, s2 = w8.quantize_e4m3(w2, False)
    d1, d2 = w8.dequantize(q1, s1), w8.dequantize(q2, s2)   # [E, H, M], [E, M_out, H] fp32

    def fn(enc):
        h = torch.relu(torch.matmul(enc.float(), d1.permute(0, 2, 1)) + b1.float().unsqueeze(1)).to(dtype).float()
        return (torch.matmul(h, d2.permute(0, 2, 1)) + b2.float().unsqueeze(1)).to(dtype)
    return fn


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_switch_on_two_calls_same_routing_and_the_oracle_over_dequantised_weights(oracle, spy, dtype):
    layer, x, weights = _layer(oracle, dtype)
    off = _run(layer, x, False)
    assert spy.counts[ENTRY] == 0 and layer._fp8_weights_ran is None, "switch off: no new call"
    assert spy.counts["tutel_amd_expert_gemm_w8_supported"] == 0
    spy.counts.clear()
    on = _run(layer, x, True)
    assert spy.counts[ENTRY] == 2 and layer._fp8_weights_ran is True, (spy.counts, layer._fp8_weights_ran)
    assert not spy.other_gemms(), spy.other_gemms()
    assert spy.gathered == [True, False], "single rank, is_postscore: fc1 gathers its rows from the tokens"
    _same_routing(on, off)
    yo, lo, crit, _ = oracle.moe_forward(x.cpu(), *weights, top_k=K, capacity_factor=1.0, fp32_gate=True, expert_fn=_dequantised_expert_fn(weights, dtype))
    assert torch.equal(on[3][0].cpu(), torch.stack(crit[1]).to(torch.int32)) and torch.equal(on[3][1].cpu(), torch.stack(crit[2]).to(torch.int32))
    TL._close(on[0], yo, dtype)
    # what quantising the weights does to this layer: reported, not asserted
    d = (on[0].double() - off[0].double()).abs()
    print(f"\nfp8 weights, {dtype}: |y_fp8 - y_16bit| max {float(d.max()):.4e} mean {float(d.mean()):.4e}; |y_16bit| max "
          f"{float(off[0].abs().max()):.4f} mean {float(off[0].double().abs().mean()):.4e}")
    assert bool(torch.isfinite(on[0].float()).all()) and float(on[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_fused_encode_against_the_bucket_form(oracle, monkeypatch, spy, dtype):
    """the gather is a row copy: _FUSE_ENCODE off (fast_encode + the bucket form inside FusedExpertsNetwork.forward) and on (fc1
    gathers) give equal output bits"""
    from tutel_amd.impls import moe_layer as ML
    layer, x, _ = _layer(oracle, dtype)
    monkeypatch.setattr(ML, "_FUSE_ENCODE", False)
    bucket = _run(layer, x, True)
    assert spy.gathered == [False, False] and layer._fp8_weights_ran is True and not spy.other_gemms()
    monkeypatch.setattr(ML, "_FUSE_ENCODE", True)
    fused = _run(layer, x, True)
    assert spy.gathered == [False, False, True, False] and layer._fp8_weights_ran is True
    _same_routing(fused, bucket)
    assert torch.equal(fused[0].view(torch.int16), bucket[0].view(torch.int16))


def test_prescore_layer_takes_the_bucket_form(oracle, spy):
    layer, x, weights = _layer(oracle, torch.bfloat16, is_postscore=False)
    on = _run(layer, x, True)
    assert spy.counts[ENTRY] == 2 and spy.gathered == [False, False] and layer._fp8_weights_ran is True and not spy.other_gemms()
    yo, *_ = oracle.moe_forward(x.cpu(), *weights, top_k=K, capacity_factor=1.0, fp32_gate=True, is_postscore=False,
                                expert_fn=_dequantised_expert_fn(weights, torch.bfloat16))
    TL._close(on[0], yo, torch.bfloat16)


def test_in_place_weight_update_requantises(oracle, spy):
    """w2 *= 2, w1 *= 0.5 in place (exact in bf16: the codes stay, the scales move): the next forward equals the oracle over the NEW
    dequantised weights and differs from the stale output"""
    dtype = torch.bfloat16
    layer, x, weights = _layer(oracle, dtype)
    before = _run(layer, x, True)
    with torch.no_grad():
        layer.experts.batched_fc2_w.mul_(2)
        layer.experts.batched_fc1_w.mul_(0.5)
    after = _run(layer, x, True)
    wg, w1, b1, w2, b2 = weights
    new = (wg, w1 * 0.5, b1, w2 * 2, b2)
    yo, *_ = oracle.moe_forward(x.cpu(), *new, top_k=K, capacity_factor=1.0, fp32_gate=True, expert_fn=_dequantised_expert_fn(new, dtype))
    TL._close(after[0], yo, dtype)
    assert not torch.equal(after[0], before[0]), "the cached images were not rebuilt"
    _same_routing(after, before)


FALLBACKS = {   # name -> (layer kwargs, forward kwargs, run kwargs, a word of the reason)
    "training_mode": ({}, {}, dict(train=True), "training mode"),
    "autocast": ({}, {}, dict(autocast=True), "autocast"),
    "dropless_megablocks_4": (dict(cf=0.0), dict(megablocks_size=4), {}, "megablocks"),
    "hidden_size_96": (dict(hidden=96), {}, {}, "shape"),
}


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_keep_the_16_bit_weights_bit_for_bit(oracle, spy, case, dtype):
    layer_kw, fwd_kw, run_kw, word = FALLBACKS[case]
    layer, x, _ = _layer(oracle, dtype, **layer_kw)
    run_kw = dict(run_kw)
    if run_kw.pop("train", False):
        layer.train()
        for p in layer.parameters():
            p.requires_grad_(False)
    off = _run(layer, x, False, **run_kw, **fwd_kw)
    on = _run(layer, x, True, **run_kw, **fwd_kw)
    assert spy.counts[ENTRY] == 0, "the new entry point was called"
    assert isinstance(layer._fp8_weights_ran, str) and word in layer._fp8_weights_ran, layer._fp8_weights_ran
    _same_routing(on, off)
    assert on[0].dtype == off[0].dtype and torch.equal(on[0], off[0]), "bit-equal to switch-off"
    assert bool(torch.isfinite(on[0].float()).all()) and float(on[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_switch_off_is_the_parent_forward(oracle, spy, dtype):
    layer, x, _ = _layer(oracle, dtype)
    off = _run(layer, x, False)
    assert layer._fp8_weights_ran is None and spy.counts[ENTRY] == 0 and spy.counts["tutel_amd_expert_gemm_w8_supported"] == 0
    assert "off" in layer.experts.w8_refusal(x, layer)
    assert not layer.experts._kmajor.holds("fc1.w8", layer.experts.batched_fc1_w, "w8"), "nothing was quantised"
    again = _run(layer, x, False)
    assert torch.equal(off[0], again[0])


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_graph_capture_replays_the_eager_forward(oracle, spy, dtype):
    from tutel_amd.impls.graph import GraphedForward
    layer, x, _ = _layer(oracle, dtype)
    layer._keep_routing = False
    layer.experts.fp8_weights = True
    with torch.no_grad():
        eager = layer(x).clone()
    assert layer._fp8_weights_ran is True and spy.counts[ENTRY] == 2
    other = (torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dtype)).cuda()
    with torch.no_grad():
        eager_other = layer(other).clone()
    g = GraphedForward(layer, x)
    assert layer._fp8_weights_ran is True
    calls = spy.counts[ENTRY]
    for _ in range(3):
        assert torch.equal(g(other), eager_other), "a replay on the second batch"
        assert torch.equal(g(x), eager), "a replay against the eager forward"
    assert spy.counts[ENTRY] == calls, "replays make no library call"


def test_first_use_inside_a_capture_falls_back_with_a_reason(oracle):
    """with nothing cached, a forward under stream capture must not quantise (that would allocate the images in the graph's pool):
    the predicate names the reason and the 16-bit weights are read"""
    layer, x, _ = _layer(oracle, torch.bfloat16)
    layer.experts.fp8_weights = True
    with torch.no_grad():
        assert layer.experts.fused_activation() == "relu" and layer.experts.w8_refusal(x, layer) is None, "admitted outside a capture"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.no_grad():
        with torch.cuda.graph(g, stream=s):
            why = layer.experts.w8_refusal(x, layer)
    torch.cuda.current_stream().wait_stream(s)
    assert isinstance(why, str) and "eager forward" in why
    assert not layer.experts._kmajor.holds("fc1.w8", layer.experts.batched_fc1_w, "w8")
