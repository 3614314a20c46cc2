"""MXFP4 expert weights in the layer (switch experts.fp4_weights, off by default), `ffn` and SwiGLU (`llama_ffn`) experts: the
switched-on forward makes exactly two calls of the W4A16 entry points (gathered then plain; glu then plain) and none of the 16-bit
GEMMs, its experts' output equals the ops called directly on the routed rows bit for bit, the layer agrees with the same layer over
the dequantised weights; a parameter update rebuilds the images; every forward that must keep its weights does, with its reason;
graph replays."""
import collections
import gc
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL                                        # noqa: E402
from test_swiglu_packed_gpu import make_layer as make_glu_layer   # noqa: E402

pytestmark = pytest.mark.gpu

PLAIN, GLU = "tutel_amd_expert_gemm_w4", "tutel_amd_expert_gemm_w4_glu"
T, M, H, HG, E, K = 64, 128, 128, 64, 8, 2
DTYPES = [torch.bfloat16, torch.float16]
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))


class Spy:
    """in front of the loaded library: counts the calls by name and keeps, per call of a W4A16 GEMM, (name, whether it gathered)"""

    def __init__(self, real):
        self._real, self.counts, self.w4 = real, collections.Counter(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args):
            self.counts[name] += 1
            if name in (PLAIN, GLU):
                self.w4.append((name, bool(args[-4])))   # slot_map: the fourth argument from the end in both
            return fn(*args)
        return counted

    def other_gemms(self):
        return {n: c for n, c in self.counts.items()
                if n not in (PLAIN, GLU) and (n.startswith("tutel_amd_moe_forward") or
                                              (n.startswith("tutel_amd_expert_gemm") and not n.endswith("_supported")))}


@pytest.fixture(autouse=True)
def leave_no_garbage():
    """layers, graphs and their device memory are gone when a test of this file ends, not whenever the cycle collector next runs: a
    later test that measures torch.cuda.memory_allocated() must not see this file's memory released in the middle of it"""
    yield
    gc.collect()


@pytest.fixture
def spy(monkeypatch):
    from tutel_amd import _lib
    s = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", s)
    return s


# the W4A16 kernel test's bar (the 16-bit GEMM's): the accumulator and the single rounding are the same
def _tol(dtype):
    return dict(rtol=2.0 ** -7, atol=2e-3) if dtype == torch.bfloat16 else dict(rtol=2.0 ** -10, atol=3e-4)


def _layer(oracle, kind, dtype, model_dim=M, **kw):
    if kind == "ffn":
        x, *weights = oracle.make_problem(T, model_dim, H, E, dtype=dtype, seed=21)
        layer = TL.make_layer(model_dim, H, E, K, 1.0, dtype, weights, gate={"fp32_gate": True}, **kw).eval()
    else:
        x, wg, *_ = oracle.make_problem(T, model_dim, HG, E, dtype=dtype, seed=21)
        g = torch.Generator().manual_seed(77)
        w1 = (torch.randn([E, model_dim, HG], generator=g) / model_dim ** 0.5).to(dtype)
        w2 = (torch.randn([E, model_dim, HG], generator=g) / model_dim ** 0.5).to(dtype)
        w3 = (torch.randn([E, HG, model_dim], generator=g) / HG ** 0.5).to(dtype)
        x = x * 0.5
        layer = make_glu_layer(model_dim, HG, E, K, 1.0, dtype, "top", weights=(wg, w1, w2, w3), gate={"fp32_gate": True}, **kw).eval()
    for p in layer.parameters():
        p.requires_grad_(False)
    return layer, x.cuda()


def _run(layer, x, fp4, fp8=False, autocast=False, **kw):
    layer.experts.fp4_weights, layer.experts.fp8_weights = fp4, fp8
    with torch.no_grad(), torch.autocast("cuda", dtype=x.dtype, enabled=autocast):
        y = layer(x, **kw)
    return y.detach().clone()


def _weight_params(layer, kind):
    ex = layer.experts
    return [(ex.batched_fc1_w, True), (ex.batched_fc2_w, False)] if kind == "ffn" else \
        [(ex.W_fc1.view(ex.W_fc1_full_shape), False), (ex.W_fc2.view(ex.W_fc2_full_shape), False), (ex.W_fc3.view(ex.W_fc3_full_shape), False)]


def _record_experts(layer, kind, monkeypatch):
    """what the experts were given and what they returned: (x, R, slot_map, y) per call"""
    seen = []
    ex = layer.experts
    if kind == "ffn":
        real = ex.forward_engine

        def forward_engine(engine, x, R=None, slot_map=None):
            y = real(engine, x, R, slot_map)
            seen.append((x, R, slot_map, y))
            return y
        monkeypatch.setattr(ex, "forward_engine", forward_engine)
    else:
        real = ex.forward_fused_w4

        def forward_fused_w4(x):
            y = real(x)
            seen.append((x, None, None, y))
            return y
        monkeypatch.setattr(ex, "forward_fused_w4", forward_fused_w4)
    return seen


def _direct(layer, kind, x, R, slot_map):
    """the ops called directly on the routed rows, over images prepared here from the parameters on the CPU"""
    from tutel_amd import ops
    from tutel_amd.experts import w4
    ex = layer.experts
    ws = [(w.detach().cpu(), km) for w, km in _weight_params(layer, kind)]
    if kind == "ffn":
        (c1, s1), (c2, s2) = (tuple(t.cuda() for t in w4.prepare(w, km)) for w, km in ws)
        h = ops.expert_gemm_w4(x, c1, s1, ex.batched_fc1_bias.detach(), H, x.shape[-1], act="relu", slot_map=slot_map, R=R)
        return ops.expert_gemm_w4(h, c2, s2, ex.batched_fc2_bias.detach(), ex.batched_fc2_w.size(2), H)
    cgu, sgu = (t.cuda() for t in w4.prepare_gate_up(ws[0][0], ws[1][0], False))
    c3, s3 = (t.cuda() for t in w4.prepare(ws[2][0], False))
    h = ops.expert_gemm_w4_glu(x, cgu, sgu, HG, x.shape[-1], act="silu")
    return ops.expert_gemm_w4(h, c3, s3, None, x.shape[-1], HG)


def _overwrite_with_dequantised(layer, kind, dtype):
    from tutel_amd.experts import w4
    with torch.no_grad():
        for w, km in _weight_params(layer, kind):
            dq = w4.dequantize(*w4.quantize_mxfp4(w, km), dtype)   # [E, N, K]
            w.copy_(dq if km else dq.transpose(1, 2))


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_switch_on_two_calls_the_direct_ops_and_the_dequantised_layer(oracle, spy, monkeypatch, kind, dtype):
    layer, x = _layer(oracle, kind, dtype)
    off = _run(layer, x, False)
    assert not spy.w4 and layer._fp4_weights_ran is None, "switch off: no new call"
    assert spy.counts[PLAIN + "_supported"] == 0 and spy.counts[GLU + "_supported"] == 0
    seen = _record_experts(layer, kind, monkeypatch)
    spy.counts.clear()
    on = _run(layer, x, True)
    assert layer._fp4_weights_ran is True, layer._fp4_weights_ran
    assert spy.w4 == ([(PLAIN, True), (PLAIN, False)] if kind == "ffn" else [(GLU, False), (PLAIN, False)]), spy.w4
    assert not spy.other_gemms(), spy.other_gemms()
    assert len(seen) == 1
    xs, R, slot_map, y = seen[0]
    assert torch.equal(_direct(layer, kind, xs, R, slot_map).view(torch.int16), y.view(torch.int16)), "the ops called directly on the routed rows"
    # a dropless run takes the same two calls
    spy.w4.clear()
    on_dropless = _run(layer, x, True, capacity_factor=0.0)
    assert layer._fp4_weights_ran is True and [n for n, _ in spy.w4] == [PLAIN if kind == "ffn" else GLU, PLAIN], (layer._fp4_weights_ran, spy.w4)
    off_dropless = _run(layer, x, False, capacity_factor=0.0)
    assert layer._fp4_weights_ran is None and len(spy.w4) == 2
    # the same layer over the dequantised weights, on its 16-bit GEMMs
    _overwrite_with_dequantised(layer, kind, dtype)
    for got, cf, what in ((on, None, "capacity factor 1"), (on_dropless, 0.0, "dropless")):
        ref = _run(layer, x, False, **({} if cf is None else dict(capacity_factor=cf)))
        err = (got.double() - ref.double()).abs()
        print(f"\nfp4 weights, {kind}, {dtype}, {what}: against the 16-bit layer over the dequantised weights max abs error "
              f"{float(err.max()):.3e}, bit-equal: {torch.equal(got, ref)}; |y| max {float(ref.abs().max()):.3f}")
        torch.testing.assert_close(got.double(), ref.double(), **_tol(dtype))
    assert bool(torch.isfinite(on.float()).all()) and float(on.abs().max()) > 0 and not torch.equal(on, off)
    assert bool(torch.isfinite(off_dropless.float()).all())


@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_parameter_update_rebuilds_the_image(oracle, spy, kind):
    """an in-place update the autograd version counter sees (an optimizer step, copy_, load_state_dict) rebuilds the images on the
    next forward; a write through `p.data` does not bump that counter -- the KMajorCache's documented rule, for these images as for
    the FP8 ones -- and is followed by invalidate_prepacked()"""
    dtype = torch.bfloat16
    layer, x = _layer(oracle, kind, dtype)
    before = _run(layer, x, True)
    p = layer.experts.batched_fc2_w if kind == "ffn" else layer.experts.W_fc3
    with torch.no_grad():
        p.mul_(2)
    after = _run(layer, x, True)
    assert layer._fp4_weights_ran is True and not torch.equal(after, before), "the cached images were not rebuilt"
    p.data.mul_(2)
    layer.experts.invalidate_prepacked()
    again = _run(layer, x, True)
    assert not torch.equal(again, after)
    _overwrite_with_dequantised(layer, kind, dtype)
    torch.testing.assert_close(again.double(), _run(layer, x, False).double(), **_tol(dtype))


FALLBACKS = {   # name -> (layer kwargs, forward kwargs, run kwargs, a word of the reason)
    "training_mode": ({}, {}, dict(train=True), "training mode"),
    "autocast": ({}, {}, dict(autocast=True), "autocast"),
    "fp8_also_on": ({}, {}, dict(fp8=True), "fp8_weights is on as well"),
    "dropless_megablocks_4": ({}, dict(capacity_factor=0.0, megablocks_size=4), {}, "megablocks"),
    "model_dim_96": (dict(model_dim=96), {}, {}, "shape"),
}


# (SwiGLU experts have no megablocks forward on any path, and their ladders no such rung: the case is the ffn experts' alone)
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind,case", [(k, c) for k in ("ffn", "llama_ffn") for c in FALLBACKS if (k, c) != ("llama_ffn", "dropless_megablocks_4")])
def test_refusals_keep_the_other_forward_bit_for_bit(oracle, spy, kind, case, dtype):
    layer_kw, fwd_kw, run_kw, word = FALLBACKS[case]
    layer, x = _layer(oracle, kind, dtype, **layer_kw)
    run_kw = dict(run_kw)
    if run_kw.pop("train", False):
        layer.train()
    off = _run(layer, x, False, **run_kw, **fwd_kw)   # (fp8_also_on: the FP8 forward alone)
    on = _run(layer, x, True, **run_kw, **fwd_kw)
    assert not spy.w4, "a W4A16 entry point was called"
    assert isinstance(layer._fp4_weights_ran, str) and word in layer._fp4_weights_ran, layer._fp4_weights_ran
    if case == "fp8_also_on":
        assert layer._fp8_weights_ran is True
    assert on.dtype == off.dtype and torch.equal(on, off), "bit-equal to the forward with the FP4 switch off"
    assert bool(torch.isfinite(on.float()).all()) and float(on.abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_graph_capture_replays_the_eager_forward(oracle, spy, kind, dtype):
    from tutel_amd.impls.graph import GraphedForward
    layer, x = _layer(oracle, kind, dtype)
    # nothing cached yet: a forward under stream capture must not quantise, and names the reason
    layer.experts.fp4_weights = True
    assert layer.experts.w4_refusal(x, layer) is None, "admitted outside a capture"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.no_grad():
        with torch.cuda.graph(g, stream=s):
            why = layer.experts.w4_refusal(x, layer)
    torch.cuda.current_stream().wait_stream(s)
    assert why == "the quantised weights are not cached yet: run one eager forward before capturing a graph"
    eager = _run(layer, x, True)
    assert layer._fp4_weights_ran is True and len(spy.w4) == 2
    other = (torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dtype) * 0.5).cuda()
    eager_other = _run(layer, other, True)
    graphed = GraphedForward(layer, x)
    assert layer._fp4_weights_ran is True
    calls = len(spy.w4)
    for _ in range(2):
        assert torch.equal(graphed(other), eager_other), "a replay on the second batch"
        assert torch.equal(graphed(x), eager), "a replay against the eager forward"
    assert len(spy.w4) == calls, "replays make no library call"
