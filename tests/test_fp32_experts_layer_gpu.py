"""fp32 experts on the native fp32 grouped GEMM (switch experts/ffn.py::_NATIVE_FP32, off by default, set here with monkeypatch): the
reference-written fp32 layer fixtures with the switch on, the switch on against off, the gathered against the bucket form, a
recognised activation, every forward that must keep ATen (bit for bit, with its reason), 16-bit layers untouched, graph capture."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL            # noqa: E402

pytestmark = pytest.mark.gpu

ENTRY = "tutel_amd_expert_gemm_f32"
FIXTURES = ["layer_f32_k1_cf1", "layer_f32_k2_cf1", "layer_f32_k2_cf2_prescore", "layer_f32_k2_drop", "layer_f32_k2_dropless",
            "layer_f32_k4_nonorm", "layer_c0_plumbing"]


class Spy:
    """in front of the loaded library (as tests/test_gate_fp32_layer_gpu.py::Spy): counts the calls by name and keeps, per call of the
    fp32 grouped GEMM, whether it gathered (slot_map, argument 21)"""

    def __init__(self, real):
        self._real, self.counts, self.gathered = real, collections.Counter(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args):
            self.counts[name] += 1
            if name == ENTRY:
                self.gathered.append(bool(args[21]))
            return fn(*args)
        return counted


@pytest.fixture
def spy(monkeypatch):
    from tutel_amd import _lib
    s = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", s)
    return s


@pytest.fixture
def matmuls(monkeypatch):
    """the operand ranks of every torch.matmul call"""
    calls, real = [], torch.matmul

    def matmul(a, b, **kw):
        calls.append((a.dim(), b.dim()))
        return real(a, b, **kw)
    monkeypatch.setattr(torch, "matmul", matmul)
    return calls


def _switch(monkeypatch, on):
    from tutel_amd.experts import ffn
    monkeypatch.setattr(ffn, "_NATIVE_FP32", on)


def _bar(y, ref):
    """the project's fp32 bar (test_layer_gpu._close): max |y - ref| / (1e-5 * max(1, |ref|_inf))"""
    y, ref = y.double().cpu(), ref.double().cpu()
    return float((y - ref).abs().max()) / (1e-5 * max(1.0, float(ref.abs().max())))


# ---- the reference's own fixtures ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture_with_the_switch_on(oracle, monkeypatch, spy, matmuls, name):
    """test_layer_gpu.py::test_layer_vs_reference_fixture with the switch on: the reference's routing element by element, y inside the
    project's fp32 bar (the chain's error at K <= 2048 is about 2e-7 * sum |a w|: the ratio to the bar is printed), and the
    expert FFN in exactly two calls of the fp32 grouped GEMM with no batched torch.matmul"""
    z = np.load(os.path.join(TL.GOLD, name + ".npz"))
    T, M, H, E, k, fp32_gate, post, norm, seed = [int(v) for v in z["meta"]]
    dtype, cf = TL.DT[str(z["dtype"][0])], float(z["cf"][0])
    assert dtype == torch.float32
    x, *weights = oracle.make_problem(T, M, H, E, dtype=dtype, seed=seed)
    layer = TL.make_layer(M, H, E, k, cf, dtype, weights, is_postscore=bool(post), normalize_gate=bool(norm),
                          gate={"fp32_gate": bool(fp32_gate)}).eval()
    layer._keep_routing = True
    _switch(monkeypatch, True)
    with torch.no_grad():
        y = layer(x.cuda())
    idx, loc = layer.last_routing
    assert torch.equal(idx.cpu(), torch.from_numpy(z["idx"]).to(torch.int32)), "expert ids"
    assert torch.equal(loc.cpu(), torch.from_numpy(z["loc"]).to(torch.int32)), "slots"
    assert torch.equal(layer.dispatch_count.cpu(), torch.from_numpy(z["dispatch_count"]))
    assert y.dtype == dtype and y.shape == (T, M)
    ref = TL._t(z["y"], dtype)
    print(f"\n{name}: max error / bar = {_bar(y[::int(z['y_row_stride'][0])], ref):.4f}")
    TL._close(y[::int(z["y_row_stride"][0])], ref, dtype)
    assert abs(float(y.l_aux) - float(z["l_aux"][0])) <= 1e-5
    assert spy.counts[ENTRY] == 2, spy.counts
    assert all(a < 3 and b < 3 for a, b in matmuls), matmuls
    assert layer._native_fp32_ran is True
    assert spy.gathered == [bool(post), False], "is_postscore=False takes the bucket form, the others gather fc1's rows from the tokens"


# ---- one small layer, every comparison -----------------------------------------------------------------------------------------
T, M, H, E, K = 300, 64, 64, 8, 2


def _layer(dtype=torch.float32, act=None, hidden=H, cf=1.0, **kw):
    torch.manual_seed(11)
    layer = TL.make_layer(M, hidden, E, K, cf, dtype, **kw).eval()
    with torch.no_grad():   # a wider spread than the reference's init
        layer.experts.batched_fc1_w.normal_(0, M ** -0.5)
        layer.experts.batched_fc2_w.normal_(0, hidden ** -0.5)
    if act is not None:
        layer.experts.activation_fn, layer.experts._act_cache = act, {}
    layer._keep_routing = True
    return layer


def _x(dtype=torch.float32):
    return torch.randn([T, M], generator=torch.Generator().manual_seed(3)).to(dtype).cuda()


def _run(layer, x, grad=False, autocast=False, **kw):
    with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = layer(x, **kw)
    return (y.detach().clone(), layer.l_aux.detach().clone(), layer.dispatch_count.clone(),
            tuple(t.clone() for t in layer.last_routing))


def _same_routing(a, b):
    assert torch.equal(a[2], b[2]) and torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1]), "routing bits"
    assert torch.equal(a[1], b[1]), "l_aux"


def test_switch_on_against_switch_off(monkeypatch, spy, matmuls):
    layer, x = _layer(), _x()
    _switch(monkeypatch, False)
    off = _run(layer, x)
    assert spy.counts[ENTRY] == 0 and layer._native_fp32_ran is None and (3, 3) in matmuls, "the parent's ATen path"
    del matmuls[:]
    _switch(monkeypatch, True)
    on = _run(layer, x)
    assert spy.counts[ENTRY] == 2 and layer._native_fp32_ran is True and all(a < 3 and b < 3 for a, b in matmuls)
    _same_routing(on, off)
    print(f"\nswitch on against off: max error / bar = {_bar(on[0], off[0]):.4f}")
    TL._close(on[0], off[0], torch.float32)
    assert float(on[0].abs().max()) > 0.05


def test_fused_encode_against_the_bucket_form(monkeypatch, spy):
    """the gather is a row copy: _FUSE_ENCODE off (fast_encode + the bucket form) and on (fc1 gathers) give equal output bits"""
    from tutel_amd.impls import moe_layer as ML
    layer, x = _layer(), _x()
    _switch(monkeypatch, True)
    monkeypatch.setattr(ML, "_FUSE_ENCODE", False)
    bucket = _run(layer, x)
    assert spy.gathered == [False, False] and layer._native_fp32_ran is True
    monkeypatch.setattr(ML, "_FUSE_ENCODE", True)
    fused = _run(layer, x)
    assert spy.gathered == [False, False, True, False] and layer._native_fp32_ran is True
    _same_routing(fused, bucket)
    assert torch.equal(fused[0].view(torch.int32), bucket[0].view(torch.int32))


def test_recognised_gelu_layer_runs_natively(monkeypatch, spy):
    layer, x = _layer(act=torch.nn.functional.gelu), _x()
    _switch(monkeypatch, False)
    off = _run(layer, x)
    _switch(monkeypatch, True)
    on = _run(layer, x)
    assert spy.counts[ENTRY] == 2 and layer._native_fp32_ran is True
    _same_routing(on, off)
    TL._close(on[0], off[0], torch.float32)


FALLBACKS = {   # name -> (layer kwargs, forward kwargs, run kwargs, a word of the reason)
    "grad_mode_with_trainable_experts": ({}, {}, dict(grad=True), "autograd"),
    "dropless_megablocks_4": (dict(cf=0.0), dict(megablocks_size=4), {}, "megablocks"),
    "hidden_size_24": (dict(hidden=24), {}, {}, "shape"),
    "unrecognised_activation": (dict(act=lambda t: t.clamp(0, 6)), {}, {}, "activation"),
    "autocast": ({}, {}, dict(autocast=True), "autocast"),
    "float64_layer": (dict(dtype=torch.float64), {}, {}, "fp32"),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_keep_the_aten_path_bit_for_bit(monkeypatch, spy, case):
    layer_kw, fwd_kw, run_kw, word = FALLBACKS[case]
    layer = _layer(**layer_kw)
    x = _x(layer_kw.get("dtype", torch.float32))
    _switch(monkeypatch, False)
    off = _run(layer, x, **run_kw, **fwd_kw)
    _switch(monkeypatch, True)
    on = _run(layer, x, **run_kw, **fwd_kw)
    assert spy.counts[ENTRY] == 0, "the new entry point was called"
    assert isinstance(layer._native_fp32_ran, str) and word in layer._native_fp32_ran, layer._native_fp32_ran
    _same_routing(on, off)
    assert on[0].dtype == off[0].dtype and torch.equal(on[0], off[0]), "bit-equal to switch-off"
    assert bool(torch.isfinite(on[0]).all()) and float(on[0].abs().max()) > 0


def test_bf16_layer_is_untouched(monkeypatch, spy):
    layer, x = _layer(dtype=torch.bfloat16), _x(torch.bfloat16)
    _switch(monkeypatch, False)
    off = _run(layer, x)
    _switch(monkeypatch, True)
    on = _run(layer, x)
    assert spy.counts[ENTRY] == 0 and spy.counts["tutel_amd_expert_gemm_f32_supported"] == 0
    _same_routing(on, off)
    assert torch.equal(on[0], off[0])


def test_graph_capture_replays_the_eager_forward(monkeypatch, spy):
    from tutel_amd.impls.graph import GraphedForward
    layer, x = _layer(cf=1.0), _x()
    layer._keep_routing = False
    _switch(monkeypatch, True)
    with torch.no_grad():
        eager = layer(x).clone()
    assert layer._native_fp32_ran is True and spy.counts[ENTRY] == 2
    other = torch.randn_like(x)
    with torch.no_grad():
        eager_other = layer(other).clone()
    g = GraphedForward(layer, x)
    assert layer._native_fp32_ran is True
    calls = spy.counts[ENTRY]
    for _ in range(3):
        assert torch.equal(g(other), eager_other), "a replay on the second batch"
        assert torch.equal(g(x), eager), "a replay against the eager forward"
    assert spy.counts[ENTRY] == calls, "replays make no library call"
