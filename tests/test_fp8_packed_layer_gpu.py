"""FP8 expert weights on the packed dropless forward (layer.dropless_packed_fp8 on top of dropless_packed and experts.fp8_weights;
impls/packed_w8.py), `ffn` and SwiGLU experts, bf16 and fp16: the switched-on forward is six launches -- routing (2), one
tutel_amd_packed_layout, the two W8A16 GEMMs over the packed tables, one tutel_amd_fast_decode_packed -- and none of the one-call
pipelines, 16-bit GEMMs or padded W8 entries; its output, routing and l_aux are the BITS of the padded dropless FP8 forward
(capacity read back to the host); it is captured in a HIP graph and replays for batches of any load; every forward that must stay
what it is without the switch does, bit for bit, with its reason."""
import collections
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL                                     # noqa: E402
from test_swiglu_packed_gpu import make_layer as make_swiglu    # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUT, W8P, GLUP, DECODE = ("tutel_amd_packed_layout", "tutel_amd_expert_gemm_w8_packed", "tutel_amd_expert_gemm_w8_glu_packed",
                             "tutel_amd_fast_decode_packed")
T, M, H, E, K = 300, 256, 256, 8, 2
DTYPES = [torch.bfloat16, torch.float16]
KINDS = ["ffn", "llama_ffn"]
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

    def new_route(self):
        return (self.counts[LAYOUT], self.counts[GLUP], self.counts[W8P], self.counts[DECODE])

    def other_gemms(self):
        """one-call pipelines, 16-bit grouped GEMMs and the padded W8 entries"""
        return {n: c for n, c in self.counts.items()
                if n not in (W8P, GLUP) and (n.startswith("tutel_amd_moe_forward") or
                                             (n.startswith("tutel_amd_expert_gemm") and not n.endswith("_supported")))}


@pytest.fixture
def spy(monkeypatch):
    from tutel_amd import _lib
    s = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", s)
    return s


def _layer(oracle, kind, dtype, hidden=H, cf=0.0, fp32_gate=True, **kw):
    """the layers of tests/test_fp8_weights_layer_gpu.py / test_fp8_weights_llama_layer_gpu.py, dropless"""
    gate = {"fp32_gate": True} if fp32_gate else {}
    if kind == "ffn":
        x, *weights = oracle.make_problem(T, M, hidden, E, dtype=dtype, seed=21)
        layer = TL.make_layer(M, hidden, E, K, cf, dtype, weights, gate=gate, **kw).eval()
    else:
        x, wg, *_ = oracle.make_problem(T, M, hidden, E, dtype=dtype, seed=21)
        g = torch.Generator().manual_seed(77 + hidden)
        w1 = (torch.randn([E, M, hidden], generator=g) / M ** 0.5).to(dtype)
        w2 = (torch.randn([E, M, hidden], generator=g) / M ** 0.5).to(dtype)
        w3 = (torch.randn([E, hidden, M], generator=g) / hidden ** 0.5).to(dtype)
        weights = (wg, w1, w2, w3)
        layer = make_swiglu(M, hidden, E, K, cf, dtype, "top", weights=weights, gate=gate, **kw)
        x = x * 0.5
    for p in layer.parameters():
        p.requires_grad_(False)
    layer._keep_routing = True
    layer.experts.fp8_weights = True
    return layer, x.cuda(), weights


def _run(layer, x, packed_fp8, packed=None, autocast=False, degree=1, **kw):
    """one forward -> (y, l_aux, dispatch_count, last_routing); packed: dropless_packed (by default the new switch's value)"""
    layer.dropless_packed_fp8 = packed_fp8
    layer.dropless_packed = packed_fp8 if packed is None else packed
    layer.last_routing = ()
    with torch.no_grad(), torch.autocast("cuda", dtype=x.dtype, enabled=autocast):
        y = layer(x, a2a_ffn_overlap_degree=degree, **kw)
    return (y.detach().clone(), layer.l_aux.detach().clone(), layer.dispatch_count.clone(), tuple(t.clone() for t in layer.last_routing))


def _same_bits(a, b, what):
    assert a[0].dtype == b[0].dtype and a[0].shape == b[0].shape, what
    assert torch.equal(a[2], b[2]), what + ": dispatch_count"
    assert len(a[3]) == 2 and len(b[3]) == 2 and torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1]), what + ": routing"
    assert torch.equal(a[1].view(-1).view(torch.int32 if a[1].dtype == torch.float32 else torch.int16),
                       b[1].view(-1).view(torch.int32 if b[1].dtype == torch.float32 else torch.int16)), what + ": l_aux"
    ne = (a[0].view(torch.int16) != b[0].view(torch.int16)).nonzero()
    assert ne.numel() == 0, f"{what}: {ne.shape[0]} of {a[0].numel()} output elements differ, the first at {tuple(int(v) for v in ne[0])}"


def _expected_calls(kind):
    return (1, 0, 2, 1) if kind == "ffn" else (1, 1, 1, 1)


# ---- the switch on: the launches, and the bits of the padded FP8 forward -------------------------------------------------------------------
CASES = {   # name -> (capacity_factor, kwargs of the packed run, kwargs of the padded FP8 run)
    "dropless": (0.0, {}, {}),
    "row_limit_drops": (-1.0, {}, {}),
    "alignment_2": (0.0, dict(degree=2), dict(degree=2)),
    # megablocks_size on the packed layout only sets the alignment (4); the padded FP8 forward has that alignment with degree = 4
    "megablocks_4": (0.0, dict(megablocks_size=4), dict(degree=4)),
}


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_switch_on_six_launches_and_the_bits_of_the_padded_fp8_forward(oracle, spy, kind, case, dtype):
    cf, packed_kw, padded_kw = CASES[case]
    layer, x, _ = _layer(oracle, kind, dtype, cf=cf)
    padded = _run(layer, x, False, **padded_kw)
    assert layer._fp8_weights_ran is True and layer._dropless_packed_ran is None, "the padded dropless FP8 forward"
    assert spy.new_route() == (0, 0, 0, 0)
    if case == "row_limit_drops":
        limit = K * int(-cf * ((T + E - 1) // E))
        assert int(padded[2].max()) > limit, "the row limit drops entries in this case"
    spy.counts.clear()
    on = _run(layer, x, True, **packed_kw)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True, (layer._dropless_packed_ran, layer._fp8_weights_ran)
    assert spy.new_route() == _expected_calls(kind), spy.counts
    assert not spy.other_gemms(), spy.other_gemms()
    assert spy.counts["tutel_amd_gate_topk"] == 1 and spy.counts["tutel_amd_compute_location"] == 1, spy.counts
    _same_bits(on, padded, f"{kind} {case}")
    assert bool(torch.isfinite(on[0].float()).all()) and float(on[0].abs().max()) > 0
    # what the packed forward leaves on the layer, as the 16-bit packed forward does
    off = layer.dropless_offsets.cpu()
    assert off.numel() == E + 1 and int(off[0]) == 0 and layer.dropless_capacity.dtype == torch.int32
    assert int(layer.dropless_capacity) == int((off[1:] - off[:-1]).max())
    assert layer.protected_shape[0] == E and layer.protected_shape[2] == M


@pytest.mark.parametrize("kind", KINDS)
def test_a_native_16_bit_gate_projects_once_and_routes_the_same(oracle, spy, kind):
    """without fp32_gate the gate projection is the library's split-K kernel (ops.gate_logits), once, in front of the routing"""
    dtype = torch.bfloat16
    layer, x, _ = _layer(oracle, kind, dtype, fp32_gate=False)
    padded = _run(layer, x, False)
    spy.counts.clear()
    on = _run(layer, x, True)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True
    assert spy.new_route() == _expected_calls(kind) and not spy.other_gemms(), spy.counts
    _same_bits(on, padded, kind + " 16-bit gate")


# ---- graph replay ------------------------------------------------------------------------------------------------------------------------
def _batches(x, wg, dtype):
    """three batches of the same T with different loads (routing replayed on the CPU to make sure): the given one; one skewed so that
    an expert holds more than 256 rows; one that leaves experts empty"""
    wgf = wg.float()

    def counts(b):
        top = (b.float().cpu() @ wgf.t()).topk(K, dim=1).indices
        return torch.bincount(top.reshape(-1), minlength=E)

    g = torch.Generator().manual_seed(9)
    noise = torch.randn(x.shape, generator=g) * 0.25
    skewed = empty = None
    for c in (0.5, 1.0, 2.0, 4.0, 8.0):
        cand = (noise + c * wgf[3] / wgf[3].norm() * M ** 0.5 * 0.25).to(dtype)
        if skewed is None and int(counts(cand).max()) > 256:
            skewed = cand
        cand = (noise + c * (wgf[1] + wgf[6]) / (wgf[1] + wgf[6]).norm() * M ** 0.5 * 0.25).to(dtype)
        if empty is None and int((counts(cand) == 0).sum()) >= 2:
            empty = cand
    assert skewed is not None and empty is not None, "the constructed batches have the loads they are meant to have"
    return [x, skewed.cuda(), empty.cuda()]


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_graph_replays_equal_the_eager_padded_fp8_forward(oracle, spy, kind, dtype):
    """a successful capture is the proof that the route has no host synchronisation"""
    from tutel_amd.impls.graph import GraphedForward
    layer, x, weights = _layer(oracle, kind, dtype)
    batches = _batches(x, weights[0], dtype)
    want = [_run(layer, b, False) for b in batches]
    assert int(want[1][2].max()) > 256, "an expert above 256 rows: two table tiles"
    assert int((want[2][2] == 0).sum()) >= 1, "empty experts"
    eager = _run(layer, x, True)        # one eager forward: it quantises and caches the images
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True
    _same_bits(eager, want[0], "eager")
    layer._keep_routing = False
    spy.counts.clear()
    g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True, "the capture took the new route"
    calls = dict(spy.counts)
    assert spy.counts[W8P] >= 1 and not spy.other_gemms(), spy.other_gemms()
    for _ in range(2):
        for b, w in zip(batches, want):
            y = g(b)
            assert torch.equal(y.view(torch.int16), w[0].view(torch.int16)), "a replay against the eager padded FP8 forward"
    assert dict(spy.counts) == calls, "replays make no library call"


def test_first_use_inside_a_capture_is_refused_with_the_capture_reason(oracle):
    """nothing cached: the admission under stream capture names the reason in _fp8_weights_ran (the forward would be the 16-bit packed
    one) and quantises nothing"""
    layer, x, _ = _layer(oracle, "ffn", torch.bfloat16)
    layer.dropless_packed_fp8 = layer.dropless_packed = True
    gate = layer.gates[0]
    args = (gate, K, 0.0, 1, 1, x.shape[-1:], False, 0, x.dtype)
    logits = torch.empty([T, E], dtype=torch.float32, device="meta")
    with torch.no_grad():
        assert layer._packed_fp8_plan(x, logits, args) is not None, "admitted outside a capture"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    layer._fp8_weights_ran = None
    with torch.cuda.stream(s), torch.no_grad():
        with torch.cuda.graph(g, stream=s):
            plan = layer._packed_fp8_plan(x, logits, args)
    torch.cuda.current_stream().wait_stream(s)
    assert plan is None and isinstance(layer._fp8_weights_ran, str) and "eager forward" in layer._fp8_weights_ran
    assert not layer.experts._kmajor.holds("fc1.w8", layer.experts.batched_fc1_w, "w8")


# ---- refusals: the forward without the switch, bit for bit, with the reason -----------------------------------------------------------------------------
REFUSALS = {   # name -> (layer kwargs, run kwargs, what to set, a word of the reason or None where the switch does not act)
    "switch_off": ({}, {}, dict(dropless_packed_fp8=False), None),
    "fp8_weights_off": ({}, {}, dict(fp8_weights=False), None),
    "training_mode": ({}, dict(train=True), {}, "inference"),
    "autocast": ({}, dict(autocast=True), {}, "one-call native path"),
    "prescore": (dict(is_postscore=False), {}, {}, "is_postscore"),
    "hidden_96": (dict(hidden=96), {}, {}, "multiples of 64"),
}


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("case", list(REFUSALS))
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_keep_the_forward_without_the_switch_bit_for_bit(oracle, spy, kind, case, dtype):
    layer_kw, run_kw, sets, word = REFUSALS[case]
    layer, x, _ = _layer(oracle, kind, dtype, **layer_kw)
    run_kw = dict(run_kw)
    if run_kw.pop("train", False):
        layer.train()
    layer.experts.fp8_weights = sets.get("fp8_weights", True)
    today = _run(layer, x, False, packed=True, **run_kw)      # dropless_packed on, the new switch off: the forward as it is without it
    today_ran = (layer._dropless_packed_ran, layer._fp8_weights_ran)
    assert spy.new_route()[1:3] == (0, 0)
    spy.counts.clear()
    on = _run(layer, x, sets.get("dropless_packed_fp8", True), packed=True, **run_kw)
    assert spy.counts[W8P] == 0 and spy.counts[GLUP] == 0, "a new entry point was called"
    _same_bits(on, today, f"{kind} {case}")
    ran = (layer._dropless_packed_ran, layer._fp8_weights_ran)
    if word is None:
        assert ran == today_ran, "the switch does not act: the reports are those without it"
    else:
        reasons = [r for r in ran if isinstance(r, str)]
        assert any(word in r for r in reasons), (word, ran)
    assert bool(torch.isfinite(on[0].float()).all()) and float(on[0].abs().max()) > 0
