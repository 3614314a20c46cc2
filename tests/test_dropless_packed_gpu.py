"""Dropless forward on the packed layout (csrc/dropless.hip) on the MI355X: the same bits as the padded dropless forward, eager and
replayed from a HIP graph for batches of any expert load, and the headline dropless shape against the fp32-accumulating oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def make_layer(M, H, E, k, cf, dtype, weights=None, **kw):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        gate = {"type": "top", "k": k, "capacity_factor": cf}
        gate.update(kw.pop("gate", {}))
        layer = moe.moe_layer(gate_type=gate,
                              experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H,
                                       "activation_fn": lambda t: torch.nn.functional.relu(t)},
                              model_dim=M, **kw)
    finally:
        torch.set_default_dtype(old)
    if weights is not None:
        wg, w1, b1, w2, b2 = weights
        with torch.no_grad():
            layer.gates[0].wg.weight.copy_(wg.to(layer.gates[0].wg.weight.dtype))
            layer.experts.batched_fc1_w.copy_(w1)
            layer.experts.batched_fc1_bias.copy_(b1)
            layer.experts.batched_fc2_w.copy_(w2)
            layer.experts.batched_fc2_bias.copy_(b2)
    return layer.cuda().eval()


def _forward(layer, x, packed, **kw):
    layer.dropless_packed = packed
    with torch.no_grad():
        y = layer(x, **kw).clone()
    ran = layer._dropless_packed_ran
    cap = layer.dropless_capacity.clone() if packed else int(layer.protected_shape[1])
    return y, layer.l_aux.clone(), layer.dispatch_count.clone(), cap, ran


def _same(layer, x, **kw):
    y0, l0, c0, cap0, _ = _forward(layer, x, False, **kw)
    y1, l1, c1, cap1, ran = _forward(layer, x, True, **kw)
    assert ran is True, ran
    assert cap1.dtype == torch.int32 and cap1.is_cuda and int(cap1) == cap0
    assert torch.equal(c0, c1) and torch.equal(l0, l1)
    assert torch.equal(y0, y1), float((y0.float() - y1.float()).abs().max())
    return cap0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fp32_gate", [False, True])
def test_packed_equals_padded_dtypes(dtype, fp32_gate):
    torch.manual_seed(1)
    layer = make_layer(256, 256, 32, 2, 0.0, dtype, gate={"fp32_gate": fp32_gate})
    x = torch.randn(1000, 256, device="cuda", dtype=dtype)
    _same(layer, x)
    _same(layer, x, megablocks_size=4)


# (T, E, k, megablocks, capacity_factor): E from 8 to 128, T = 1 and T not a multiple of 128, a limit from a negative factor
CASES = [(1, 8, 1, 0, 0.0), (1, 128, 4, 4, 0.0), (333, 8, 2, 0, 0.0), (333, 128, 1, 4, 0.0), (333, 64, 4, 0, -0.5),
         (700, 16, 2, 4, -1.0), (2000, 128, 2, 0, 0.0), (2000, 8, 4, 4, -0.3), (517, 32, 1, 0, -2.0)]


@pytest.mark.parametrize("T,E,k,mega,cf", CASES)
def test_packed_equals_padded_shapes(T, E, k, mega, cf):
    torch.manual_seed(T * 7 + E + k)
    layer = make_layer(256, 384, E, k, cf, torch.bfloat16)
    x = torch.randn(T, 256, device="cuda", dtype=torch.bfloat16)
    _same(layer, x, megablocks_size=mega)
    # every token on the same k experts (identical rows route identically): the largest load there is, most experts empty
    cap = _same(layer, x[:1].expand(T, 256).contiguous(), megablocks_size=mega)
    if cf == 0.0:
        assert cap == -(-T // max(mega, 1)) * max(mega, 1)


def test_graph_replays_packed_for_any_load():
    """captured once on the packed layout, replayed for batches whose maximum load differs -- one beyond anything seen while warming
    up or capturing (the padded path would have had to grow its workspace and run again), one with every token on k experts"""
    from tutel_amd.impls.graph import GraphedForward
    T, M, H, E, k = 1024, 256, 256, 16, 2
    torch.manual_seed(5)
    layer = make_layer(M, H, E, k, 0.0, torch.bfloat16)
    x0 = torch.randn(T, M, device="cuda", dtype=torch.bfloat16)
    g = GraphedForward(layer, x0, capacity_factor=0.0, dropless_packed=True)
    assert layer.dropless_packed is False   # the wrapper's setting does not leak into the layer
    skew = x0.clone()
    skew[: T // 2] = x0[0]
    inputs = [x0, x0 * 3 - 1, skew, x0[:1].expand(T, M).contiguous(), torch.randn(T, M, device="cuda", dtype=torch.bfloat16)]
    want = []
    for x in inputs:
        y, l_aux, _, cap, _ = _forward(layer, x, False, capacity_factor=0.0)
        want.append((y, l_aux, cap))
    caps = [w[2] for w in want]
    assert len(set(caps)) >= 3 and max(caps) == T
    for _ in range(2):
        for x, (y, l_aux, _) in zip(inputs, want):
            out = g(x)
            assert torch.equal(out, y), float((out.float() - y.float()).abs().max())
            assert torch.equal(g.l_aux.reshape(-1), l_aux.reshape(-1))


def test_graphed_forward_packed_refuses_uncovered_shape():
    from tutel_amd.impls.graph import GraphedForward
    layer = make_layer(256, 64, 8, 2, 0.0, torch.bfloat16)   # H = 64: below the packed GEMM's 128 columns
    x = torch.randn(256, 256, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="packed"):
        GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
    with pytest.raises(ValueError):
        GraphedForward(layer, x, capacity_factor=0.0)


def test_packed_headline_dropless_shape_vs_oracle(oracle):
    """BASELINE configs[2]: T=4096, M=H=2048, E=64, top-2, capacity_factor=0, megablocks 4 -- packed vs the fp32-accumulating oracle
    (the tolerance of tests/test_layer_gpu.py::test_dropless_headline_shape_vs_oracle), and bit for bit vs the padded layout"""
    T, M, H, E, k = 4096, 2048, 2048, 64, 2
    dtype = torch.bfloat16
    x, *weights = oracle.make_problem(T, M, H, E, dtype=dtype, seed=3)
    layer = make_layer(M, H, E, k, 0.0, dtype, weights, gate={"fp32_gate": True})
    xd = x.cuda()
    cap = _same(layer, xd, megablocks_size=4)
    y, _, counts, dcap, _ = _forward(layer, xd, True, megablocks_size=4)
    yo, lo, crit, _ = oracle.moe_forward(x, *weights, top_k=k, capacity_factor=0.0, fp32_gate=True, accum_fp32=True)
    assert torch.equal(counts.cpu(), crit[5]) and int(dcap) == cap == (crit[4] + 3) // 4 * 4
    y, yo = y.double().cpu(), yo.double()
    err = (y - yo).abs()
    assert bool((err <= 2 ** -7 * yo.abs() + 2e-3).all()), float(err.max())
