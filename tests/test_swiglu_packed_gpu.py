"""SwiGLU experts on the packed dropless layout on the MI355X: the fused gate/up GEMM (one launch) against the two launches it
replaces, bit for bit, and against fp32; a llama_ffn layer's packed forward against its padded dropless forward, eager and replayed
from a HIP graph; the refusals; the headline dropless shape against the fp32-accumulating oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = ["silu", "gelu", "relu"]


# ---- the kernel: tutel_amd_expert_gemm_gate_up ---------------------------------------------------------------------------------
def _two_launches(a, wg, wu, act, rc, al):
    from tutel_amd import ops
    g = ops.expert_gemm(a, wg, None, True, act=act, row_counts=rc, row_align=al)
    return ops.expert_gemm(a, wu, None, True, mul=g, row_counts=rc, row_align=al)


def _limits(R, rc, al):
    if rc is None:
        return None
    return [min(R, -(-int(c) // al) * al) for c in rc.cpu()]


def _kernel_operands(E, R, M, H, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = (torch.randn([E, R, M], generator=g, device="cuda") * 0.5).to(dtype)
    wg = (torch.randn([E, H, M], generator=g, device="cuda") / M ** 0.5).to(dtype)
    wu = (torch.randn([E, H, M], generator=g, device="cuda") / M ** 0.5).to(dtype)
    return a, wg, wu


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gate_up_equals_two_launches(dtype, act):
    """R, H and M across the 256-row, 128-feature and 64-deep tile edges; with and without dropless row counts"""
    from tutel_amd import ops
    E = 3
    for R in (1, 100, 256, 300, 1024):
        for H in (128, 384, 2048):
            for M in (256, 2048):
                a, wg, wu = _kernel_operands(E, R, M, H, dtype, R + H + M)
                cases = [(None, 1), (torch.tensor([R, max(R // 3, 1), 0], dtype=torch.int32, device="cuda"), 4)]
                for rc, al in cases:
                    want = _two_launches(a, wg, wu, act, rc, al)
                    got = ops.expert_gemm_gate_up(a, wg, wu, act=act, row_counts=rc, row_align=al)
                    lim = _limits(R, rc, al)
                    for e in range(E):
                        n = R if lim is None else lim[e]
                        assert torch.equal(got[e, :n], want[e, :n]), (R, H, M, e, rc is not None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gate_up_vs_fp32(dtype):
    """against fp32 products (act rounded once, the product rounded once): the bar of
    tests/test_layer_gpu.py::test_llama_expert_fused_glu_gemm_vs_oracle"""
    from tutel_amd import ops
    E, R, M, H = 6, 200, 256, 320
    a, wg, wu = _kernel_operands(E, R, M, H, dtype, 3)
    for act, fn in (("silu", torch.nn.functional.silu), ("gelu", torch.nn.functional.gelu), ("relu", torch.relu)):
        y = ops.expert_gemm_gate_up(a, wg, wu, act=act)
        af = a.double()
        gate = fn(torch.matmul(af, wg.double().transpose(1, 2))).to(dtype).double()
        ref = (gate * torch.matmul(af, wu.double().transpose(1, 2))).to(dtype)
        err = (y.double() - ref.double()).abs().cpu()
        ref = ref.double().cpu()
        if dtype == torch.float16:
            assert float(err.max()) <= 1e-3, float(err.max())
        else:
            assert bool((err <= 2 ** -7 * ref.abs() + 2e-3).all()), float(err.max())


def test_gate_up_refuses_what_it_does_not_cover():
    from tutel_amd import _lib, ops
    a, wg, wu = _kernel_operands(2, 64, 256, 128, torch.bfloat16, 1)
    with pytest.raises(_lib.TutelAmdError, match="relu, gelu or silu"):
        ops.expert_gemm_gate_up(a, wg, wu, act="none")


# ---- the layer ----------------------------------------------------------------------------------------------------------------
def make_layer(M, H, E, k, cf, dtype, gate_type="top", weights=None, act=None, **kw):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        gate = {"type": gate_type, "k": k, "capacity_factor": cf}
        gate.update(kw.pop("gate", {}))
        experts = {"type": "llama_ffn", "num_experts_per_device": E, "hidden_size_per_expert": H}
        if act is not None:
            experts["activation_fn"] = act
        layer = moe.moe_layer(gate_type=gate, experts=experts, model_dim=M, **kw)
    finally:
        torch.set_default_dtype(old)
    g = torch.Generator().manual_seed(E * 31 + H)
    with torch.no_grad():
        if weights is not None:
            wg, w1, w2, w3 = weights
            layer.gates[0].wg.weight.copy_(wg.to(layer.gates[0].wg.weight.dtype))
        else:   # a wider spread than the reference's normal(0, 0.01): outputs well above the dtype's smallest normals
            w1 = torch.randn([E, M, H], generator=g) / M ** 0.5
            w2 = torch.randn([E, M, H], generator=g) / M ** 0.5
            w3 = torch.randn([E, H, M], generator=g) / H ** 0.5
        ex = layer.experts
        ex.W_fc1.copy_(w1.reshape(-1)); ex.W_fc2.copy_(w2.reshape(-1)); ex.W_fc3.copy_(w3.reshape(-1))
    return layer.cuda().eval()


def _forward(layer, x, packed, **kw):
    layer.dropless_packed = packed
    with torch.no_grad():
        y = layer(x, **kw).clone()
    ran = layer._dropless_packed_ran
    cap = layer.dropless_capacity.clone() if packed and ran is True else int(layer.protected_shape[1])
    return y, layer.l_aux.clone(), layer.dispatch_count.clone(), cap, ran


def _same(layer, x, **kw):
    y0, l0, c0, cap0, _ = _forward(layer, x, False, **kw)
    y1, l1, c1, cap1, ran = _forward(layer, x, True, **kw)
    assert ran is True, ran
    assert cap1.dtype == torch.int32 and cap1.is_cuda and int(cap1) == cap0
    assert torch.equal(c0, c1) and torch.equal(l0, l1)
    assert torch.equal(y0, y1), float((y0.float() - y1.float()).abs().max())
    return cap0


@pytest.mark.parametrize("gate_type", ["top", "cosine_top"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_packed_equals_padded_dtypes_gates(dtype, gate_type):
    torch.manual_seed(1)
    layer = make_layer(256, 256, 32, 2, 0.0, dtype, gate_type)
    x = torch.randn(1000, 256, device="cuda", dtype=dtype)
    _same(layer, x)
    _same(layer, x, megablocks_size=4)


# (T, E, k, megablocks, capacity_factor): the cases of tests/test_dropless_packed_gpu.py
CASES = [(1, 8, 1, 0, 0.0), (1, 128, 4, 4, 0.0), (333, 8, 2, 0, 0.0), (333, 128, 1, 4, 0.0), (333, 64, 4, 0, -0.5),
         (700, 16, 2, 4, -1.0), (2000, 128, 2, 0, 0.0), (2000, 8, 4, 4, -0.3), (517, 32, 1, 0, -2.0)]


@pytest.mark.parametrize("gate_type", ["top", "cosine_top"])
@pytest.mark.parametrize("T,E,k,mega,cf", CASES)
def test_packed_equals_padded_shapes(T, E, k, mega, cf, gate_type):
    torch.manual_seed(T * 7 + E + k)
    layer = make_layer(256, 384, E, k, cf, torch.bfloat16, gate_type)
    x = torch.randn(T, 256, device="cuda", dtype=torch.bfloat16)
    _same(layer, x, megablocks_size=mega)
    # every token on the same k experts (identical rows route identically): the largest load there is, most experts empty
    cap = _same(layer, x[:1].expand(T, 256).contiguous(), megablocks_size=mega)
    if cf == 0.0:
        assert cap == -(-T // max(mega, 1)) * max(mega, 1)


def test_graph_replays_packed_swiglu_for_any_load():
    """captured once on the packed layout, replayed for batches whose maximum load differs -- one beyond anything seen while warming
    up or capturing, one with every token on k experts -- each equal to the eager padded forward"""
    from tutel_amd.impls.graph import GraphedForward
    T, M, H, E, k = 1024, 256, 256, 16, 2
    torch.manual_seed(5)
    layer = make_layer(M, H, E, k, 0.0, torch.bfloat16)
    x0 = torch.randn(T, M, device="cuda", dtype=torch.bfloat16)
    g = GraphedForward(layer, x0, capacity_factor=0.0, dropless_packed=True)
    assert layer.dropless_packed is False
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


@pytest.mark.parametrize("case", ["training", "activation", "H=64"])
def test_refusals_raise_and_eager_keeps_todays_result(case):
    from tutel_amd.impls.graph import GraphedForward
    H = 64 if case == "H=64" else 256
    act = (lambda t: torch.clamp(t, -1.0, 1.0)) if case == "activation" else None
    torch.manual_seed(2)
    layer = make_layer(256, H, 8, 2, 0.0, torch.bfloat16, act=act)
    if case == "training":
        layer.train()
    x = torch.randn(256, 256, device="cuda", dtype=torch.bfloat16)
    y0, l0, c0, _, _ = _forward(layer, x, False)
    y1, l1, c1, _, ran = _forward(layer, x, True)
    assert isinstance(ran, str) and ran, ran   # the reason
    assert torch.equal(y0, y1) and torch.equal(l0, l1) and torch.equal(c0, c1)
    with pytest.raises(ValueError, match="packed"):
        GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
    assert layer.dropless_packed is True   # (left as _forward set it: the wrapper restores the layer's own setting)


def test_packed_swiglu_headline_dropless_shape_vs_oracle(oracle):
    """BASELINE configs[2] with SwiGLU experts: T=4096, M=H=2048, E=64, top-2, capacity_factor=0, megablocks 4 -- packed vs the
    fp32-accumulating oracle (the bar of tests/test_dropless_packed_gpu.py::test_packed_headline_dropless_shape_vs_oracle), and bit
    for bit vs the padded layout"""
    T, M, H, E, k = 4096, 2048, 2048, 64, 2
    dtype = torch.bfloat16
    x, wg, *_ = oracle.make_problem(T, M, H, E, dtype=dtype, seed=3)
    # nn.Linear-style init, as oracle.make_problem gives the ffn test: expert outputs of the same size, so that their bf16 rounding
    # (k of them summed in the decode) sits inside the same bar -- with randn / sqrt(fan_in) they reach [1, 2), where one ulp is 2^-7
    g = torch.Generator().manual_seed(7)
    w1 = ((torch.rand([E, M, H], generator=g) * 2 - 1) / M ** 0.5).to(dtype)
    w2 = ((torch.rand([E, M, H], generator=g) * 2 - 1) / M ** 0.5).to(dtype)
    w3 = ((torch.rand([E, H, M], generator=g) * 2 - 1) / H ** 0.5).to(dtype)
    layer = make_layer(M, H, E, k, 0.0, dtype, weights=(wg, w1, w2, w3), gate={"fp32_gate": True})
    xd = x.cuda()
    cap = _same(layer, xd, megablocks_size=4)
    y, _, counts, dcap, _ = _forward(layer, xd, True, megablocks_size=4)
    yo, _, crit, _ = oracle.moe_forward(x, wg, w1, None, w2, None, top_k=k, capacity_factor=0.0, fp32_gate=True,
                                        expert_fn=lambda enc: oracle.expert_llama_ffn(enc, w1, w2, w3, accum_fp32=True))
    assert torch.equal(counts.cpu(), crit[5]) and int(dcap) == cap == (crit[4] + 3) // 4 * 4
    y, yo = y.double().cpu(), yo.double()
    err = (y - yo).abs()
    assert bool((err <= 2 ** -7 * yo.abs() + 2e-3).all()), float(err.max())
