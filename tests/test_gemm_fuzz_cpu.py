"""The gated-GEMM fuzzer (tests/test_gemm_fuzz_gpu.py) without a GPU: its generator alone (deterministic, every promised edge class drawn
at the default length and seed, every drawn case inside the limits the fuzzer states), its float64 reference against a brute-force
triple loop on tiny inputs with both weight layouts and the `ep` permutation written out by index, the condition under which the exact
power-of-two check holds in fp16, and the bound itself: it accepts the reference and rejects one with a single gating element taken
from the neighbouring row."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _gemm_fuzz as F   # noqa: E402
from test_gemm_fuzz_gpu import DEFAULT_CASES, SEED   # noqa: E402

_ACT = {"none": lambda x: x, "relu": lambda x: max(x, 0.0), "gelu": lambda x: 0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0))),
        "silu": lambda x: x / (1.0 + math.exp(-x))}


@pytest.fixture(scope="module")
def cases():
    return F.gen_glu_cases(DEFAULT_CASES, SEED)


def test_generator_is_deterministic_and_draws_every_promised_class(cases):
    assert cases == F.gen_glu_cases(DEFAULT_CASES, SEED)
    assert cases[:40] == F.gen_glu_cases(40, SEED), "the first cases must not depend on how many follow"
    assert cases != F.gen_glu_cases(DEFAULT_CASES, SEED + 1)
    seen = set()
    for d in cases:
        seen |= F.glu_classes(d)
    F.check_promised("glu", seen, F.GLU_PROMISED, DEFAULT_CASES, DEFAULT_CASES)
    with pytest.raises(AssertionError):
        F.check_promised("glu", seen - {"inplace"}, F.GLU_PROMISED, DEFAULT_CASES, DEFAULT_CASES)


def test_every_drawn_case_is_inside_the_stated_limits():
    for d in F.gen_glu_cases(10 * DEFAULT_CASES, SEED):
        tag = F.glu_tag(d)
        assert d["E"] * d["R"] * d["N"] * d["K"] <= F.MAX_WORK, tag
        assert d["E"] in F.GLU_E and d["R"] in F.GLU_R and d["N"] in F.GLU_N and d["K"] in F.GLU_K and d["K"] % 64 == 0 and d["N"] % 8 == 0, tag
        assert d["form"] in F.FORMS and d["act"] in F.GLU_ACT and d["tile"] in F.GLU_TILE and d["store"] in F.GLU_STORE, tag
        assert d["impl"] in F.GLU_IMPL or d["case"] < len(F._HEAD), tag
        if d["form"] == "gate_up":
            assert d["kmajor"] and not d["bias"] and d["act"] != "none" and d["layout"] == "contig", tag
        assert (d["layout"] == "ep") == (d["W"] in (2, 4)) and (d["W"] == 0 or d["R"] % d["W"] == 0), tag
        assert not d["inplace"] or d["form"] in F.GATED, tag
        assert d["row_align"] in (1, 4, 32), tag
        if d["row_counts"] is not None:
            c = d["row_counts"]
            assert len(c) == d["E"] and all(0 <= v <= d["R"] for v in c), tag
            assert (0 in c and d["R"] in c) if d["E"] > 1 else c[0] in (0, d["R"]), tag
            assert all(0 <= lim <= d["R"] and lim >= v for lim, v in zip(F.row_limits(d), c)), tag
        else:
            assert F.row_limits(d) == [d["R"]] * d["E"], tag
        if d["form"] == "mul_pow2" and d["dtype"] == "f16":
            assert d["act"] != "relu", tag


def _brute(a, w, bias, kmajor, act, G, dtype):
    E, R, K = a.shape
    N = w.shape[1] if kmajor else w.shape[2]
    ref = torch.zeros([E, R, N], dtype=torch.float64)
    v = torch.zeros([E, R, N], dtype=torch.float64)
    for e in range(E):
        for r in range(R):
            for n in range(N):
                s = math.fsum(float(a[e, r, k]) * float(w[e, n, k] if kmajor else w[e, k, n]) for k in range(K))
                if bias is not None:
                    s += float(bias[e, n])
                s = _ACT[act](s)
                v[e, r, n] = s
                ref[e, r, n] = s * float(G[e, r, n]) if G is not None else s
    return ref.to(dtype).double(), v


@pytest.mark.parametrize("kmajor,act,with_bias,gate,dtype", [
    (True, "none", False, "none", torch.bfloat16), (False, "relu", True, "random", torch.float16), (True, "gelu", True, "random", torch.bfloat16),
    (False, "silu", False, "pow2", torch.float16), (True, "relu", True, "mask", torch.bfloat16), (False, "none", True, "pow2", torch.bfloat16)])
def test_ref_glu_equals_a_triple_loop(kmajor, act, with_bias, gate, dtype):
    E, R, N, K = 2, 4, 6, 5
    g = torch.Generator().manual_seed(N * 100 + len(act) + int(kmajor))
    a = torch.randn([E, R, K], generator=g).to(dtype)
    w = (torch.rand([E, N, K] if kmajor else [E, K, N], generator=g) * 2 - 1).to(dtype)
    bias = torch.randn([E, N], generator=g).to(dtype) if with_bias else None
    G = {"none": None, "random": torch.randn([E, R, N], generator=g).to(dtype), "pow2": F.pow2_gate(E, R, N).to(dtype),
         "mask": (torch.rand([E, R, N], generator=g) < 0.5).to(dtype)}[gate]
    ref, v = F.ref_glu(a, w, bias, kmajor, act, G, dtype)
    bref, bv = _brute(a, w, bias, kmajor, act, G, dtype)
    torch.testing.assert_close(v, bv, rtol=1e-13, atol=1e-14)
    # rounded once to the dtype: the same value except where the two float64 sums straddle a rounding boundary (none at these sizes)
    assert torch.equal(ref, bref)
    if act != "none" and kmajor:     # the fused gate/up form: the gate rounded to the dtype, then ONE rounding of gate * up
        gate_r = F.ref_gate(a, w, act, dtype)
        _, bg = _brute(a, w, None, True, act, None, dtype)
        assert torch.equal(gate_r.double(), bg.to(dtype).double())
        w_up = (torch.rand([E, N, K], generator=g) * 2 - 1).to(dtype)
        got, up = F.ref_glu(a, w_up, None, True, "none", gate_r, dtype)
        _, bup = _brute(a, w_up, None, True, "none", None, dtype)
        torch.testing.assert_close(up, bup, rtol=1e-13, atol=1e-14)
        assert torch.equal(got, (up * gate_r.double()).to(dtype).double())


def test_ep_permutation_by_index():
    E, W, C, X = 3, 4, 5, 2
    t = torch.arange(E * W * C * X, dtype=torch.float32).view(E, W * C, X)
    p = F.to_ep(t, W, gap=1, fill=-1.0)
    assert list(p.shape) == [W, E, C + 1, X]
    for w in range(W):
        for e in range(E):
            for c in range(C):
                assert torch.equal(p[w, e, c], t[e, w * C + c])
            assert bool((p[w, e, C] == -1.0).all())
    back, gap = F.from_ep(p, W, gap=1)
    assert torch.equal(back, t) and list(gap.shape) == [W, E, 1, X] and bool((gap == -1.0).all())
    assert torch.equal(F.from_ep(F.to_ep(t, W), W)[0], t)
    # the (stride_e, stride_w, rows_per_w, ld) the launch is given address exactly these elements
    d = dict(W=W, E=E, R=W * C, N=8, K=64)
    (ase, asw, arpw, lda), (dse, dsw, drpw, ldd) = F.ep_layouts(d)
    A = torch.arange(W * E * C * 64).view(W, E, C, 64)
    D = torch.arange(W * E * (C + 1) * 8).view(W, E, C + 1, 8)
    for e in range(E):
        for r in range(W * C):
            assert int(A.reshape(-1)[e * ase + (r // arpw) * asw + (r % arpw) * lda]) == int(A[r // C, e, r % C, 0])
            assert int(D.reshape(-1)[e * dse + (r // drpw) * dsw + (r % drpw) * ldd]) == int(D[r // C, e, r % C, 0])


def test_pow2_gate_differs_between_neighbours_and_is_exact_in_both_dtypes():
    G = F.pow2_gate(3, 9, 16)
    assert bool((G[:, 1:] != G[:, :-1]).all()) and bool((G[:, :, 1:] != G[:, :, :-1]).all())
    assert set(G.abs().unique().tolist()) == {1.0, 2.0, 4.0}
    assert float(G[1, 2, 3]) == -(2.0 ** ((1 + 6 + 15) % 3))
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(G.to(dt).double(), G)


def test_fp16_pow2_cases_leave_out_at_most_the_cap(cases):
    """the condition of the fuzzer's exact check: where |v| >= 2^-13 an fp16 result times 1, 2 or 4 is a normal number, so rounding
    commutes with the product; the share of a case below that is capped at 0.2 % (expected: about 0.03 %)"""
    n = 0
    # every default-length case, and the small ones of the full-length list: where one element is more than the cap the generator redraws
    small = [d for d in F.gen_glu_cases(10 * DEFAULT_CASES, SEED)[DEFAULT_CASES:] if d["E"] * d["R"] * d["N"] < 1000]
    assert any(d["form"] == "mul_pow2" and d["dtype"] == "f16" for d in small)
    for d in cases + small:
        if d["form"] == "mul_pow2" and d["dtype"] == "f16":
            a, w, bias, G, _ = F.make_glu_inputs(d)
            _, v = F.ref_glu(a, w, bias, d["kmajor"], d["act"], G, torch.float16)
            share = float(F.pow2_left_out(v, torch.float16).double().mean())
            assert share <= F.POW2_LEFT_OUT_CAP, (F.glu_tag(d), share)
            if v.numel() >= 1000:    # the scaling the 0.03 % rests on: the product's standard deviation is 0.58 (gelu / silu of it: from 0.3)
                assert float(v.std()) >= (0.25 if d["act"] != "none" else 0.55), F.glu_tag(d)
            n += 1
    assert n >= 3
    assert not bool(F.pow2_left_out(torch.zeros([4]), torch.bfloat16).any())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gate", ["random", "pow2"])
def test_bound_accepts_the_reference_and_rejects_a_gate_from_the_next_row(dtype, gate):
    E, R, N, K = 2, 9, 16, 64
    g = torch.Generator().manual_seed(5)
    a = torch.randn([E, R, K], generator=g).to(dtype)
    w = ((torch.rand([E, N, K], generator=g) * 2 - 1) / math.sqrt(K)).to(dtype)
    G = (F.pow2_gate(E, R, N) if gate == "pow2" else torch.randn([E, R, N], generator=g)).to(dtype)
    ref, v = F.ref_glu(a, w, None, True, "none", G, dtype)
    bound = F.glu_bound(ref, G, dtype)
    assert bool(((ref - ref).abs() <= bound).all()) and bool((bound > 0).all())
    # one element gated by the value of the row below it: that element, and no other, is beyond the bound
    score = v[:, :-1].abs() * (G.double()[:, 1:] - G.double()[:, :-1]).abs()
    e, r, n = [int(i) for i in (score == score.max()).nonzero()[0]]
    G2 = G.clone()
    G2[e, r, n] = G[e, r + 1, n]
    wrong, _ = F.ref_glu(a, w, None, True, "none", G2, dtype)
    over = (wrong - ref).abs() > bound
    assert bool(over[e, r, n]) and int(over.sum()) == 1
    # and with the pow2 pattern every element of usual magnitude is, for the gate of the row above (the sign differs) as for the gate of
    # the column to the left (sign and magnitude differ)
    if gate == "pow2":
        for dim in (1, 2):
            shifted, _ = F.ref_glu(a, w, None, True, "none", torch.roll(G, 1, dim), dtype)
            far = (shifted - ref).abs() > bound
            assert bool((far[:, 1:, 1:])[v[:, 1:, 1:].abs() >= 0.05].all())
    assert bool((F.glu_bound(ref, None, dtype) <= bound).all())
