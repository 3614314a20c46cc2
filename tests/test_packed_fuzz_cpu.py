"""The packed-kernel fuzzers (tests/test_packed_fuzz_gpu.py) without a GPU: their references (tests/_packed_fuzz.py) against brute force
on tiny inputs -- a Python loop over entries, rows and columns -- so that a wrong reference cannot agree with a wrong kernel by
construction; their generators alone (every promised edge class drawn at the default length and seed, no drawn case refused by
tutel_amd_packed_plan, every reference layout within the plan's bounds); and what the public packed GEMM refuses, on the host."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _packed_fuzz as F   # noqa: E402
from test_packed_fuzz_gpu import DEFAULT_CASES, SEEDS   # noqa: E402


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _plan(L, T, E, k, limit, align):
    from tutel_amd import _lib
    p = _lib.PackedPlan()
    rc = L.tutel_amd_packed_plan(T, E, k, 128, 128, 128, _lib.BF16, limit, align, ctypes.byref(p))
    assert rc == 0, (T, E, k, limit, align, L.tutel_amd_last_error())
    return p


# ---- references against brute force ---------------------------------------------------------------------------------------------
def _brute_locations(idx, E):
    k, T = idx.shape
    run = [0] * E
    loc = np.zeros([k, T], dtype=np.int32)
    for j in range(k):
        for t in range(T):
            e = int(idx[j, t])
            if 0 <= e < E:
                loc[j, t] = run[e]
                run[e] += 1
    return loc, np.array(run, dtype=np.int32)


def _brute_layout(cnt, idx, loc, E, limit, align, rows_bound):
    k, T = idx.shape
    L = None
    if limit > 0:
        L = limit
        while L % align:
            L += 1
    off, tiles, cap, kept_all = [0], [], 0, []
    for e in range(E):
        kept = int(cnt[e]) if L is None else min(int(cnt[e]), L)
        rows = kept
        while rows % align:
            rows += 1
        r = 0
        while r < rows:
            tiles.append((e, off[e] + r))
            r += 256
        off.append(off[e] + rows)
        cap = max(cap, rows)
        kept_all.append(kept)
    slot = [-1] * rows_bound
    for j in range(k):
        for t in range(T):
            e, l = int(idx[j, t]), int(loc[j, t])
            if 0 <= e < E and l < kept_all[e]:
                slot[off[e] + l] = j * T + t
    return off, cap, tiles, slot


@pytest.mark.parametrize("seed", range(40))
def test_layout_reference_against_brute_force(seed):
    g = np.random.default_rng(seed)
    E = int(g.choice([1, 2, 3, 5, 8]))
    k = int(min(E, g.choice([1, 2, 3])))
    T = int(g.choice([1, 2, 7, 40, 300]))
    align = int(g.choice([1, 2, 4, 8, 128, 256]))
    limit = int(g.choice([0, 1, 2, 5, 37, 290]))
    d = dict(T=T, E=E, k=k, mode=str(g.choice(["random", "skewed", "all_on_k"])), mask_p=float(g.choice([0.0, 0.3])), seed=seed)
    idx = F.make_routing(d)
    for t in range(T):   # k distinct experts per token where not masked
        col = [int(v) for v in idx[:, t] if v >= 0]
        assert len(set(col)) == len(col)
    loc, cnt = F.ref_locations(idx, E)
    bl, bc = _brute_locations(idx, E)
    assert np.array_equal(loc, bl) and np.array_equal(cnt, bc)
    rows_bound = k * T + E * (align - 1) + 5
    ref = F.ref_layout(cnt, idx, loc, E, limit, align, rows_bound)
    off, cap, tiles, slot = _brute_layout(cnt, idx, loc, E, limit, align, rows_bound)
    assert ref["offsets"].tolist() == off and ref["capacity"] == cap and ref["ntiles"] == len(tiles)
    assert [tuple(t) for t in ref["tiles"].tolist()] == tiles and ref["slot"].tolist() == slot
    assert int(ref["keep"].sum()) == sum(1 for s in slot if s >= 0)


def test_rows_routing_gives_the_rows_it_is_asked_for():
    rows = [0, 3, 1, 0, 5]
    for T, k in ((None, 1), (5, 2), (4, 3)):
        idx, loc = F.rows_routing(rows, T, k)
        l2, cnt = F.ref_locations(idx.numpy(), len(rows))
        assert cnt.tolist() == rows and np.array_equal(l2, loc.numpy())
    assert F.offsets_from_rows(rows, 4) == [0, 0, 4, 8, 8, 16]


def _act(name, v):
    if name == "relu":
        return max(v, 0.0)
    if name == "gelu":
        return 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))
    if name == "silu":
        return v / (1.0 + math.exp(-v))
    return v


@pytest.mark.parametrize("kmajor", [True, False])
@pytest.mark.parametrize("act", ["none", "relu", "gelu", "silu"])
def test_gemm_reference_against_brute_force(kmajor, act):
    torch.manual_seed(3)
    dtype = torch.bfloat16
    off = [0, 2, 2, 5]
    E, N, K = 3, 4, 6
    a = torch.randn(7, K).to(dtype)
    w = torch.randn(*([E, N, K] if kmajor else [E, K, N])).to(dtype)
    bias = torch.randn(E, N).to(dtype)
    mul = torch.randn(7, N).to(dtype)
    mul[0, 1] = 0
    for b, m in ((bias, None), (None, mul), (bias, mul)):
        ref = F.ref_gemm(a, w, b, kmajor, act, m, off, dtype)
        assert ref.shape == (5, N)
        for e in range(E):
            for r in range(off[e], off[e + 1]):
                for n in range(N):
                    s = sum(float(a[r, c]) * float(w[e, n, c] if kmajor else w[e, c, n]) for c in range(K))
                    s = _act(act, s + (float(b[e, n]) if b is not None else 0.0)) * (float(m[r, n]) if m is not None else 1.0)
                    assert float(ref[r, n]) == float(torch.tensor(s, dtype=torch.float64).to(dtype)), (e, r, n)


def test_gradient_references_and_bounds_against_brute_force():
    torch.manual_seed(4)
    off = [0, 3, 3, 4]
    a, b = torch.randn(6, 2).to(torch.float16), torch.randn(6, 3).to(torch.float16)
    ref, bnd = F.ref_wgrad(a, b, off)
    dref, mag, n = F.ref_bgrad(b, off)
    assert n.tolist() == [3, 0, 1]
    for e in range(3):
        rows = range(off[e], off[e + 1])
        for j in range(3):
            assert float(dref[e, j]) == pytest.approx(sum(float(b[r, j]) for r in rows), abs=1e-12)
            assert float(mag[e, j]) == pytest.approx(sum(abs(float(b[r, j])) for r in rows), abs=1e-12)
            for i in range(2):
                assert float(ref[e, i, j]) == pytest.approx(sum(float(a[r, i]) * float(b[r, j]) for r in rows), abs=1e-12)
                assert float(bnd[e, i, j]) == pytest.approx(sum(abs(float(a[r, i]) * float(b[r, j])) for r in rows), abs=1e-12)
    assert bool((ref[1] == 0).all()) and bool((dref[1] == 0).all())
    # the bias-gradient bound: the fp32 running sum in row order, rounded once, stays inside it; a lost row does not (700 rows)
    g = torch.Generator().manual_seed(9)
    for dtype in (torch.bfloat16, torch.float16):
        B = torch.randn([700, 64], generator=g).to(dtype)
        s = torch.zeros(64)
        for r in range(700):
            s = s + B[r].float()
        dref, mag, n = F.ref_bgrad(B, [0, 700])
        bound = F.bgrad_bound(dref, mag, n, dtype)
        assert bool(((s.to(dtype).double() - dref[0]).abs() <= bound[0]).all())
        lost = (s - B[0].float()).to(dtype).double()
        assert float(((lost - dref[0]).abs() > bound[0]).double().mean()) > 0.5


def test_decode_and_encode_references_against_brute_force(oracle):
    d = dict(T=9, E=4, k=3, mode="random", mask_p=0.2, seed=11)
    idx = F.make_routing(d)
    loc, cnt = F.ref_locations(idx, 4)
    T, E, k, M, align, limit = 9, 4, 3, 5, 4, 3
    rb = k * T + E * (align - 1)
    ref = F.ref_layout(cnt, idx, loc, E, limit, align, rb)
    assert ref["row_limit"] == 4 and bool(((idx >= 0) & ~ref["keep"]).any())    # the limit really drops entries
    g = torch.Generator().manual_seed(1)
    buf = torch.randn([rb, M], generator=g).to(torch.bfloat16)
    buf[int(ref["offsets"][-1]):] = float("nan")
    gates = torch.rand([k, T], generator=g)
    C = int(ref["kept"].max())
    pad = F.padded_rows(buf, ref["offsets"], ref["kept"], C)
    it, lt = torch.from_numpy(idx), torch.from_numpy(loc)
    crit = (E, [it[j] for j in range(k)], [lt[j] for j in range(k)], [gates[j] for j in range(k)], C, None)
    want = oracle.fast_decode(pad, crit, is_postscore=True)
    x = torch.randn([T, M], generator=g).to(torch.bfloat16)
    for t in range(T):
        acc = np.zeros([M], dtype=np.float32)
        for j in range(k):
            e, l = int(idx[j, t]), int(loc[j, t])
            f = np.zeros([M], dtype=np.float32)
            if e >= 0 and ref["keep"][j, t]:
                f = np.float32(gates[j, t]) * buf[int(ref["offsets"][e]) + l].float().numpy()
            acc = f if j == 0 else acc + f
            gg = float(oracle.gate_grad(x, pad, it[j], lt[j], C)[t])
            if e >= 0 and ref["keep"][j, t]:
                assert gg == pytest.approx(float((x[t].double() * buf[int(ref["offsets"][e]) + l].double()).sum()), abs=1e-5)
            else:
                assert gg == 0.0
        assert torch.equal(torch.from_numpy(acc).to(torch.bfloat16), want[t]), t
    enc = F.ref_encode(x, ref["slot"], gates)
    for r in range(rb):
        q = int(ref["slot"][r])
        row = (np.float32(gates.reshape(-1)[q]) * x[q % T].float().numpy()) if q >= 0 else np.zeros([M], dtype=np.float32)
        assert torch.equal(torch.from_numpy(row).to(torch.bfloat16), enc[r])
    assert torch.equal(F.gathered(x, ref["slot"])[ref["slot"] < 0], torch.zeros([int((ref["slot"] < 0).sum()), M], dtype=torch.bfloat16))


# ---- the generators alone --------------------------------------------------------------------------------------------------------
def test_layout_generator_draws_every_promised_class_inside_the_plan(L):
    seen = set()
    for d in F.gen_layout_cases(DEFAULT_CASES, SEEDS["layout"]):
        assert d["k"] <= min(d["E"], 16) and d["k"] * d["E"] <= 8192 and 1 <= d["T"] <= 20000 and d["align"] in F.LAYOUT_ALIGN
        p = _plan(L, d["T"], d["E"], d["k"], d["limit"], d["align"])
        idx = F.make_routing(d)
        loc, cnt = F.ref_locations(idx, d["E"])
        ref = F.ref_layout(cnt, idx, loc, d["E"], d["limit"], d["align"], p.rows_bound)
        assert int(ref["offsets"][-1]) <= p.rows_bound and ref["ntiles"] <= p.tiles_bound, F.layout_tag(d)
        assert (ref["row_limit"] or 0) == p.row_limit
        seen |= F.layout_classes(d, ref, p.rows_bound, idx)
    F.check_promised("layout", seen, F.LAYOUT_PROMISED, DEFAULT_CASES, DEFAULT_CASES)
    assert [F.layout_tag(d) for d in F.gen_layout_cases(10 * DEFAULT_CASES, SEEDS["layout"])[:DEFAULT_CASES]] == \
        [F.layout_tag(d) for d in F.gen_layout_cases(DEFAULT_CASES, SEEDS["layout"])]      # the long form starts with the default cases


def _rows_case_inside_the_plan(L, d):
    n, E = sum(d["rows"]), d["E"]
    p = _plan(L, max(n, 1), E, 1, 0, d["align"])
    off = F.offsets_from_rows(d["rows"], d["align"])
    tiles = sum(-(-F.round_up(r, d["align"]) // F.TILE) for r in d["rows"])
    assert off[-1] <= p.rows_bound and tiles <= p.tiles_bound and p.rows_bound >= 1 and p.tiles_bound >= 1
    return p, off


def test_gemm_generator_draws_every_promised_class_inside_the_plan(L):
    seen, once = set(), set()
    for d in F.gen_gemm_cases(DEFAULT_CASES, SEEDS["gemm"]):
        _, off = _rows_case_inside_the_plan(L, d)
        assert d["N"] % 8 == 0 and d["N"] >= 8 and d["K"] % 64 == 0 and (d["kmajor"] or (d["act"] in ("none", "relu") and not d["mul"] and not d["gather"]))
        assert off[-1] * d["N"] * d["K"] <= (1 << 31) and d["E"] * d["N"] * d["K"] <= (1 << 25)
        seen |= F.gemm_classes(d)
        if d["kmajor"]:
            once.add(d["E"] * (-(-d["N"] // 256)) >= 256)
    F.check_promised("gemm", seen, F.GEMM_PROMISED, DEFAULT_CASES, DEFAULT_CASES)
    assert once == {True, False}       # both sides of the W_ONCE switch; both sides of the rotation switch: cap<256 / cap>=256 above


def test_grad_generator_draws_every_promised_class_inside_the_plan(L):
    seen = set()
    for d in F.gen_grad_cases(DEFAULT_CASES, SEEDS["grad"]):
        _rows_case_inside_the_plan(L, d)
        assert d["Na"] % 8 == 0 and d["Nb"] % 8 == 0
        seen |= F.grad_classes(d)
    F.check_promised("grad", seen, F.GRAD_PROMISED, DEFAULT_CASES, DEFAULT_CASES)


def test_decode_generator_draws_every_promised_class_inside_the_plan(L):
    seen = set()
    for d in F.gen_decode_cases(DEFAULT_CASES, SEEDS["decode"]):
        assert d["k"] <= min(d["E"], 16)
        p = _plan(L, d["T"], d["E"], d["k"], d["limit"], d["align"])
        idx = F.make_routing(d)
        loc, cnt = F.ref_locations(idx, d["E"])
        ref = F.ref_layout(cnt, idx, loc, d["E"], d["limit"], d["align"], p.rows_bound)
        assert int(ref["offsets"][-1]) <= p.rows_bound and ref["ntiles"] <= p.tiles_bound
        C = max(1, int(ref["kept"].max()))
        M = F.decode_M(d, d["E"], C)
        assert d["E"] * C * M <= (1 << 25)
        seen |= F.decode_classes(d, ref, p.rows_bound, M, idx)
    F.check_promised("decode", seen, F.DEC_PROMISED, DEFAULT_CASES, DEFAULT_CASES)


def test_layer_generator_draws_every_promised_class_inside_the_plan(L):
    from tutel_amd import _lib
    seen = set()
    for d in F.gen_layer_cases(DEFAULT_CASES, SEEDS["layer"]):
        limit, align = F.layer_limit_alignment(d)
        assert d["cf"] == 0 or limit >= 1       # a negative factor really sets a limit
        p = _lib.PackedPlan()
        rc = L.tutel_amd_packed_plan(d["T"], d["E"], d["k"], d["M"], d["H"], d["M"], _lib.BF16 if d["dtype"] == "bf16" else _lib.F16, limit, align,
                                     ctypes.byref(p))
        assert rc == 0, (F.layer_tag(d), L.tutel_amd_last_error())
        assert d["experts"] in ("ffn", "swiglu") and d["act"] in ("relu", "gelu", "silu") and d["T"] in F.LAYER_T + [t // 2 ** i for t in F.LAYER_T for i in range(1, 14)]
        seen |= F.layer_classes(d)
    F.check_promised("layer", seen, F.LAYER_PROMISED, DEFAULT_CASES, DEFAULT_CASES)


# ---- the public packed GEMM on the host: what it refuses, before anything is enqueued -----------------------------------------------
def test_packed_gemm_takes_narrow_n_and_refuses_bad_shapes_before_enqueueing(L):
    """N below 128 is covered (include/tutel_amd.h; the fuzzer draws N from 8): the only refusals are N not a multiple of 8, K not a
    multiple of 64, the n-major restrictions and bad pointers -- each answered on the host with fake pointers, nothing launched"""
    from tutel_amd import _lib
    fake = ctypes.c_void_p(0x10000)   # never dereferenced on the host, and nothing may reach the device

    def call(N=8, K=64, ldd=None, kmajor=1, act=_lib.ACT_NONE, mul=None, offsets=fake, dtype=_lib.BF16, D=fake):
        return L.tutel_amd_expert_gemm_packed(fake, K, None, 0, None, fake, kmajor, N * K, K if kmajor else N, None, 0, mul, D, N if ldd is None else ldd,
                                              4, 64, N, K, dtype, act, offsets, fake, fake, fake, 8, None)
    assert call(N=12, ldd=16) not in (0, _lib.ENOTSUP) and b"multiple of 8" in L.tutel_amd_last_error()
    assert call(N=4, ldd=8) not in (0, _lib.ENOTSUP) and b"multiple of 8" in L.tutel_amd_last_error()
    assert call(K=96) not in (0, _lib.ENOTSUP) and b"multiple of 64" in L.tutel_amd_last_error()
    assert call(N=0) not in (0, _lib.ENOTSUP)
    assert call(offsets=None) not in (0, _lib.ENOTSUP) and b"null" in L.tutel_amd_last_error()
    assert call(D=ctypes.c_void_p(0x10008)) not in (0, _lib.ENOTSUP) and b"aligned" in L.tutel_amd_last_error()
    assert call(kmajor=0, act=_lib.ACT_GELU) == _lib.ENOTSUP and b"n-major" in L.tutel_amd_last_error()
    assert call(kmajor=0, mul=fake) == _lib.ENOTSUP and b"k-major" in L.tutel_amd_last_error()
    assert call(dtype=_lib.F32) == _lib.ENOTSUP and b"16-bit" in L.tutel_amd_last_error()
    # the weight gradient: N_a, N_b from 8 (a loader chunk is 8 columns: wholly inside or outside), other widths refused
    def wgrad(Na, Nb):
        return L.tutel_amd_expert_wgrad_packed(fake, Na, fake, Nb, None, 0, 0, None, fake, 4, 64, Na, Nb, _lib.BF16, None, None)
    assert wgrad(12, 8) == _lib.ENOTSUP and b"multiples of 8" in L.tutel_amd_last_error()
    assert wgrad(8, 8) not in (0, _lib.ENOTSUP) and b"null" in L.tutel_amd_last_error()    # the shape passes; the null offsets do not
