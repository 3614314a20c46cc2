"""The packed-kernel fuzzers (tests/test_packed_fuzz_gpu.py) without a GPU: their references (tests/_packed_fuzz.py) against brute force
on tiny inputs -- a Python loop over entries, rows and columns -- so that a wrong reference cannot agree with a wrong kernel by
construction; their generators alone (every promised edge class drawn at the default length and seed, no drawn case refused by
tutel_amd_packed_plan, every reference layout within the plan's bounds); the generator of the training forms
(tests/test_packed_train_forms_gpu.py), the guard bands (a simulated over-read gives NaN, a simulated over-write trips moat_intact, and
neither shows without the band) and the row-sampled GEMM reference; and what the public packed GEMM refuses, on the host."""
import ctypes
import hashlib
import json
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


# ---- the training forms: generator, guard bands, row sampling (tests/test_packed_train_forms_gpu.py) ---------------------------------
def _digest(cases):
    return hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()


def test_the_older_generators_draw_the_cases_they_drew_before_the_training_forms():
    """digests of the case dicts (json, sorted keys) computed on the commit before gen_train_form_cases existed"""
    assert _digest(F.gen_gemm_cases(DEFAULT_CASES, SEEDS["gemm"])) == "89214435fbfce59e39284d6b83652b3df51ac7cb302c713d0112db612b2a3dc7"
    assert _digest(F.gen_gemm_cases(10 * DEFAULT_CASES, SEEDS["gemm"])) == "5c6a68b5459ffdad9363b83ee7ee80d00054a863ebae0f9f383f539fb58a6a78"
    assert _digest(F.gen_grad_cases(DEFAULT_CASES, SEEDS["grad"])) == "e438d5f66d03dbb842ab06df2426505e1e9b773500fb712ad2f1e5beff162573"
    assert _digest(F.gen_grad_cases(10 * DEFAULT_CASES, SEEDS["grad"])) == "fc600d723c87e6f64cd7c48cb72106565a6d3b0f6caf17c32fc694a6d5181b90"


def _train_ref(L, d):
    idx = F.train_routing(d)
    T, E, k = d["T"], d["E"], d["k"]
    assert idx.shape == (k, T) and k in (1, 2, 3, 4) and k <= E and d["align"] in F.TRAIN_ALIGN
    live = idx >= 0
    srt = np.sort(np.where(live, idx, -1 - np.arange(k)[:, None]), axis=0)
    assert bool((srt[1:] != srt[:-1]).all()) and int(idx.max()) < E, "a token chooses an expert twice"
    p = _plan(L, T, E, k, 0, d["align"])
    loc, cnt = F.ref_locations(idx, E)
    ref = F.ref_layout(cnt, idx, loc, E, 0, d["align"], p.rows_bound)
    assert int(ref["offsets"][-1]) <= p.rows_bound and ref["ntiles"] <= p.tiles_bound, F.train_tag(d)
    return ref, p


def test_train_form_generator_draws_every_promised_class_within_its_memory_bounds(L):
    from test_packed_train_forms_gpu import DEFAULT_CASES as N_TRAIN, SEED
    long = F.gen_train_form_cases(10 * N_TRAIN, SEED)
    assert long[:N_TRAIN] == F.gen_train_form_cases(N_TRAIN, SEED) and long[:7] == F.gen_train_form_cases(7, SEED)     # case i does not depend on n
    assert F.gen_gemm_cases(5, SEEDS["gemm"]) == F.gen_gemm_cases(DEFAULT_CASES, SEEDS["gemm"])[:5]
    seen = set()
    for d in long:
        ref, p = _train_ref(L, d)
        used = int(ref["offsets"][-1])
        assert used > 0, F.train_tag(d)
        assert d["T"] in F.TRAIN_T or d["mode"] == "all3"
        assert d["T"] == 1 or F.free_token(ref["slot"], d["T"]) is not None, "no token left for the slot map's band to name"
        if d["kind"] == "wgrad":
            assert d["Na"] in F.WG_N and d["Nb"] in F.WG_N and d["E"] * d["Na"] * d["Nb"] <= (1 << 23)
            assert used * d["Na"] * d["Nb"] <= 2 * F.F64_BUDGET, F.train_tag(d)
        else:
            assert d["N"] % 8 == 0 and d["K"] % 64 == 0 and d["E"] * d["N"] * d["K"] <= (1 << 25)          # weights below 64 MiB
            assert p.rows_bound * max(d["N"], d["K"]) * 2 <= (1 << 28), F.train_tag(d)                      # no operand above 256 MiB
            assert (d["act"], d["bias"]) == ("none", False) or d["kind"] == "nmajor"
            rows = F.tile_sample_rows(ref["tiles"], ref["offsets"], d["seed"])
            assert min(used, rows.size) * d["N"] * d["K"] <= 2 * F.F64_BUDGET
        if d["case"] < N_TRAIN:
            seen |= F.train_classes(d, ref)
    F.check_promised("train forms", seen, F.TRAIN_PROMISED, N_TRAIN, N_TRAIN)


def test_the_two_fixed_cases_and_their_float64_sample(L):
    """K = N = 2048 over 96 tile-table entries from 3 experts of 8192 rows, n-major gathered and k-major; the sampled rows hold the
    first and the last row of every tile"""
    from test_packed_train_forms_gpu import SEED
    for d, kind in zip(F.gen_train_form_cases(2, SEED), ("nmajor", "pp")):
        ref, _ = _train_ref(L, d)
        assert d["kind"] == kind and d["gather"] and (d["N"], d["K"]) == (2048, 2048) and d["act"] == "none"
        assert ref["rows"].tolist() == [8192] * 3 and ref["ntiles"] == 96 and int(ref["slot"].max()) >= 2 * d["T"]
        assert bool((np.diff(ref["slot"][:8192] % d["T"]) < 0).any()), "an expert's token rows are read in ascending order"
        assert 24576 * 2048 * 2048 > F.F64_BUDGET                                 # so the runner samples
        rows = set(F.tile_sample_rows(ref["tiles"], ref["offsets"], d["seed"]).tolist())
        assert len(rows) >= 3 * 96
        for t in range(96):
            assert 256 * t in rows and 256 * t + 255 in rows
    # a ragged layout: the last row of a tile is the expert's last row, not the tile's 256th
    off = [0, 300, 300, 301]
    rows = F.tile_sample_rows([(0, 0), (0, 256), (2, 300)], off, 5).tolist()
    assert {0, 255, 256, 299, 300} <= set(rows) and max(rows) == 300


@pytest.mark.parametrize("seed", range(200))
def test_row_sampled_gemm_reference_equals_the_full_one(seed):
    g = np.random.default_rng(1000 + seed)
    E = int(g.choice([1, 2, 3, 5]))
    cnt = g.choice([0, 1, 2, 5, 9], size=E)
    off = np.concatenate([[0], np.cumsum(cnt)])
    used = int(off[-1])
    if used == 0:
        cnt[0], off, used = 3, off + 3, 3
        off[0] = 0
    N, K = int(g.choice([1, 4, 7])), int(g.choice([2, 6]))
    kmajor, act = bool(g.integers(2)), str(g.choice(["none", "relu", "gelu", "silu"]))
    dtype = [torch.bfloat16, torch.float16][int(g.integers(2))]
    tg = torch.Generator().manual_seed(seed)
    a = torch.randn([used + 2, K], generator=tg).to(dtype)
    w = torch.randn([E, N, K] if kmajor else [E, K, N], generator=tg).to(dtype)
    bias = torch.randn([E, N], generator=tg).to(dtype) if g.integers(2) else None
    mul = torch.randn([used + 2, N], generator=tg).to(dtype) if g.integers(2) else None
    full = F.ref_gemm(a, w, bias, kmajor, act, mul, off, dtype)
    rows = np.unique(g.integers(0, used, size=int(g.integers(1, used + 2))))
    want, exact, mag = F.ref_gemm_rows(a, w, bias, kmajor, act, mul, off, dtype, rows)
    assert torch.equal(want, full[torch.from_numpy(rows)])
    assert torch.equal(exact.to(dtype).double(), want) and bool((mag >= 0).all())
    if act == "none" and mul is None:
        assert bool((exact.abs() <= mag * (1 + 1e-12) + 1e-300).all())


def _raw(view):
    """the whole buffer of a moated view, and the view's first element in it"""
    buf, band, _ = view._moat
    return buf, band


def _sim_gather(xv, slot_v, rows, over_row=0, over_slot=0):
    """a gather as the kernels do it, on the moated buffers themselves: packed row r reads slot entry r + over_slot and token row
    q % T + over_row -- addressed from the view's first element, so that an index past the view lands in the band"""
    (xb, x0), (sb, s0) = _raw(xv), _raw(slot_v)
    T, K = xv.shape
    out = torch.zeros([rows, K], dtype=xv.dtype)
    for r in range(rows):
        q = int(sb[s0 + r + over_slot])
        if q >= 0:
            t = q % T + over_row
            out[r] = xb[x0 + t * K:x0 + (t + 1) * K]
    return out


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, [5, 8]), (torch.float16, [1, 2048]), (torch.float32, [3, 136, 8]), (torch.int32, [7]),
                                         (torch.bfloat16, [3, 4]), (torch.bfloat16, [64])])
def test_moated_view_is_aligned_contiguous_and_banded(dtype, shape):
    n = int(np.prod(shape))
    t = (torch.arange(n) % 100).reshape(shape).to(dtype)
    v = F.moated(t)
    buf, band = _raw(v)
    es = t.element_size()
    assert v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous() and torch.equal(v, t)
    assert v.data_ptr() % 16 == 0 and (v.data_ptr() - buf.data_ptr()) == band * es and buf.numel() == 2 * band + n
    width = n // shape[0] if len(shape) > 1 else 1
    assert band * es >= 4096 and band >= 64 * width and (band * es) % 16 == 0
    assert F.moated(t, rows=200)._moat[1] >= 200 * width
    edge = torch.cat([buf[:band], buf[band + n:]])
    assert bool(torch.isnan(edge).all()) if dtype.is_floating_point else bool((edge == F.SENTINEL).all())
    F.moat_intact(v)
    assert bool((F.moated(t, fill=3)._moat[0][:band] == 3).all())


def test_guard_bands_turn_an_overread_into_nan_and_an_overwrite_into_a_failure():
    """the harness's own mutation test: each simulated off-by-one is caught WITH the band, and would pass unseen without it"""
    T, K, k = 6, 8, 2
    g = torch.Generator().manual_seed(2)
    x = torch.randn([T, K], generator=g).to(torch.bfloat16)
    slot = np.array([7, 0, -1, 11, 8, 2, 10, 4, -1, -1], dtype=np.int64)     # live rows name tokens 1, 0, 5, 2, 2, 4, 4 of k T = 12 entries
    free = F.free_token(slot, T)
    assert free == 3
    x[free] = float("nan")
    used = 8
    xv = F.moated(x)
    sv = F.moated(torch.from_numpy(slot).int(), fill=free)
    want = F.gathered(x, slot[:used])
    assert not bool(torch.isnan(want).any())
    assert torch.equal(_sim_gather(xv, sv, used), want)
    # (1) one token row past the array: the last token's neighbour is the band
    assert bool(torch.isnan(_sim_gather(xv, sv, used, over_row=1)[3]).all())      # row 3 names token T - 1
    # (2) one slot-map entry past its end: the band's entry names the NaN token
    assert bool(torch.isnan(_sim_gather(xv, sv, len(slot), over_slot=1)[-1]).all())
    # without the bands: the same reads inside one shared buffer return somebody else's finite values, and nothing is NaN
    pool = torch.cat([x.clone().nan_to_num_(0.5).view(-1), torch.ones([4 * K], dtype=x.dtype)])
    bare = pool[:T * K].view(T, K)
    bare._moat = (pool, 0, 0)
    spool = torch.cat([torch.from_numpy(slot).int(), torch.zeros([4], dtype=torch.int32)])
    sbare = spool[:len(slot)]
    sbare._moat = (spool, 0, 0)
    assert not bool(torch.isnan(_sim_gather(bare, sbare, used, over_row=1)).any())
    assert not bool(torch.isnan(_sim_gather(bare, sbare, len(slot), over_slot=1)).any())
    # (3) a store one row past the output (and one before it) trips moat_intact; a store inside does not
    for dtype in (torch.bfloat16, torch.float32):
        o = F.moated(torch.full([4, K], 3.0, dtype=dtype), fill=F.OUT_FILL)
        buf, band = _raw(o)
        o[3] = 1.0
        F.moat_intact(o)
        buf[band + 4 * K:band + 5 * K] = 1.0
        with pytest.raises(AssertionError, match="after"):
            F.moat_intact(o)
        o = F.moated(torch.full([4, K], 3.0, dtype=dtype), fill=F.OUT_FILL)
        o._moat[0][band - 1] = 1.0
        with pytest.raises(AssertionError, match="before"):
            F.moat_intact(o)
    n = F.moated(torch.zeros([4], dtype=torch.float16))       # a NaN band is compared by its bits: NaN != NaN does not fool it
    F.moat_intact(n)
    n._moat[0][0] = 0.0
    with pytest.raises(AssertionError):
        F.moat_intact(n)


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
