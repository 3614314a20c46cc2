"""Seeded fuzzer of the packed kernels in the forms a SwiGLU training step on the packed layout relies on ("not shipped"):
the n-major packed GEMM with its rows gathered through the slot map, the k-major ping-pong kernel as a plain product (no activation,
no bias) on both sides of its weights-streamed-once switch, and the weight / bias gradient with gathered operands at N_a, N_b up to
2048 -- every launch already in the library, reached through `ops`, over layouts of real routings (k in {1, 2, 4} distinct choices per
token, a share masked, alignment 1 / 8 / 128, T up to 4096: a permuted slot map with values up to k T - 1).

Every operand sits in a guard band (tests/_packed_fuzz.py::moated): NaN around the inputs, a sentinel around the outputs the caller
allocates, a valid entry naming a NaN token row around the slot map.  A read next to an operand shows as a NaN in a failing
comparison and a store next to an output as a changed band -- at shapes far too small to walk off mapped memory.
  gemm   against float64 on the same rounded inputs (all rows, or the first, last and two random rows of every tile above
         F.F64_BUDGET), the n-major form also within one rounding of an fp32 sum; every gathered launch bit for bit equal to the same
         launch on a materialised packed copy of the tokens (pad rows zeros, rows past offsets[E] NaN)
  grad   the 16-bit form within F.wgrad_bound / F.bgrad_bound, the fp32 form within the bounds of tests/test_packed_amp_gpu.py, the
         accumulating form D + G bit for bit (tests/test_packed_main_grad_gpu.py); gathered against materialised bit for bit
  all    rows at or past offsets[E] keep their pre-fill, every band intact, a second call the same bits, the output not all zero
The default run takes 60 cases, --runslow 600; `python tests/test_packed_train_forms_gpu.py [cases] [seed]` runs any length."""
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _packed_fuzz as F   # noqa: E402
from test_packed_fuzz_gpu import _check_layout, _fail, _first_violation, _gemm_tol, _plan, _sentinel_layout   # noqa: E402

DEFAULT_CASES = 60
SEED = 7075
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(F._INT_VIEW[t.element_size()])


def routing_layout(d):
    """the case's layout from the library (compute_location, packed_layout) checked against the integer reference, its slot map rebound
    to a moated copy whose band names the token row nobody reads -> (layout, reference, rows_bound, that token or None)"""
    from tutel_amd import ops
    T, E, k = d["T"], d["E"], d["k"]
    idx = F.train_routing(d)
    idx_d = torch.from_numpy(idx).cuda()
    loc_d, cnt_d, _, _, _ = ops.compute_location(idx_d, E)
    loc, cnt = loc_d.cpu().numpy(), cnt_d.cpu().numpy()
    loc_r, cnt_r = F.ref_locations(idx, E)
    assert np.array_equal(cnt, cnt_r) and np.array_equal(loc, loc_r), "compute_location differs from the stable rank"
    plan = _plan(T, E, k, 0, d["align"])
    ref = F.ref_layout(cnt, idx, loc, E, 0, d["align"], plan["rows_bound"])
    lay = _sentinel_layout(E, plan)
    ops.packed_layout(cnt_d, idx_d, loc_d, 0, d["align"], plan["rows_bound"], plan["tiles_bound"], plan["row_limit"], out=lay)
    _check_layout(lay, ref, plan, idx, loc, T)
    free = F.free_token(ref["slot"], T)
    # the band of an index table holds an index: the free token (its row is NaN), or token 0 where every token is read
    lay.slot_map = F.moated(lay.slot_map, fill=free if free is not None else 0)
    return lay, ref, plan["rows_bound"], free


def _tokens(g, T, N, dtype, free):
    x = torch.randn([T, N], generator=g).to(dtype)
    if free is not None:
        x[free] = NAN
    return x


def _packed_copy(rows, rb, used):
    """[rb, N] on the host: the live rows (pad rows as given: zeros), NaN from offsets[E] on"""
    t = torch.full([rb, rows.shape[1]], NAN, dtype=rows.dtype)
    t[:used] = rows[:used]
    return t


def run_gemm_case(d, lay, ref, rb, free, stats):
    from tutel_amd import ops
    dtype = F.DTYPES[d["dtype"]]
    E, N, K, T = d["E"], d["N"], d["K"], d["T"]
    kmajor = d["kind"] == "pp"
    off, used = ref["offsets"], int(ref["offsets"][-1])
    assert used > 0, "the case has no live row"
    g = torch.Generator().manual_seed(d["seed"])
    # the k-major product reads the array as the backward of weights kept "as stored" does: storage [E, K', N'], K' = N and N' = K
    w = ((torch.rand([E, N, K] if kmajor else [E, K, N], generator=g) * 2 - 1) / math.sqrt(K)).to(dtype)
    bias = torch.randn([E, N], generator=g).to(dtype) if d["bias"] else None
    mul = None
    if d["mul"]:
        mul = torch.randn([rb, N], generator=g)
        mul[torch.rand([rb, N], generator=g) < 0.25] = 0
        mul = mul.to(dtype)
    slot = ref["slot"][:used]
    if d["gather"]:
        x = _tokens(g, T, K, dtype, free)
        a_rows = F.gathered(x, slot)
        xd = F.moated(x, device="cuda")
        zero = F.moated(torch.zeros([max(K, 8)], dtype=dtype), device="cuda")
    else:
        a_rows = torch.randn([used, K], generator=g).to(dtype)
        xd = zero = None
    assert not bool(torch.isnan(a_rows).any()), "the reference itself reads the NaN token"
    xpd = F.moated(_packed_copy(a_rows, rb, used), device="cuda")
    wd = F.moated(w, device="cuda")
    bd = F.moated(bias, device="cuda") if bias is not None else None
    md = F.moated(mul, device="cuda") if mul is not None else None

    def run(gather):
        o = F.moated(torch.full([rb, N], 3.0, dtype=dtype, device="cuda"), fill=F.OUT_FILL)
        ops.expert_gemm_packed(xd if gather else xpd, wd, bd, kmajor, lay, act=d["act"], gather=gather or None, zero_row=zero if gather else None, mul=md, out=o)
        F.moat_intact(o, "out")
        return o
    got_d = run(d["gather"])
    assert torch.equal(_bits(got_d), _bits(run(d["gather"]))), "a second call gave other bits"
    if d["gather"]:
        same = _bits(got_d) == _bits(run(False))
        if not bool(same.all()):
            r = int((~same).any(1).nonzero()[0])
            raise AssertionError(f"gathered and materialised launches differ in {int((~same).any(1).sum())} rows, the first row {r} (slot {int(ref['slot'][r]) if r < rb else None})")
    for t, what in ((xd, "x"), (xpd, "packed a"), (wd, "w"), (bd, "bias"), (md, "mul"), (zero, "zero_row"), (lay.slot_map, "slot_map")):
        if t is not None:
            F.moat_intact(t, what)
    got = got_d.cpu()
    assert bool((got[used:] == 3.0).all()), "a row at or past offsets[E] was written"
    assert bool((got[:used] != 0).any()), "the output is all zero"
    full = used * N * K <= F.F64_BUDGET
    rows = np.arange(used) if full else F.tile_sample_rows(ref["tiles"], off, d["seed"])
    want, exact, mag = F.ref_gemm_rows(a_rows, w, bias, kmajor, d["act"], mul, off, dtype, rows)
    gr = got[torch.from_numpy(rows)].double()
    rtol, atol = _gemm_tol(dtype)
    bars = [("gemm bar", (gr - want).abs(), atol + rtol * want.abs())]
    if not kmajor:
        bars.append(("one rounding of an fp32 sum", (gr - exact).abs(), F.nmajor_bound(exact, mag, K, dtype)))
    for what, err, bar in bars:
        if not bool((err <= bar).all()):   # (NaN-safe: a NaN fails the comparison)
            i, c = _first_violation(err - bar, err.shape)
            raise AssertionError(f"{what}: row {int(rows[i])} column {c}: {float(gr[i, c])} vs {float(exact[i, c])} ({int((~(err <= bar)).sum())} elements beyond it)")
        stats["gemm"] = max(stats.get("gemm", 0.0), float((err / bar).max()))
    if mul is not None:
        assert bool((got[:used][mul[:used] == 0] == 0).all()), "a zero in mul did not give an exact zero"


def _prefill(shape, g, empty):
    """random fp32 values, a quarter of them of magnitude ~1e6 (adding a gradient rounds); -0.0 in every third element of an expert
    without rows (an add of +0.0 would turn it into +0.0)"""
    d = torch.randn(shape, generator=g)
    d = torch.where(torch.rand(shape, generator=g) < 0.25, d * 1e6, d)
    for e in empty:
        d[e].view(-1)[::3] = -0.0
    return d


def _check_grad_forms(form, fn, dtype, ref, bar16, bar32, empty, g, what, stats):
    """fn(**kw) -> the gradient: the case's form against its bound, and what ties the forms together"""
    f32 = torch.float32
    if form == "16":
        got_d = fn()
        got = got_d.cpu()
        err, bar = (got.double() - ref).abs(), bar16
        assert torch.equal(_bits(got_d), _bits(fn())), f"{what}: a second call gave other bits"
    else:
        G_d = fn(out_dtype=f32)
        got = G_d.cpu()
        assert got.dtype == f32
        err, bar = (got.double() - ref).abs(), bar32
        assert torch.equal(_bits(G_d.to(dtype)), _bits(fn())), f"{what}: the fp32 sums rounded once are not the 16-bit form's bits"
        assert torch.equal(_bits(G_d), _bits(fn(out_dtype=f32))), f"{what}: a second call gave other bits"
    if not bool((err <= bar).all()):
        at = _first_violation(err - bar, err.shape)
        raise AssertionError(f"{what}{at} = {float(got[tuple(at)])} vs {float(ref[tuple(at)])} ({int((~(err <= bar)).sum())} elements beyond the bound)")
    nz = bar > 0
    if bool(nz.any()):
        stats["grad"] = max(stats.get("grad", 0.0), float((err[nz] / bar[nz]).max()))
    assert bool((got[empty] == 0).all()), f"{what} of an expert without rows is not exactly zero"
    assert bool((got != 0).any()), f"{what} is all zero"
    if form == "acc":
        D0 = _prefill(got.shape, g, empty)
        D = F.moated(D0, fill=F.OUT_FILL, device="cuda")
        ret = fn(accumulate_into=D)
        assert ret.data_ptr() == D.data_ptr()
        F.moat_intact(D, what + " accumulate_into")
        # (values, as tests/test_packed_main_grad_gpu.py compares them: an untouched -0.0 is the -0.0 + 0.0 = +0.0 of the sum; bits below)
        assert torch.equal(D, D0.cuda() + G_d), f"{what}: D is not D + G bit for bit"
        assert not torch.equal(_bits(D.cpu()), _bits(D0))
        for e in empty:
            assert torch.equal(_bits(D[e].cpu()), _bits(D0[e])), f"{what}: an expert without rows was touched"
        D2 = F.moated(D0, fill=F.OUT_FILL, device="cuda")
        fn(accumulate_into=D2)
        assert torch.equal(_bits(D2), _bits(D)), f"{what}: a second accumulating call gave other bits"
    return got


def run_grad_case(d, lay, ref, rb, free, stats):
    from tutel_amd import ops
    dtype = F.DTYPES[d["dtype"]]
    E, Na, Nb, T = d["E"], d["Na"], d["Nb"], d["T"]
    off, used = ref["offsets"], int(ref["offsets"][-1])
    assert used > 0, "the case has no live row"
    g = torch.Generator().manual_seed(d["seed"])
    slot = ref["slot"][:used]

    def operand(N, is_gathered):
        """-> (what the launch takes, the materialised packed copy on the device, the packed rows on the host)"""
        if is_gathered:
            x = _tokens(g, T, N, dtype, free)
            rows = _packed_copy(F.gathered(x, slot), rb, used)
            return F.moated(x, device="cuda"), F.moated(rows, device="cuda"), rows
        rows = _packed_copy(torch.randn([used, N], generator=g).to(dtype), rb, used)
        dev = F.moated(rows, device="cuda")
        return dev, dev, rows
    a_dev, a_mat, a_rows = operand(Na, d["gather"] == "a")
    b_dev, b_mat, b_rows = operand(Nb, d["gather"] == "b")
    gather = None if d["gather"] == "none" else d["gather"]
    zero = F.moated(torch.zeros([max(Na, Nb, 8)], dtype=dtype), device="cuda") if gather else None
    empty = [e for e in range(E) if off[e + 1] == off[e]]
    n_e = torch.from_numpy(ref["kept"].astype(np.float64))      # pad rows are zeros: their products and additions are exact
    wref, bnd = F.ref_wgrad(a_rows[:used], b_rows[:used], off)
    assert not bool(torch.isnan(wref).any())
    bar16 = F.wgrad_bound(wref, bnd, dtype)
    bar32 = 2 ** -23 * wref.abs() + 2 * n_e.view(-1, 1, 1) * 2 ** -24 * bnd      # tests/test_packed_amp_gpu.py
    _check_grad_forms(d["form"], lambda **kw: ops.expert_wgrad_packed(a_dev, b_dev, lay, gather=gather, zero_row=zero, **kw), dtype, wref, bar16, bar32, empty, g, "dW",
                      stats)
    if gather:   # the gathered launch against the same launch on the materialised copy, in the case's form
        kw = {} if d["form"] == "16" else dict(out_dtype=torch.float32)
        assert torch.equal(_bits(ops.expert_wgrad_packed(a_dev, b_dev, lay, gather=gather, zero_row=zero, **kw)), _bits(ops.expert_wgrad_packed(a_mat, b_mat, lay, **kw))), \
            "gathered and materialised launches differ"
    if d["gather"] != "b":   # the bias gradient sums packed rows (it has no gathered form)
        dref, mag, n = F.ref_bgrad(b_rows[:used], off)
        db16 = F.bgrad_bound(dref, mag, n, dtype)
        db32 = n_e.unsqueeze(1) * 2 ** -24 * mag + 2 ** -23 * dref.abs()
        _check_grad_forms(d["form"], lambda **kw: ops.expert_bgrad_packed(b_dev, lay, **kw), dtype, dref, db16, db32, empty, g, "db", stats)
    for t, what in ((a_dev, "a"), (b_dev, "b"), (a_mat, "a copy"), (b_mat, "b copy"), (zero, "zero_row"), (lay.slot_map, "slot_map")):
        if t is not None:
            F.moat_intact(t, what)


def run_train_form_fuzz(n_cases, seed, verbose=False, stats=None):
    """-> list of failure descriptions (stats: the largest error over its bound, per kind of check)"""
    bad, seen, t0 = [], set(), time.time()
    stats = {} if stats is None else stats
    for d in F.gen_train_form_cases(n_cases, seed):
        tag = F.train_tag(d)
        try:
            lay, ref, rb, free = routing_layout(d)
            seen |= F.train_classes(d, ref)
            assert free is not None or d["T"] == 1, "no token is left unread for the slot map's band to name"
            (run_grad_case if d["kind"] == "wgrad" else run_gemm_case)(d, lay, ref, rb, free, stats)
        except Exception as ex:  # noqa: BLE001 -- the sweep reports every failing case
            _fail(bad, tag, ex, verbose)
        if verbose and (d["case"] + 1) % 20 == 0:
            print(f"{d['case'] + 1} train form cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    F.check_promised("train forms", seen, F.TRAIN_PROMISED, n_cases, DEFAULT_CASES)
    stats["seen"] = sorted(seen)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_packed_train_forms_fuzz_vs_float64(n_cases):
    stats = {}
    t0 = time.time()
    bad = run_train_form_fuzz(n_cases, SEED, stats=stats)
    print(f"{n_cases} train form cases in {time.time() - t0:.1f} s, {len(bad)} failed; largest error over bound: gemm {stats.get('gemm', 0):.3f}, grad {stats.get('grad', 0):.3f}")
    assert not bad, f"{len(bad)} of {n_cases} cases failed:\n" + "\n".join(bad[:20])


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10 * DEFAULT_CASES
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else SEED
    st = {}
    failed = run_train_form_fuzz(n, sd, verbose=True, stats=st)
    print("cases", n, "failed", len(failed), "largest error over bound", {k: v for k, v in st.items() if k != "seen"})
    sys.exit(1 if failed else 0)
