"""The PLAIN form of the 128 x 256 ring GEMM kernel, without a GPU: who takes it (gemm_plain_admits, csrc/gemm_plan.hip, asked through
armed calls -- tutel_amd_expert_gemm_plan_next -- with integer "pointers" that are never followed, then tutel_amd_expert_gemm_last_form),
its switch (tutel_amd_gemm_plain / TUTEL_AMD_GEMM_PLAIN), and its three division-free index helpers (csrc/gemm_plain.h, compiled here
with g++) against the division forms they replace, computed in numpy with 64-bit integers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from test_gemm_plan_cpu import fused_location, set_knobs  # noqa: E402  (the planner test's knobs and its fused-location call)

P, W, D, X4, X5, G, B = (i << 24 for i in range(1, 8))            # "device pointers", 16 MiB apart
BF16, F16 = 2, 1
NONE, RELU = 0, 1
GENERAL, PLAIN = 0, 1


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def gemm(E=256, R=128, N=256, K=128, km=1, act=RELU, dtype=BF16, a_rpw=None, d_rpw=None, ldd=None, rc=0, mul=0, gather=0, bias=0):
    """tutel_amd_expert_gemm / _glu / _gather on contiguous operands; a_rpw / d_rpw < R: the rows of an expert split over source ranks
    that lie back to back (the same bytes, so every other condition stays as it was)"""
    ldd, ldw = ldd or N, (K if km else N)
    a_rpw, d_rpw = a_rpw or R, d_rpw or R
    rows, b = (X4 if rc else None), (B if bias else None)
    if gather:
        return ("tutel_amd_expert_gemm_gather", (P, K, X4, 64, X5, W, km, N * K, ldw, b, N if bias else 0, D, R * ldd, ldd, E, R, N, K, dtype, act, rows, 1, None))
    head = (P, R * K, min(a_rpw, R) * K, a_rpw, K, W, km, N * K, ldw, b, N if bias else 0)
    tail = (D, R * ldd, min(d_rpw, R) * ldd, d_rpw, ldd, E, R, N, K, dtype, act, rows, 1, None)
    return ("tutel_amd_expert_gemm_glu", head + (G,) + tail) if mul else ("tutel_amd_expert_gemm", head + tail)


def form(L, call, mode=-1, store=-1, **knobs):
    """the form the call would launch: (status, TUTEL_GEMM_FORM_*, family of the plan)"""
    from tutel_amd import _lib
    name, args = call
    set_knobs(L, knobs)
    assert L.tutel_amd_set_option(_lib.OPT_GEMM_STORE, store) == 0
    was = L.tutel_amd_gemm_plain(mode)
    try:
        plans = (_lib.GemmPlan * 2)()
        assert L.tutel_amd_expert_gemm_plan_next(ctypes.byref(plans), 0) == 0
        status = getattr(L, name)(*args)
        fam = [p.family for p in plans]
        return status, L.tutel_amd_expert_gemm_last_form(None), fam
    finally:
        set_knobs(L, {})
        L.tutel_amd_set_option(_lib.OPT_GEMM_STORE, -1)
        L.tutel_amd_gemm_plain(was)


def test_the_predicate_on_both_sides_of_every_condition(L):
    from tutel_amd import _lib
    RING = _lib.GEMM_FAMILIES.index("RING")
    yes = lambda call, **kw: form(L, call, **kw)[:2] == (0, PLAIN)
    no = lambda call, **kw: form(L, call, **kw)[:2] == (0, GENERAL)
    assert form(L, gemm()) == (0, PLAIN, [RING, -1])
    # the plan: the 128-row ring (family, bm, ni, ns, buf, k-major weights) and nothing else
    assert no(gemm(), impl=1) and no(gemm(), impl=0) and no(gemm(km=0)) and no(gemm(E=2)) and yes(gemm(E=2), impl=4)
    assert yes(gemm(R=128)) and no(gemm(R=129)) and no(gemm(R=256)) and no(gemm(E=4, R=1024, N=2048, K=512))
    assert no(gemm(), tile=1) and no(gemm(), tile=3)
    # plain rows: every row of A, and of D, in one source rank
    for R in (128, 72):
        assert yes(gemm(R=R, a_rpw=R)) and yes(gemm(R=R, a_rpw=R + 1)) and no(gemm(R=R, a_rpw=R - 1)) and no(gemm(R=R, a_rpw=R // 2))
        assert yes(gemm(R=R, d_rpw=R)) and yes(gemm(R=R, d_rpw=R + 1)) and no(gemm(R=R, d_rpw=R - 1)) and no(gemm(R=R, d_rpw=R // 2))
    # no gating operand, no row counts (peer rows exist inside the expert-parallel pipeline only: no single-GEMM entry point states them)
    assert no(gemm(mul=1)) and no(gemm(rc=1)) and no(gemm(gather=1, rc=1))
    # 16-byte output rows; write-through stores
    assert yes(gemm(ldd=264)) and no(gemm(ldd=260))
    assert yes(gemm(), store=1) and no(gemm(), store=0) and no(gemm(), store=2)
    # whole 256-column tiles (K is a multiple of 64 or the call is refused before it plans)
    assert yes(gemm(N=512)) and no(gemm(N=384)) and no(gemm(N=264)) and yes(gemm(E=64, N=1024, K=64))
    st, f, fam = form(L, gemm(K=96))
    assert st == -1 and fam == [-1, -1]
    # the rotation in 32 bits: (ntn + 3 E_loc) * nk < 2^31
    big = 1 << 22
    assert (1 + 3 * big) * 170 < 2 ** 31 <= (1 + 3 * big) * 171
    assert yes(gemm(E=big, K=64 * 170)) and no(gemm(E=big, K=64 * 171))
    # the other dtype, activations, a bias, gathered rows: all admitted
    assert yes(gemm(dtype=F16, act=NONE)) and yes(gemm(bias=1)) and yes(gemm(gather=1)) and yes(gemm(gather=1, bias=1, act=3)) and yes(gemm(act=2))
    # the switch: 0 never, 1 and automatic wherever admitted -- and never where not
    assert no(gemm(), mode=0) and yes(gemm(), mode=1) and yes(gemm(), mode=-1) and no(gemm(mul=1), mode=1) and no(gemm(gather=1), mode=0)


def test_the_fused_location_launch_takes_it_too(L):
    """tutel_amd_moe_forward on its fused-location route: the query notes nothing, the fc1 launch after it is admitted"""
    for mode, want in ((1, PLAIN), (0, GENERAL)):
        st, f, fam = form(L, fused_location(64, 128, 128, 1024), mode=mode)
        assert (st, f) == (0, want) and fam[1] >= 0, (mode, st, f, fam)


def test_the_plan_record_is_the_same_for_both_forms_and_armed_calls_are_not_counted(L):
    from tutel_amd import _lib
    n0, n1 = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    L.tutel_amd_expert_gemm_last_form(ctypes.byref(n0))

    def plan(mode):
        was = L.tutel_amd_gemm_plain(mode)
        try:
            plans = (_lib.GemmPlan * 2)()
            assert L.tutel_amd_expert_gemm_plan_next(ctypes.byref(plans), 0) == 0
            name, args = gemm(bias=1)
            assert getattr(L, name)(*args) == 0
            return [getattr(plans[0], n) for n, _ in _lib.GemmPlan._fields_]
        finally:
            L.tutel_amd_gemm_plain(was)
    assert plan(0) == plan(1)
    L.tutel_amd_expert_gemm_last_form(ctypes.byref(n1))
    assert list(n0) == list(n1)


def test_the_switch_its_default_and_its_environment_name(L):
    from tutel_amd import _lib
    assert _lib.GEMM_PLAIN_ENV == "TUTEL_AMD_GEMM_PLAIN"
    assert (_lib.GEMM_FORM_NONE, _lib.GEMM_FORM_GENERAL, _lib.GEMM_FORM_PLAIN) == (-1, 0, 1)
    was = L.tutel_amd_gemm_plain(-2)
    try:
        assert L.tutel_amd_gemm_plain(0) == was and L.tutel_amd_gemm_plain(-2) == 0 and L.tutel_amd_gemm_plain(1) == 0 and L.tutel_amd_gemm_plain(-1) == 1
        L.tutel_amd_gemm_plain(0)
        assert L.tutel_amd_gemm_plain(2) == -1 and b"out of range" in L.tutel_amd_last_error() and L.tutel_amd_gemm_plain(-2) == 0
        assert L.tutel_amd_gemm_plain(-3) == -1 and L.tutel_amd_gemm_plain(-2) == 0
    finally:
        L.tutel_amd_gemm_plain(was)
    # a fresh process: automatic unless the environment says otherwise; no grouped GEMM yet on its thread
    code = "from tutel_amd import _lib; L = _lib.lib(); print(L.tutel_amd_gemm_plain(-2), L.tutel_amd_expert_gemm_last_form(None))"
    for value, want in ((None, "-1 -1"), ("0", "0 -1"), ("1", "1 -1")):
        env = {k: v for k, v in os.environ.items() if k != "TUTEL_AMD_GEMM_PLAIN"}
        if value is not None:
            env["TUTEL_AMD_GEMM_PLAIN"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


# ---- the helpers against / and % -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = tmp_path_factory.mktemp("gemm_plain_fuzz") / "gemm_plain_fuzz.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tutel_amd", "csrc"),
                        os.path.join(HERE, "gemm_plain_fuzz.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return ctypes.CDLL(str(so))


def _run(fn, *cols, dtype=np.int32):
    cols = [np.ascontiguousarray(c, dtype=dtype) for c in cols]
    out = np.empty_like(cols[0])
    fn(ctypes.c_long(cols[0].size), *[c.ctypes.data_as(ctypes.c_void_p) for c in cols], out.ctypes.data_as(ctypes.c_void_p))
    return out.astype(np.int64)


def test_the_argument_block_is_five_scalar_loads(H):
    assert H.plain_args_bytes() == 160


def test_rotation_equals_the_division_form(H):
    """rot = ((pair + 3 e) * nk / npair) % nk for e < 4096, npair = ntn <= 64, nk <= 512: every (npair, nk) with the extreme experts and
    tiles, a random sample in between, and the largest values the host admits"""
    rng = np.random.default_rng(20260)
    npair, nk = np.meshgrid(np.arange(1, 65), np.arange(1, 513), indexing="ij")
    npair, nk = npair.ravel(), nk.ravel()
    cols = []
    for e in (0, 1, 2, 4094, 4095):
        for pair in (np.zeros_like(npair), npair - 1, npair // 2):
            cols.append((pair, np.full_like(npair, e), nk, npair))
    n = 2_000_000
    r_np = rng.integers(1, 65, n)
    cols.append((rng.integers(0, 1 << 30, n) % r_np, rng.integers(0, 4096, n), rng.integers(1, 513, n), r_np))
    # the admitted limit: (npair + 3 E_loc) * nk just below 2^31, the last expert's last tile
    for npair_, E_loc, nk_ in ((1, 1 << 22, 170), (64, 4096, 512), (8, 715825, 1000), (3, 1, 357913941), (1, 357913940, 2), (64, 64, 8388607)):
        assert (npair_ + 3 * E_loc) * nk_ < 2 ** 31
        assert _run(H.plain_rot_fits, [npair_], [E_loc], [nk_])[0] == 1
        ee = np.unique(np.clip(np.array([0, 1, E_loc // 2, E_loc - 2, E_loc - 1]), 0, E_loc - 1))
        pp = np.unique(np.array([0, npair_ // 2, npair_ - 1]))
        e_, p_ = np.meshgrid(ee, pp, indexing="ij")
        cols.append((p_.ravel(), e_.ravel(), np.full(e_.size, nk_), np.full(e_.size, npair_)))
    for npair_, E_loc, nk_ in ((1, 1 << 22, 171), (2, 357913941, 2), (64, 64, 8388608)):
        assert (npair_ + 3 * E_loc) * nk_ >= 2 ** 31 and _run(H.plain_rot_fits, [npair_], [E_loc], [nk_])[0] == 0
    for pair, e, nk_, npair_ in cols:
        pair, e, nk_, npair_ = (np.asarray(c, dtype=np.int64) for c in (pair, e, nk_, npair_))
        want = ((pair + 3 * e) * nk_ // npair_) % nk_
        got = _run(H.plain_rot, pair, e, nk_, npair_)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:4]


def test_slot_to_token_equals_the_remainder(H):
    """q % T for q < k * T, k <= 8, T <= 65536: every T at the edges of every multiple, and a random sample"""
    rng = np.random.default_rng(20261)
    T = np.arange(1, 65537, dtype=np.int64)
    qs, ts = [], []
    for k in range(1, 9):
        for d in (0, 1, -1):
            q = k * T + d
            keep = (q >= 0) & (q < 8 * T)
            qs.append(q[keep]); ts.append(T[keep])
    qs.append(np.zeros_like(T)); ts.append(T)
    tr = rng.integers(1, 65537, 2_000_000)
    qs.append(rng.integers(0, 1 << 40, tr.size) % (8 * tr)); ts.append(tr)
    qs.append(np.array([8 * 65536 - 1, 2 ** 31 - 1, 2 ** 31 - 1])); ts.append(np.array([65536, 65536, 1]))
    q, t = np.concatenate(qs), np.concatenate(ts)
    assert np.array_equal(_run(H.plain_slot_token, q, t), q % t)


def test_row_offsets_equal_the_split_form(H):
    """(m / rpw) * stride_w + (m % rpw) * ld for rows m < 128 <= rpw is m * ld, whatever stride_w"""
    m, ld = np.meshgrid(np.arange(128, dtype=np.int64), np.array([8, 64, 72, 2048, 2056, 65536, (2 ** 31 - 1) // 127], dtype=np.int64), indexing="ij")
    m, ld = m.ravel(), ld.ravel()
    got = _run(H.plain_row_off, m, ld)
    for rpw in (128, 129, 1 << 20):
        for stride_w in (0, 12345678):
            assert np.array_equal(got, (m // rpw) * stride_w + (m % rpw) * ld)


def test_the_reciprocal_division_is_exact_over_32_bits(H):
    """what the three helpers and the kernel's work-item split rest on: floor(x / d) for ANY 32-bit x and d >= 1"""
    rng = np.random.default_rng(20262)
    d = np.concatenate([np.arange(1, 4097), rng.integers(1, 1 << 32, 200_000), [2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 16, 65537]]).astype(np.int64)
    for x in (np.zeros_like(d), d - 1, d, d + 1, (2 ** 32 - 1) // d * d, (2 ** 32 - 1) // d * d - 1, np.full_like(d, 2 ** 32 - 1),
              rng.integers(0, 1 << 32, d.size)):
        x = np.clip(x, 0, 2 ** 32 - 1)
        got = _run(H.plain_div, x, d, dtype=np.uint32)
        assert np.array_equal(got, x // d)
