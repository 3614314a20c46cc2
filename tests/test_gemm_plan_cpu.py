"""Which kernel every grouped GEMM runs, pinned without a GPU.  The library picks the kernel, its variant and its grid in one pure
function (gemm_plan, csrc/gemm_plan.hip); tutel_amd_expert_gemm_plan_next shows the answer of the next entry point before any HIP call.
This test walks a table of cases -- a small product of shapes, layouts and knobs plus named rows on both sides of every boundary the
planner has -- and compares status, error text and EVERY field of the plan with tests/golden/gemm_plans.json.  That file was recorded
from the tree BEFORE the planner existed (its launchers patched to note the kernel's own symbol and launch geometry instead of
launching), so a change to a rule shows up here and nowhere else first.  Pointers are aligned integers that are never dereferenced.

    python tests/test_gemm_plan_cpu.py --record     rewrites the golden file from the tree at hand (after changing a rule on purpose)
"""
import ctypes
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_gemm_refusals_cpu import Q, moe_args, packed_fwd  # noqa: E402  (the pipelines' argument structs, same fake pointers)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.json")
P, W, D, X4, X5, G = (i << 24 for i in range(1, 7))      # "device pointers", 16 MiB apart
F32, BF16 = 0, 2
NONE, RELU, GELU, SILU = 0, 1, 2, 3
ENOTSUP = 1001
AUTO = dict(impl=-1, tile=-1, persist=-1, splitk=-1, corun=0, ffn=-1)
# every refusal text the planner and the checks around it can answer with TUTEL_AMD_ENOTSUP: each must appear in the table
ENOTSUP_TEXTS = [
    "tutel_expert_gemm_gather_fl: this launch does not take the fused-location ring kernel",
    "tutel_amd_expert_gemm_gate_up: not covered: the gate activation must be relu, gelu or silu",
    "tutel_amd_expert_gemm_gate_up: not covered: operands past 2 GiB",
    "tutel_amd_expert_gemm_gate_up: not covered: output rows must be 16-byte aligned",
    "tutel_expert_gemm_packed: operands past 2 GiB are not covered",
    "tutel_amd_expert_gemm_packed: not covered: 16-bit operands only",
    "tutel_amd_expert_gemm_packed: not covered: n-major weights take act none or relu",
    "tutel_amd_expert_gemm_packed: not covered: the gated form takes k-major weights",
]


# ---- the entry points: (name, ctypes arguments) per kind of case -------------------------------------------------------------------
def padded(E, R, N, K, km=1, act=RELU, dtype=BF16, rc=0, mul=0, gather=0, ldd=0, far=0):
    """tutel_amd_expert_gemm / _glu (mul) / _gather (gather).  ldd: an output row pitch of its own; far: rows of A in two ranks 2 GiB
    apart, so that 32-bit offsets do not reach them (by stride alone)"""
    ldd, ldw, rows = ldd or N, (K if km else N), (X4 if rc else None)
    if gather:
        return ("tutel_amd_expert_gemm_gather", (P, K, X4, 64, X5, W, km, N * K, ldw, None, 0, D, R * ldd, ldd, E, R, N, K, dtype, act, rows, 1, None))
    a_rpw, a_sw = (max(R // 2, 1), 1 << 30) if far else (R, 0)
    head = (P, R * K, a_sw, a_rpw, K, W, km, N * K, ldw, None, 0)
    tail = (D, R * ldd, 0, R, ldd, E, R, N, K, dtype, act, rows, 1, None)
    return ("tutel_amd_expert_gemm_glu", head + (G,) + tail) if mul else ("tutel_amd_expert_gemm", head + tail)


def gate_up(E, R, N, K, act=RELU, rc=0, ldd=0, far=0):
    ldd = ldd or N
    a_rpw, a_sw = (max(R // 2, 1), 1 << 30) if far else (R, 0)
    return ("tutel_amd_expert_gemm_gate_up", (P, R * K, a_sw, a_rpw, K, W, G, N * K, K, D, R * ldd, 0, R, ldd, E, R, N, K, BF16, act,
                                              X4 if rc else None, 1, None))


def packed(E, N, K, tiles, km=1, act=RELU, dtype=BF16, mul=0, gather=0, rows=4096):
    return ("tutel_amd_expert_gemm_packed", (P, K, X4 if gather else None, 64 if gather else 0, X5 if gather else None, W, km, N * K,
                                             K if km else N, None, 0, G if mul else None, D, N, E, rows, N, K, dtype, act, X4, X4, X4, X4, tiles, None))


def ffn(E, R, M, H, gather=0):
    return ("tutel_amd_expert_ffn", (P, 0 if gather else R * M, M, X4 if gather else None, 64 if gather else 0, X5 if gather else None, W, H * M, M,
                                     None, 0, D, R * H, H, G, M * H, H, None, 0, D + (1 << 23), R * M, M, E, R, M, H, M, BF16, RELU, None))


def fused_location(E, C, M, H, T=64, k=1):
    """tutel_amd_moe_forward on its fused-location route: out[0] its eligibility query, out[1] the fc1 launch after a yes"""
    m = moe_args(dict(T=T, M=M, H=H, M_out=M, num_experts=E, k=k, capacity=C), fl_ws=Q[18], fl_ws_bytes=1 << 16, ws_bytes=1 << 24)
    return ("tutel_amd_moe_forward", (None, ctypes.byref(m), None))


def packed_forward(E, T, M, H, glu=1):
    """tutel_amd_moe_forward_packed[_glu]: out[0] fc1 (glu: the fused gate/up GEMM over the packed layout), out[1] fc2"""
    return packed_fwd(dict(T=T, M=M, H=H, M_out=M, num_experts=E, k=2), w_up=Q[33] if glu else False, ws_bytes=1 << 24)


KINDS = dict(padded=padded, gate_up=gate_up, packed=packed, ffn=ffn, fl=fused_location, fwd=packed_forward)


def _cases():
    out = []

    def add(kind, *a, **kw):
        knobs = {k: kw.pop(k) for k in list(kw) if k in AUTO}
        if (kind, a, kw, knobs) not in out:            # (a row that belongs to two of the groups below stands once)
            out.append((kind, a, kw, knobs))

    # ---- the product: four shapes (below / at the chip with one M-tile; half / whole chip with 256-row tiles) x layout x IMPL x TILE
    for shape in [(256, 128, 256, 128), (4, 1024, 2048, 512)]:
        for km in (1, 0):
            for impl in (-1, 0, 1, 2, 4):
                for tile in (-1, 0, 1, 2, 3, 4):
                    add("padded", *shape, km=km, impl=impl, tile=tile)
    for shape in [(2, 128, 256, 128), (8, 1024, 2048, 512)]:
        for km in (1, 0):
            for tile in (-1, 0, 1, 2, 3, 4):
                add("padded", *shape, km=km, tile=tile)
    # ---- rows per expert: 128 | 129 (one M-tile or not), 255 | 256 (K-tile rotation, a full tile), a tail of 224 | 225 rows (RAGGED)
    for R in (128, 129, 224, 225, 255, 256, 480, 481):
        for km in (1, 0):
            add("padded", 256, R, 256, 128, km=km)
    # ---- "the grid covers the chip": E_loc * ceil(N / 256) at 255 | 256, for the 128 x 256 ring and for W_ONCE
    for E in (255, 256):
        add("padded", E, 128, 256, 128)
        add("padded", E, 200, 256, 128)
        add("padded", E, 128, 256, 128, impl=4)
    add("padded", 128, 128, 512, 128)
    add("padded", 128, 128, 504, 128)
    # ---- 256 x 256 tiles at 95 | 96, 128 | 129, 191 | 192, with and without the co-run hint; 256 x 128 tiles at 191 | 192
    for E in (95, 96, 128, 129, 191, 192):
        for km in (1, 0):
            for corun in (0, 1):
                add("padded", E, 256, 256, 512, km=km, corun=corun)
    for N in (191 * 128, 192 * 128):
        add("padded", 1, 256, N, 128)
    for E in (63, 64):
        add("padded", E, 256, 384, 128)
    # ---- N at 120 | 128, 248 | 256, 384 with one M-tile and with 256-row tiles
    for N in (120, 128, 248, 256, 384):
        add("padded", 256, 128, N, 128)
        add("padded", 256, 512, N, 128)
        add("padded", 256, 512, N, 128, km=0)
    # ---- K: one K-tile, two, eight
    for K in (64, 128, 512):
        add("padded", 256, 128, 256, K)
        add("padded", 4, 1024, 2048, K, tile=4)
    # ---- split-K: its band, nk < 8, odd nk, tiles not a multiple of four, partial tiles, row counts, the gated form, unaligned rows
    for kw in (dict(), dict(K=256), dict(K=576), dict(R=1000), dict(rc=1), dict(mul=1), dict(ldd=2052), dict(km=0), dict(tile=4), dict(tile=1),
               dict(corun=1), dict(far=1)):
        a = dict(dict(E=4, R=1024, N=2048, K=512), **kw)
        add("padded", a.pop("E"), a.pop("R"), a.pop("N"), a.pop("K"), splitk=1, **a)
    for E in (95, 96, 97, 100, 188, 192):
        add("padded", E, 256, 256, 512, splitk=1)
    # ---- the ping-pong kernel's forms: bias before / after the K loop, row counts, W_ONCE, a partial last tile
    for persist in (-1, 0):
        add("padded", 8, 1024, 2048, 512, persist=persist)
        add("padded", 256, 256, 256, 128, persist=persist)
        add("padded", 256, 200, 256, 128, persist=persist)
        add("padded", 8, 1024, 2048, 512, rc=1, persist=persist)
    # ---- row counts, the gated form, gathered rows, unaligned output rows, operands past 2 GiB, dtype, activations: every regime
    for shape in [(256, 128, 256, 128), (4, 1024, 2048, 512), (8, 1024, 2048, 512), (2, 128, 128, 128)]:
        for kw in (dict(rc=1), dict(mul=1), dict(gather=1), dict(ldd=shape[2] + 4), dict(far=1), dict(dtype=1, act=GELU), dict(act=NONE, km=0)):
            add("padded", *shape, **kw)
    add("padded", 4, 1024, 2048, 512, tile=3, far=1)
    add("padded", 4, 1024, 2048, 512, tile=3, ldd=2052)
    add("padded", 2, 128, 256, 128, act=7)
    add("padded", 1 << 20, 1 << 20, 256, 128)                       # the grid itself too large
    add("padded", 1, 1 << 20, 2048, 128)                            # an expert's output past 2 GiB: plain stores
    # ---- the packed layout: ping-pong (k-major), register-staged (n-major), tiles_bound 1 | 300, the chip covered or not
    for tiles in (1, 300):
        for E in (2, 256):
            add("packed", E, 256, 128, tiles)
            add("packed", E, 256, 128, tiles, km=0, act=NONE)
        add("packed", 2, 248, 128, tiles, mul=1, gather=1, act=SILU)
    add("packed", 2, 256, 128, 1 << 30)                              # grid too large
    add("packed", 2, 256, 128, 1 << 30, km=0)
    add("packed", 2, 256, 128, 1, dtype=F32)
    add("packed", 2, 256, 128, 1, km=0, act=GELU)
    add("packed", 2, 256, 128, 1, km=0, mul=1)
    add("packed", 2, 256, 1024, 1, rows=1 << 20)                     # operands past 2 GiB
    add("packed", 2, 256, 128, 1, act=7)
    # ---- the fused gate/up GEMM, padded and (through the packed forward) packed
    for E, R in ((2, 300), (256, 128), (64, 512)):
        add("gate_up", E, R, 256, 128)
        add("gate_up", E, R, 200, 128, act=SILU, rc=1)
    add("gate_up", 2, 300, 256, 128, act=NONE)
    add("gate_up", 2, 300, 256, 128, ldd=260)
    add("gate_up", 2, 300, 256, 2048, far=1)
    add("gate_up", 1 << 20, 1 << 20, 256, 128)
    for glu in (1, 0):
        add("fwd", 2, 64, 128, 128, glu=glu)
        add("fwd", 64, 4096, 256, 512, glu=glu)
    # ---- the FFN pair: covered or not (TUTEL_OPT_FFN_FUSED = 1), and the option's default
    for ffn_opt in (1, -1):
        add("ffn", 256, 128, 256, 256, ffn=ffn_opt)
    add("ffn", 2, 128, 256, 256, ffn=1)
    add("ffn", 256, 128, 256, 256, gather=1, ffn=1)
    add("ffn", 256, 128, 256, 256, ffn=1, impl=4)
    add("ffn", 256, 160, 256, 256, ffn=1)
    add("ffn", 256, 128, 256, 248, ffn=1)
    # ---- fused location: the query and the launch after it; one K-tile, a grid that does not cover the chip, forced kernels
    add("fl", 64, 128, 128, 1024)
    add("fl", 64, 128, 64, 1024)
    add("fl", 2, 128, 128, 1024)
    add("fl", 2, 128, 128, 1024, impl=4)
    add("fl", 64, 128, 128, 1024, tile=0)
    add("fl", 64, 128, 128, 1024, tile=1)
    add("fl", 64, 128, 128, 1024, impl=1)
    return out


CASES = _cases()


def case_name(case):
    kind, a, kw, knobs = case
    return kind + "(" + ", ".join([str(v) for v in a] + ["%s=%s" % kv for kv in list(kw.items()) + list(knobs.items())]) + ")"


def set_knobs(L, knobs):
    from tutel_amd import _lib
    k = dict(AUTO, **knobs)
    for key, opt in (("impl", _lib.OPT_GEMM_IMPL), ("tile", _lib.OPT_GEMM_TILE), ("persist", _lib.OPT_GEMM_PERSIST), ("splitk", _lib.OPT_GEMM_SPLITK),
                     ("ffn", _lib.OPT_FFN_FUSED)):
        assert L.tutel_amd_set_option(opt, k[key]) == 0
    return k["corun"]


def ask(L, case):
    """status, error text and the two plans of one case, asked through tutel_amd_expert_gemm_plan_next (fields at 0 left out)"""
    from tutel_amd import _lib
    kind, a, kw, knobs = case
    name, args = KINDS[kind](*a, **kw)
    corun = set_knobs(L, knobs)
    try:
        plans = (_lib.GemmPlan * 2)()
        marker = "tutel_amd_set_option: unknown key 99"
        assert L.tutel_amd_set_option(99, 0) == -1
        assert L.tutel_amd_expert_gemm_plan_next(ctypes.byref(plans), corun) == 0
        status = getattr(L, name)(*args)
        text = L.tutel_amd_last_error().decode()
    finally:
        set_knobs(L, {})
    row = dict(status=status, error=None if text == marker else text)
    for i, p in enumerate(plans):
        if p.family >= 0:
            row["plan%d" % i] = {n: getattr(p, n) for n, _ in _lib.GemmPlan._fields_ if getattr(p, n) != 0 or n == "family"}
    return row


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def _full(plan):
    from tutel_amd import _lib
    return {n: plan.get(n, 0) for n, _ in _lib.GemmPlan._fields_}


def test_every_case_plans_as_recorded(L, golden):
    assert sorted(golden) == sorted(case_name(c) for c in CASES), "the golden file and the case list name different cases"
    wrong = []
    for c in CASES:
        got, want = ask(L, c), golden[case_name(c)]
        same = got["status"] == want["status"] and got["error"] == want["error"]
        for slot in ("plan0", "plan1"):
            same = same and (slot in got) == (slot in want) and (slot not in got or _full(got[slot]) == _full(want[slot]))
        if not same:
            wrong.append((case_name(c), got, want))
    assert not wrong, "%d of %d cases plan differently; the first:\n got  %s\n want %s\n for  %s" % (
        len(wrong), len(CASES), wrong[0][1], wrong[0][2], wrong[0][0])


def test_the_arm_clears_itself(L):
    """one armed call answers without launching; the next call on the thread is an ordinary one (here: refused by its own checks)"""
    from tutel_amd import _lib
    plans = (_lib.GemmPlan * 2)()
    for first in (padded(2, 128, 256, 128), padded(2, 128, 256, 96)):          # a call that plans, a call refused before it plans
        assert L.tutel_amd_expert_gemm_plan_next(ctypes.byref(plans), 0) == 0
        getattr(L, first[0])(*first[1])
        seen = plans[0].family
        name, args = padded(2, 128, 12, 128)
        assert getattr(L, name)(*args) == -1 and L.tutel_amd_last_error() == b"tutel_amd_expert_gemm: N=12 must be a multiple of 8"
        assert plans[0].family == seen
    assert L.tutel_amd_expert_gemm_plan_next(None, 0) == -1


def test_the_table_reaches_every_family_variant_and_refusal(golden):
    from tutel_amd import _lib
    plans = [_full(row[s]) for row in golden.values() for s in ("plan0", "plan1") if s in row]
    assert len(golden) == len(CASES) == len(set(case_name(c) for c in CASES))
    assert {p["family"] for p in plans} == set(range(len(_lib.GEMM_FAMILIES)))
    ring = [p for p in plans if p["family"] == _lib.GEMM_FAMILIES.index("RING")]
    pp = [p for p in plans if p["family"] == _lib.GEMM_FAMILIES.index("PINGPONG")]
    assert {p["ni"] for p in ring} == {2, 4} and {p["ns"] for p in ring} == {2, 3} and {p["bm"] for p in ring} == {128, 256}
    for field in ("buf", "fl", "w_kmajor", "lds_epilogue"):
        assert {p[field] for p in ring} == {0, 1}, field
    for field in ("w_once", "ragged", "early_bias", "splitk", "packed", "gate_up", "lds_epilogue"):
        assert {p[field] for p in pp} == {0, 1}, field
    for field in ("rot_on", "fits32", "covered"):
        assert {p[field] for p in plans} == {0, 1}, field
    assert {p["d_store"] for p in plans} >= {0, 1}
    assert {row["status"] for row in golden.values()} >= {0, ENOTSUP, -1} and {p["status"] for p in plans} == {0, 1}
    texts = {row["error"] for row in golden.values() if row["status"] == ENOTSUP}
    assert texts >= set(ENOTSUP_TEXTS), set(ENOTSUP_TEXTS) - texts
    assert any(row["error"] is not None and row["error"].endswith("grid too large") for row in golden.values())


def write_golden(rows, path=GOLDEN):
    """one compact line per case"""
    lines = ["%s: %s" % (json.dumps(name), json.dumps(rows[name], separators=(",", ":"))) for name in rows]
    open(path, "w").write("{\n" + ",\n".join(lines) + "\n}\n")


if __name__ == "__main__":
    if "--record" in sys.argv:
        from tutel_amd import _lib
        _lib.build()
        write_golden({case_name(c): ask(_lib.lib(), c) for c in CASES})
        print("recorded", len(CASES), "cases ->", GOLDEN)
