"""The fuzzers of csrc/dispatch.hip (tests/test_dispatch_fuzz_gpu.py) without a GPU: their generators alone (every promised edge class drawn
at the default length and seed, every operand within the element budget by construction, the long form starting with the default cases);
their references (tests/_dispatch_fuzz.py) against the C oracle on the plain-layout cases with short rows -- encode and decode bit for
bit, the gate gradient within the bound of the oracle's own serial fp32 sum and equal where the sums are exact -- and against brute force
for the two bucket orders; and the bar of the gate-gradient fuzzer against an emulation of a wave's summation order in numpy fp32."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _dispatch_fuzz as D   # noqa: E402
from test_dispatch_fuzz_gpu import DEFAULT_CASES, SEEDS   # noqa: E402

ORACLE_M = 264      # the oracle's scalar loops take the short rows


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_but_zero_sign(got, want):
    """equal values, and equal bits except where the reference is a zero of either sign (test_ops_gpu.py::test_encode_decode_vs_oracle)"""
    return torch.equal(got.float(), want.float()) and bool(((_bits(got) == _bits(want)) | (want.float() == 0)).all())


def _crit(d, c, gates):
    k, T = d["k"], d["T"]
    it, lt = torch.from_numpy(c["idx"]), torch.from_numpy(c["loc"])
    return (d["E"], [it[j] for j in range(k)], [lt[j] for j in range(k)], [gates[j].float() if gates is not None else torch.ones([T]) for j in range(k)],
            c["C"], None)


def _sized(d, c, rows):
    assert d["T"] * d["M"] <= D.BUDGET and rows * d["M"] <= D.BUDGET, (d, c["C"])
    assert d["k"] <= d["E"] and d["k"] in D.K_CHOICES and d["E"] in D.E_CHOICES and d["M"] in D.row_lengths(d["dtype"])
    assert d["T"] in D.T_CHOICES + [8200, 4100] and d["scale"] in D.SCALES
    idx = c["idx"]
    for t in range(0, d["T"], max(1, d["T"] // 50)):        # k distinct experts per token where not masked
        col = [int(v) for v in idx[:, t] if v >= 0]
        assert len(set(col)) == len(col) and all(v < d["E"] for v in col)


# ---- the generators alone ------------------------------------------------------------------------------------------------------------
def test_row_lengths_are_the_ones_the_fuzzers_promise():
    for dtype, vn in (("bf16", 8), ("f16", 8), ("f32", 4)):
        lens = D.row_lengths(dtype)
        assert len(set(lens)) == len(lens) and 3 * len(lens) <= D.SWEEP < D.PERIOD <= DEFAULT_CASES       # case i: dtype i % 3, length (i // 3) % len
        assert {v * vn for v in D.V_CHOICES} <= set(lens) and max(lens) == 1030 * vn
        assert {1, 7, 50, 1023} <= set(lens) and {2032 // (16 // vn), 2048 // (16 // vn)} <= set(lens)
    assert {100, 1028, 4100, 1016, 1024} <= set(D.row_lengths("bf16")) and {515, 508, 512} <= set(D.row_lengths("f32"))
    # the thresholds the lengths straddle: 64 (UNR - 1) for UNR = 2, 4, 8, and twice that per wave with the split
    for edge in (64, 192, 448):
        assert {edge - 1, edge, edge + 1} <= set(D.V_CHOICES) or {edge, edge + 1} <= set(D.V_CHOICES)
    assert D.split_per(1030) == 576 and D.wave_trace(0, 576, 4) == (2, 1) and D.split_per(129) == 128 and D.split_per(128) == 64
    assert D.wave_trace(0, 512, 8) == (1, 0) and D.wave_trace(0, 449, 8) == (1, 7) and D.wave_trace(0, 448, 8) == (0, 7)
    assert [D.unr_of(D.kmax_of(k), 1) for k in (1, 2, 3, 4, 5, 8, 9, 16)] == [8, 4, 2, 2, 1, 1, 1, 1] and D.unr_of(1, 2) == 4 and D.unr_of(2, 2) == 2


@pytest.mark.parametrize("what", ["decode", "encode", "ggrad"])
def test_generator_draws_every_promised_class_within_the_budget(what):
    gen, make, classes, promised = {"decode": (D.gen_decode_cases, D.decode_case, D.decode_classes, D.DECODE_PROMISED),
                                    "encode": (D.gen_encode_cases, D.encode_case, D.encode_classes, D.ENCODE_PROMISED),
                                    "ggrad": (D.gen_ggrad_cases, D.ggrad_case, D.ggrad_classes, D.GGRAD_PROMISED)}[what]
    cases = gen(DEFAULT_CASES, SEEDS[what])
    assert gen(10 * DEFAULT_CASES, SEEDS[what])[:DEFAULT_CASES] == cases and gen(7, SEEDS[what]) == cases[:7]      # case i does not depend on n
    seen = set()
    lengths = {dt: set() for dt in D.ROW_DTYPES}
    for d in cases:
        c = make(d)
        _sized(d, c, d["E"] * c["C"])
        lengths[d["dtype"]].add(d["M"])
        seen |= classes(d, c)
    D.check_promised(what, seen, promised, DEFAULT_CASES, DEFAULT_CASES)
    for dt in D.ROW_DTYPES:
        assert lengths[dt] >= set(D.row_lengths(dt)), (dt, sorted(set(D.row_lengths(dt)) - lengths[dt]))


# ---- the bucket orders against brute force ---------------------------------------------------------------------------------------------
def test_row_orders_against_brute_force():
    """chunk-major [C/c][E][c] and expert-sliced [E_loc/s][W][s][C], written out as loops over the output rows"""
    for E, C, chunk in ((3, 6, 2), (1, 5, 5), (8, 4, 1), (2, 9, 3)):
        want = [e * C + ci * chunk + r for ci in range(C // chunk) for e in range(E) for r in range(chunk)]
        assert D.row_order(E, C, "chunk", chunk=chunk).tolist() == want
    for E, C, s, W in ((8, 3, 2, 2), (6, 2, 1, 3), (4, 5, 4, 1), (24, 2, 3, 4), (1, 3, 1, 1)):
        e_loc = E // W
        want = [(w * e_loc + b * s + j) * C + l for b in range(e_loc // s) for w in range(W) for j in range(s) for l in range(C)]
        assert D.row_order(E, C, "sliced", s=s, W=W).tolist() == want
    assert D.row_order(3, 4, "plain").tolist() == list(range(12))
    # the orders a generated case takes are permutations of its plain rows
    for d in D.gen_decode_cases(DEFAULT_CASES, SEEDS["decode"]):
        c = D.decode_case(d)
        n = d["E"] * c["C"]
        if n:
            order = D.row_order(d["E"], c["C"], c["layout"], c["chunk"], c["s"], c["W"])
            assert sorted(order.tolist()) == list(range(n))
            assert torch.equal(_bits(c["buf"]), _bits(c["plain"][torch.from_numpy(order)]))


# ---- the references against the C oracle -----------------------------------------------------------------------------------------------
def test_decode_reference_against_the_oracle_bit_for_bit(oracle):
    n = 0
    for d in D.gen_decode_cases(2 * DEFAULT_CASES, SEEDS["decode"]):
        if d["M"] > ORACLE_M:
            continue
        c = D.decode_case(d)
        if c["C"] == 0:
            assert not bool(c["want"].float().abs().sum()), D.decode_tag(d, c)
            continue
        # the reference takes the plain rows whatever the case's bucket order: the kernel's buffer is a permutation of them (above)
        got = oracle.fast_decode(c["plain"].view(d["E"], c["C"], d["M"]), _crit(d, c, c["gates"]), is_postscore=True)
        assert _same_but_zero_sign(c["want"], got), D.decode_tag(d, c)
        n += 1
    assert n >= 40


def test_encode_reference_against_the_oracle_bit_for_bit(oracle):
    n = 0
    for d in D.gen_encode_cases(2 * DEFAULT_CASES, SEEDS["encode"]):
        if d["M"] > ORACLE_M:
            continue
        c = D.encode_case(d)
        if c["C"] == 0:
            assert c["want"].numel() == 0
            continue
        got = oracle.fast_encode(c["x"], _crit(d, c, c["gates"]), is_postscore=c["gates"] is None).view(-1, d["M"])
        assert _same_but_zero_sign(c["plain"], got), D.encode_tag(d, c)
        order = torch.from_numpy(D.row_order(d["E"], c["C"], c["layout"], c["chunk"], c["s"], c["W"]))
        assert torch.equal(_bits(c["want"]), _bits(c["plain"][order]))            # the output order: a host-side permutation of the plain result
        slot = c["slot"]
        assert int((slot >= 0).sum()) == int(D.keep_mask(c["idx"], c["loc"], c["C"]).sum())
        n += 1
    assert n >= 40


def test_gate_grad_reference_against_the_oracle(oracle):
    """the oracle adds the M products serially in fp32: within 1.01 M 2^-24 sum |row_i x_i| of float64, equal where every partial sum
    is exact (the integer class), exactly 0 for a dropped or masked entry"""
    n = exact = 0
    for d in D.gen_ggrad_cases(2 * DEFAULT_CASES, SEEDS["ggrad"]):
        if d["M"] > ORACLE_M:
            continue
        c = D.ggrad_case(d)
        it, lt = torch.from_numpy(c["idx"]), torch.from_numpy(c["loc"])
        for j in range(d["k"]):
            got = oracle.gate_grad(c["x"], c["buf"], it[j], lt[j], c["C"]).double()
            assert bool((got[~c["keep"][j]] == 0).all()) and bool((c["ref"][j][~c["keep"][j]] == 0).all())
            assert bool(((got - c["ref"][j]).abs() <= 1.01 * (d["M"] + 1) * 2.0 ** -24 * c["mag"][j]).all()), D.ggrad_tag(d, c)
            if d["integer"]:
                assert torch.equal(got, c["ref"][j]), D.ggrad_tag(d, c)
                exact += 1
        n += 1
    assert n >= 40 and exact >= 10


# ---- the gate-gradient bar ---------------------------------------------------------------------------------------------------------------
def test_the_summation_order_of_a_wave_stays_inside_the_gate_grad_bar():
    """lane-strided fp32 chains and the six-step butterfly, emulated in numpy fp32, against float64 for every generated gradient case: the
    emulation stays inside D.gate_grad_bound (so a correct kernel passes); a sum that loses its last pass does not (so the bar bites)"""
    lost = 0
    for d in D.gen_ggrad_cases(DEFAULT_CASES, SEEDS["ggrad"]):
        c = D.ggrad_case(d)
        emu = D.emulate_gate_grad(c["x"], c["buf"], c["idx"], c["loc"], c["C"], d["dtype"])
        assert emu.dtype == torch.float32 and bool((emu[~c["keep"]] == 0).all())
        err, bound = (emu.double() - c["ref"]).abs(), D.gate_grad_bound(c["mag"], d["M"])
        assert bool((err <= bound).all()), (D.ggrad_tag(d, c), float((err - bound).max()))
        if d["integer"]:
            assert torch.equal(emu.double(), c["ref"]), D.ggrad_tag(d, c)
        per = 64 * D.vec_elems(d["dtype"])
        if d["M"] % per == 0 and d["M"] > per and bool(c["keep"].any()) and not d["integer"]:
            cut = D.emulate_gate_grad(c["x"][:, :d["M"] - per], c["buf"][:, :d["M"] - per], c["idx"], c["loc"], c["C"], d["dtype"])
            assert float((((cut.double() - c["ref"]).abs() > bound) & c["keep"]).double().sum()) > 0.5 * float(c["keep"].sum()), D.ggrad_tag(d, c)
            lost += 1
    assert lost >= 3
