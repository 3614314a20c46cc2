"""Seeded fuzzers of csrc/dispatch.hip over row lengths and launch shapes, each a `run_*` function returning its failing cases.  The
references (tests/_dispatch_fuzz.py) are numpy fp32 / float64 restatements of the operations' definitions on the same rounded inputs;
tests/test_dispatch_fuzz_cpu.py pins them against the C oracle.  The row lengths straddle every entry threshold of the unrolled loops of
encode and decode, with and without the two-waves-per-token split, every partial last wave and the scalar tail; k takes every KMAX
instantiation and the any-k kernel; capacities from "nothing dropped" to 0.
  decode   tutel_amd_fast_decode in ALL FOUR values of TUTEL_OPT_DECODE (k > 16: the any-k kernel, once), the three bucket orders: equal to the
           reference by value, and by bits wherever the reference is non-zero (the convention of test_ops_gpu.py::test_encode_decode_vs_oracle)
  encode   tutel_amd_fast_encode, copy and gated, the three output orders: bit for bit; TUTEL_OPT_GEMM_STORE 0 and -1 the same bits
  ggrad    tutel_amd_gate_grad (what ops.gate_grad calls; bf16, fp16, fp32) against float64 within F.gate_grad_bound, torch.equal where the
           operands are small integers, exactly 0 for dropped and masked entries
The C entry points are called as tutel_amd/ops.py calls them, so that every operand sits in a guard band (_packed_fuzz.moated: NaN around
the inputs, a masked id / location 0 / an empty slot around the index tables, a sentinel around the outputs, every band intact afterwards).
No case is skipped or shrunk at run time, and a refusal of a drawn case is a failure.  The default run takes 96 cases each, --runslow 960;
`python tests/test_dispatch_fuzz_gpu.py [cases] [seed] [what]` runs any length and writes dispatch_<what>_fuzz_<seed>.json into the
repository's ignored `*_out/` directory."""
import json
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

import _dispatch_fuzz as D   # noqa: E402
import _packed_fuzz as F     # noqa: E402

DEFAULT_CASES = 96
SEEDS = {"decode": 8080, "encode": 8081, "ggrad": 8082}


def _fail(bad, tag, ex, verbose):
    bad.append(tag + " :: " + (str(ex) or type(ex).__name__)[:300].replace("\n", " "))
    if verbose:
        print("FAIL", bad[-1], flush=True)


def _abi():
    from tutel_amd import _lib
    return _lib.lib(), {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(L, rc, what):
    assert rc == 0, f"{what} refused a drawn case (status {rc}): {L.tutel_amd_last_error().decode('utf-8', 'replace')}"


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _first_difference(got, want):
    ne = (_bits(got) != _bits(want)).nonzero()
    r, c = int(ne[0][0]), int(ne[0][1])
    return f"{ne.shape[0]} elements differ, first row {r} column {c}: {float(got[r, c])!r} vs {float(want[r, c])!r}"


def _tables(c):
    """idx and loc on the device, a masked id and location 0 in their bands: what a read past a table follows stays inside the buffers"""
    return (F.moated(torch.from_numpy(c["idx"]), fill=-1, device="cuda"), F.moated(torch.from_numpy(c["loc"]), fill=0, device="cuda"))


def _out(shape, dtype):
    return F.moated(torch.full(shape, 3.0, dtype=dtype, device="cuda"), fill=F.OUT_FILL)


def run_decode_fuzz(n_cases, seed, verbose=False):
    """tutel_amd_fast_decode against D.ref_decode.  Every case with k <= 16 runs in all four launch shapes.  -> list of failure descriptions"""
    from tutel_amd import _lib, ops
    L, DT = _abi()
    bad, seen, t0 = [], set(), time.time()
    try:
        for d in D.gen_decode_cases(n_cases, seed):
            tag = D.decode_tag(d)
            try:
                c = D.decode_case(d)
                tag = D.decode_tag(d, c)
                seen |= D.decode_classes(d, c)
                T, E, k, M, C = d["T"], d["E"], d["k"], d["M"], c["C"]
                dtype = D.DTYPES[d["dtype"]]
                buf, gates = F.moated(c["buf"], device="cuda"), F.moated(c["gates"], device="cuda") if c["gates"] is not None else None
                idx, loc = _tables(c)
                want = c["want"].cuda()
                nonzero = want.float() != 0
                for mode in (range(4) if k <= 16 else [-1]):
                    ops.set_option(_lib.OPT_DECODE, mode)
                    out = _out([T, M], dtype)
                    _ok(L, L.tutel_amd_fast_decode(buf.data_ptr(), DT[dtype], idx.data_ptr(), loc.data_ptr(), gates.data_ptr() if gates is not None else None,
                                                   DT[gates.dtype] if gates is not None else 0, T, M, k, C, E, c["chunk"], c["s"], c["W"], out.data_ptr(),
                                                   _stream()), "tutel_amd_fast_decode")
                    F.moat_intact(out, f"out (TUTEL_OPT_DECODE={mode})")
                    # values, then bits except where the reference is a zero of either sign
                    if not (torch.equal(out.float(), want.float()) and bool(((_bits(out) == _bits(want)) | ~nonzero).all())):
                        raise AssertionError(f"TUTEL_OPT_DECODE={mode}: " + _first_difference(out.cpu(), c["want"]))
                for what, t in (("buf", buf), ("gates", gates), ("idx", idx), ("loc", loc)):
                    if t is not None:
                        F.moat_intact(t, what)
            except Exception as ex:  # noqa: BLE001 -- the sweep reports every failing case
                _fail(bad, tag, ex, verbose)
            if verbose and (d["case"] + 1) % 100 == 0:
                print(f"{d['case'] + 1} dispatch decode cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    finally:
        ops.set_option(_lib.OPT_DECODE, -1)
    D.check_promised("dispatch decode", seen, D.DECODE_PROMISED, n_cases, DEFAULT_CASES)
    return bad


def run_encode_fuzz(n_cases, seed, verbose=False):
    """tutel_amd_fast_encode against D.ref_encode, bit for bit, with plain (TUTEL_OPT_GEMM_STORE = 0) and write-through (-1) row stores.
    -> list of failure descriptions"""
    from tutel_amd import _lib, ops
    L, DT = _abi()
    bad, seen, t0 = [], set(), time.time()
    try:
        for d in D.gen_encode_cases(n_cases, seed):
            tag = D.encode_tag(d)
            try:
                c = D.encode_case(d)
                tag = D.encode_tag(d, c)
                seen |= D.encode_classes(d, c)
                T, E, M, C = d["T"], d["E"], d["M"], c["C"]
                dtype = D.DTYPES[d["dtype"]]
                n_slots = E * C
                x, gates = F.moated(c["x"], device="cuda"), F.moated(c["gates"], device="cuda") if c["gates"] is not None else None
                slot = F.moated(torch.from_numpy(c["slot"]).int() if n_slots else torch.full([1], -1, dtype=torch.int32), fill=-1, device="cuda")
                want = c["want"].cuda()
                for store in (0, -1):
                    ops.set_option(_lib.OPT_GEMM_STORE, store)
                    out = _out([max(n_slots, 1), M], dtype)
                    _ok(L, L.tutel_amd_fast_encode(x.data_ptr(), DT[dtype], slot.data_ptr(), gates.data_ptr() if gates is not None else None,
                                                   DT[gates.dtype] if gates is not None else 0, T, M, n_slots, C, E, c["chunk"], c["s"], c["W"], out.data_ptr(),
                                                   _stream()), "tutel_amd_fast_encode")
                    F.moat_intact(out, f"out (TUTEL_OPT_GEMM_STORE={store})")
                    if n_slots == 0:
                        assert bool((out == 3.0).all()), "an encode of no slots wrote a row"
                    elif not torch.equal(_bits(out), _bits(want)):
                        raise AssertionError(f"TUTEL_OPT_GEMM_STORE={store}: " + _first_difference(out.cpu(), c["want"]))
                for what, t in (("x", x), ("gates", gates), ("slot_map", slot)):
                    if t is not None:
                        F.moat_intact(t, what)
            except Exception as ex:  # noqa: BLE001
                _fail(bad, tag, ex, verbose)
            if verbose and (d["case"] + 1) % 100 == 0:
                print(f"{d['case'] + 1} dispatch encode cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    finally:
        ops.set_option(_lib.OPT_GEMM_STORE, -1)
    D.check_promised("dispatch encode", seen, D.ENCODE_PROMISED, n_cases, DEFAULT_CASES)
    return bad


def run_ggrad_fuzz(n_cases, seed, verbose=False):
    """tutel_amd_gate_grad against float64: |got - ref| <= 1.01 (M / 64 + 16) 2^-24 sum |row_i x_i| (D.gate_grad_bound: derived from the
    length of a lane's chain, not tuned to the kernel); equal to the reference where the operands are integers from -3 to 3 (every partial
    sum is exact); exactly 0 for a dropped or masked entry; ops.gate_grad the same bits.  -> list of failure descriptions"""
    from tutel_amd import ops
    L, DT = _abi()
    bad, seen, t0 = [], set(), time.time()
    for d in D.gen_ggrad_cases(n_cases, seed):
        tag = D.ggrad_tag(d)
        try:
            c = D.ggrad_case(d)
            tag = D.ggrad_tag(d, c)
            seen |= D.ggrad_classes(d, c)
            T, k, M, C = d["T"], d["k"], d["M"], c["C"]
            dtype = D.DTYPES[d["dtype"]]
            x, buf = F.moated(c["x"], device="cuda"), F.moated(c["buf"], device="cuda")
            idx, loc = _tables(c)
            out = F.moated(torch.full([k, T], 3.0, device="cuda"), fill=F.OUT_FILL)
            _ok(L, L.tutel_amd_gate_grad(x.data_ptr(), buf.data_ptr(), DT[dtype], idx.data_ptr(), loc.data_ptr(), T, M, k, C, out.data_ptr(), _stream()),
                "tutel_amd_gate_grad")
            for what, t in (("ggate", out), ("x", x), ("buf", buf), ("idx", idx), ("loc", loc)):
                F.moat_intact(t, what)
            got = out.cpu()
            assert bool((got[~c["keep"]] == 0).all()), "the gate gradient of a dropped / masked entry is not exactly zero"
            err, bound = (got.double() - c["ref"]).abs(), D.gate_grad_bound(c["mag"], M)
            if not bool((err <= bound).all()):       # (NaN-safe: a NaN fails the comparison)
                j, t = np.unravel_index(int(torch.nan_to_num(err - bound, nan=float("inf")).argmax()), err.shape)
                raise AssertionError(f"ggate[{j}][{t}] = {float(got[j, t])!r} vs {float(c['ref'][j, t])!r}: error {float(err[j, t]):.3e}, bound {float(bound[j, t]):.3e}")
            if d["integer"]:
                assert torch.equal(got.double(), c["ref"]), "integer operands: the sums are exact in fp32, the result is not"
            assert torch.equal(ops.gate_grad(x, buf, idx, loc, C), out), "ops.gate_grad gave other bits than the entry point it calls"
        except Exception as ex:  # noqa: BLE001
            _fail(bad, tag, ex, verbose)
        if verbose and (d["case"] + 1) % 100 == 0:
            print(f"{d['case'] + 1} dispatch gate-grad cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    D.check_promised("dispatch gate gradient", seen, D.GGRAD_PROMISED, n_cases, DEFAULT_CASES)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_dispatch_decode_fuzz_every_launch_shape_vs_reference(n_cases):
    bad = run_decode_fuzz(n_cases, seed=SEEDS["decode"])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_dispatch_encode_fuzz_every_output_order_vs_reference(n_cases):
    bad = run_encode_fuzz(n_cases, seed=SEEDS["encode"])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_dispatch_gate_grad_fuzz_vs_float64(n_cases):
    bad = run_ggrad_fuzz(n_cases, seed=SEEDS["ggrad"])
    assert not bad, "\n".join(bad[:20])


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10 * DEFAULT_CASES
    what = sys.argv[3] if len(sys.argv) > 3 else "decode"
    runners = {"decode": run_decode_fuzz, "encode": run_encode_fuzz, "ggrad": run_ggrad_fuzz}
    assert what in runners, f"what: one of {sorted(runners)}"
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else SEEDS[what]
    t_start = time.time()
    failed = runners[what](n, sd, verbose=True)
    # the run-record directory of tests/test_fuzz_gpu.py's driver: the `*_out/` entry of .gitignore
    out_dir = os.path.join(ROOT, next(ln.strip().rstrip("/") for ln in open(os.path.join(ROOT, ".gitignore")) if ln.strip().endswith("_out/")))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"dispatch_{what}_fuzz_{sd}.json"), "w") as f:
        json.dump(dict(source="tests/test_dispatch_fuzz_gpu.py", cases=n, seed=sd, seconds=round(time.time() - t_start, 2), failed=failed), f, indent=1)
    print("cases", n, "failed", len(failed))
    sys.exit(1 if failed else 0)
