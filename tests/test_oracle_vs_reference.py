"""Pins the oracle against the reference.  Live, where the reference tree is present (python package imported from it + its C++
CPU kernels compiled into oracle/_ref/ by oracle/Makefile): tests/golden/make_golden*.py --check.  On any box: the plain-C port
of the reference's CPU kernels against what the reference's OWN compiled kernels wrote (tests/golden/ref_kernels.npz, made by
tests/golden/make_golden_ref_kernels.py); the rest of the live checks are replayed by tests/test_reference_checks.py and
tests/test_oracle_golden.py."""
import hashlib
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("TUTEL_REFERENCE", "/root/reference")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "tutel")), reason="reference tree not present on this box")
def test_oracle_equals_live_reference():
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "tutel_custom_kernel.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden.py"), "--check"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "tutel")), reason="reference tree not present on this box")
def test_oracle_expert_parallel_equals_live_reference_over_gloo():
    """The oracle's W-rank simulation (moe_forward_ep: routing per rank, all-to-all layout, experts on the received rows, return
    all-to-all, decode; cross-rank capacity for dropless and for inequivalent_tokens) against the reference RUNNING with W = 2 / 4
    ranks over gloo in this container: y, the rows each rank's experts receive, dispatch counts -- bit for bit."""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "tutel_custom_kernel.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_ep.py"), "--check"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _sha(t):
    t = t.contiguous()
    import torch
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()).hexdigest()


def _same_or_within_places(got, want, what, places=4):
    """the reference's bits, or -- on a host whose ATen CPU GEMMs / reductions accumulate in another order than the host the fixture
    was written on -- within `places` places of the largest element in the value's dtype, with a warning"""
    import torch
    g, w = got.double(), want.double()
    if torch.equal(g, w):
        return
    place = float(torch.finfo(got.dtype).eps) * max(float(w.abs().max()), 1e-30)
    worst = float((g - w).abs().max())
    assert worst <= places * place, f"{what}: max diff {worst:.3e} from the reference (one place of {got.dtype} here: {place:.3e})"
    warnings.warn(f"{what}: not the reference's bits on this host (max diff {worst:.3e}, within {places} places of {got.dtype})")


@pytest.mark.parametrize("T,M,H,E,k,cf,post,dts", [(512, 64, 32, 16, 2, 1.0, True, "float32"), (300, 64, 32, 12, 4, 1.0, False, "float32"),
                                                    (512, 64, 32, 16, 2, 0.5, True, "float32"), (512, 64, 32, 16, 1, 0.0, True, "float32"),
                                                    (512, 64, 64, 16, 2, 1.0, True, "bfloat16"), (256, 64, 32, 8, 2, 1.0, True, "float64"),
                                                    (4096, 2048, 64, 64, 2, 1.0, True, "float32")])
def test_reference_kernels_equal_the_port(T, M, H, E, k, cf, post, dts):
    """oracle/moe_oracle.c's fast_encode / fast_decode against the reference's OWN compiled CPU kernels (custom_kernel.cpp
    `invoke_cpu_fp32`, called as fast_dispatch.py:16-29,52-66 call it; oracle/ref_kernels.py): on the routing the reference's CPU
    path computed for these seeded inputs, the port's encoded rows and decoded tokens must be the reference kernels' bit for bit
    (sha256 of the bytes), and so must the whole layer's routing and encoded rows; y and l_aux are the reference-kernel layer's.  The last case is the headline's routing shape (64 experts, 4096 tokens, model_dim 2048) with a thin
    expert.  The port is the kernel pair bench.py's cpu_baseline times where oracle/_ref/ is absent."""
    import torch
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from oracle import moe_oracle as O
    z = np.load(os.path.join(GOLD, "ref_kernels.npz"))
    p = f"T{T}_M{M}_H{H}_E{E}_k{k}_cf{cf}_{'post' if post else 'pre'}_{dts}|"     # (make_golden_ref_kernels.py case_id)
    dtype = getattr(torch, dts)
    x, wg, w1, b1, w2, b2 = O.make_problem(T, M, H, E, dtype=dtype, seed=11)
    # (a reduction over millions of elements: its last place depends on the thread count, hence the relative bar)
    chk, want = float(sum(t.double().abs().sum() for t in (x, wg, w1, b1, w2, b2))), float(z[p + "in_checksum"][0])
    assert abs(chk - want) <= 1e-6 * abs(want), "seeded inputs must regenerate"
    idx, loc, gates = (torch.from_numpy(z[p + n]) for n in ("idx", "loc", "gates"))
    crit = (E, list(idx), list(loc), [g.to(dtype) for g in gates], int(z[p + "capacity"][0]), torch.from_numpy(z[p + "counts"]))
    enc = O.fast_encode(x.float(), crit, post)
    assert list(enc.shape) == list(z[p + "encode_shape"])
    assert _sha(enc) == str(z[p + "encode_sha256"][0]), "fast_encode differs from the reference's kernel"
    dec = O.fast_decode(enc, crit, post)
    assert list(dec.shape) == list(z[p + "decode_shape"])
    assert _sha(dec) == str(z[p + "decode_sha256"][0]), "fast_decode differs from the reference's kernel"
    # the whole layer through the port: its routing is the reference's, its encoded rows (layer dtype) the reference kernels' bits,
    # its output and l_aux the reference-kernel layer's
    y, l_aux, mine, st = O.moe_forward(x, wg, w1, b1, w2, b2, top_k=k, capacity_factor=cf, is_postscore=post)
    assert all(torch.equal(a.long(), b) for a, b in zip(mine[1], idx)) and all(torch.equal(a.long(), b) for a, b in zip(mine[2], loc)), \
        "expert ids / bucket slots differ from the reference's"
    assert int(mine[4]) == int(z[p + "capacity"][0]) and torch.equal(mine[5].long(), torch.from_numpy(z[p + "counts"]))
    assert _sha(st["encoded"]) == str(z[p + "layer_encoded_sha256"][0]), "encoded rows of the layer differ from the reference kernels'"
    if _sha(y) != str(z[p + "y_sha256"][0]):
        rows = torch.from_numpy(z[p + "y_rows"])
        _same_or_within_places(y.reshape(-1, y.shape[-1])[rows], torch.from_numpy(z[p + "y_sample"]).to(y.dtype), "layer output y")
    _same_or_within_places(l_aux.reshape(1), torch.tensor([float(z[p + "l_aux"][0])], dtype=torch.float64).to(l_aux.dtype), "l_aux")


def test_bench_cpu_baseline_times_the_reference_kernels():
    """bench.py's cpu_baseline leg (the only place outside tests/ and smoke() that may touch oracle/): with oracle/_ref/ present it
    reports kind "reference" (the reference's compiled kernels, compared bit for bit with the port before either is quoted) and carries
    the port's figure beside it; without it, kind "port" and says so.  A small shape here, the headline's on the GPU box."""
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import bench
    from oracle import ref_kernels as R
    r = bench.cpu_baseline(512, 256, 128, 16, 2, max_seconds=4.0)
    assert r["unit"] == "tokens/s" and r["value"] > 0 and r["cores"] >= 1
    assert r["port"]["kind"] == "port" and r["port"]["value"] > 0
    if R.available():
        assert r["kind"] == "reference" and "oracle/_ref" in r["kind_note"] and "bit for bit" in r["sample"]
    else:
        assert r["kind"] == "port" and r["value"] == r["port"]["value"] and "oracle/_ref/ is not on this box" in r["kind_note"]
