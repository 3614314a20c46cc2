"""Generates tests/golden/ref_kernels.npz: the reference's OWN compiled CPU kernels (oracle/_ref/tutel_custom_kernel.so, see
oracle/Makefile and oracle/ref_kernels.py) on the cases of tests/test_oracle_vs_reference.py::test_reference_kernels_equal_the_port.
Per case: the routing the reference's CPU path computed (expert ids, bucket slots, gates, capacity, dispatch counts), the sha256
of what its fast_encode (x in fp32 -> [E, C, M]) and fast_decode (those rows -> [T, M]) returned, and the whole layer run through
its kernels (encoded rows, y, l_aux), so that the plain-C port can be checked against them on any box.  The inputs are seeded (oracle/moe_oracle.py make_problem) and carry a checksum.

    make -C oracle && python tests/golden/make_golden_ref_kernels.py [--check]
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

# (T, M, H, E, k, capacity_factor, is_postscore, dtype): the test's parametrization
CASES = [(512, 64, 32, 16, 2, 1.0, True, "float32"), (300, 64, 32, 12, 4, 1.0, False, "float32"),
         (512, 64, 32, 16, 2, 0.5, True, "float32"), (512, 64, 32, 16, 1, 0.0, True, "float32"),
         (512, 64, 64, 16, 2, 1.0, True, "bfloat16"), (256, 64, 32, 8, 2, 1.0, True, "float64"),
         (4096, 2048, 64, 64, 2, 1.0, True, "float32")]
SEED = 11
SAMPLE_ROWS = 16
OUT = os.path.join(HERE, "ref_kernels.npz")


def case_id(T, M, H, E, k, cf, post, dts):
    return f"T{T}_M{M}_H{H}_E{E}_k{k}_cf{cf}_{'post' if post else 'pre'}_{dts}"


def sha256(t):
    t = t.contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()).hexdigest()


def checksum(tensors):
    return float(sum(t.double().abs().sum() for t in tensors))


def reference_case(T, M, H, E, k, cf, post, dts):
    from oracle import moe_oracle as O, ref_kernels as R
    x, wg, w1, b1, w2, b2 = O.make_problem(T, M, H, E, dtype=getattr(torch, dts), seed=SEED)
    y, l_aux, crit, st = R.moe_forward(x, wg, w1, b1, w2, b2, top_k=k, capacity_factor=cf, is_postscore=post)
    enc = R.fast_encode(x.float(), crit, post)
    dec = R.fast_decode(enc, crit, post)
    E_, idx, loc, gates, C, cnt = crit
    rows = torch.randperm(y.reshape(-1, y.shape[-1]).shape[0], generator=torch.Generator().manual_seed(0))[:SAMPLE_ROWS].sort().values
    p = case_id(T, M, H, E, k, cf, post, dts) + "|"
    return {p + "in_checksum": np.array([checksum([x, wg, w1, b1, w2, b2])]),
            p + "idx": torch.stack([i.to(torch.int64) for i in idx]).numpy(),
            p + "loc": torch.stack([l.to(torch.int64) for l in loc]).numpy(),
            p + "gates": torch.stack([g.to(torch.float64) for g in gates]).numpy(),
            p + "capacity": np.array([int(C)]), p + "counts": cnt.to(torch.int64).numpy(),
            p + "encode_sha256": np.array([sha256(enc)]), p + "decode_sha256": np.array([sha256(dec)]),
            p + "encode_shape": np.array(list(enc.shape)), p + "decode_shape": np.array(list(dec.shape)),
            # the whole layer through the reference's kernels: encoded rows in the layer dtype, output y (digest + a seeded sample of
            # rows, for hosts whose ATen GEMMs round differently), l_aux
            p + "layer_encoded_sha256": np.array([sha256(st["encoded"])]), p + "y_sha256": np.array([sha256(y)]),
            p + "y_rows": rows.numpy(), p + "y_sample": y.reshape(-1, y.shape[-1])[rows].double().numpy(),
            p + "l_aux": np.array([float(l_aux)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute and compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    from oracle import ref_kernels as R
    if not R.available():
        sys.exit("oracle/_ref/tutel_custom_kernel.so is missing: `make -C oracle` where the reference tree is present")
    out = {}
    for c in CASES:
        out.update(reference_case(*c))
    if args.check:
        z = np.load(OUT)
        bad = sorted(set(z.files) ^ set(out)) + [n for n in out if n in z.files and not np.array_equal(z[n], out[n])]
        print("ref-kernels fixture: %d mismatches %s" % (len(bad), bad[:10]))
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
