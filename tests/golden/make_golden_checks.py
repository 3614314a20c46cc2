"""Generates tests/golden/reference_checks.npz: the observations of tests/_reference_checks.py (the function-level and drop-in
surface checks of make_golden.py --check, the tutel.net check of make_golden_ep.py --check, over gloo) made with the REFERENCE itself (python package from TUTEL_REFERENCE + its C++ CPU
kernels compiled into oracle/_ref/), plus the digests of the softmax scores they route on.  tests/test_reference_checks.py replays them against
this repository's oracle and product on any box.  --check compares both sides live instead of writing.

    make -C oracle && python tests/golden/make_golden_checks.py [--check]
"""
import argparse
import logging
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TUTEL_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "reference_checks.npz")
# the reference package is also called `tutel`: it must win over the repo's alias package
sys.path = [REF, os.path.join(ROOT, "oracle", "_ref")] + [p for p in sys.path if os.path.abspath(p or ".") != ROOT] + [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _reference_checks as C  # noqa: E402


class ReferenceImpl:
    def __init__(self):
        logging.disable(logging.CRITICAL)
        import tutel
        assert os.path.abspath(tutel.__file__).startswith(REF), tutel.__file__
        from tutel import moe
        from tutel.impls import losses
        from tutel.jit_kernels.gating import fast_cumsum_sub_one
        from tutel.impls.jit_compiler import tutel_custom_kernel
        self.moe, self.losses, self.cumsum, self.ck = moe, losses, fast_cumsum_sub_one, tutel_custom_kernel

    def route(self, scores, k, cf, norm):
        return self.moe.top_k_routing(scores, k, capacity_factor=cf, normalize_gate=norm)

    def encode(self, x, crit, post):
        return self.moe.fast_encode(x, crit, post)

    def decode(self, y, crit, post):
        return self.moe.fast_decode(y, crit, post)

    def cumsum_sub_one(self, m):
        return self.cumsum(m)

    def gate_grad(self, x, buf, idx, loc, C_):
        gg = torch.empty([x.shape[0]])
        self.ck.invoke_cpu_fp32([gg, idx, loc, x, buf], [x.shape[0], x.shape[1], C_], 2)
        return gg

    def dispatch(self, E, C_, M, idx, loc, gates, post, x):
        d = self.moe.fast_dispatcher(E, C_, M, torch.float32)
        d.update(idx, loc, gates, capacity=C_, is_postscore=post)
        enc = d.encode(x)
        return enc, d.decode(enc.view(E, -1, M))

    def gshard_loss(self, scores, ids):
        return self.losses.gshard_loss(scores, ids)

    def load_importance_loss(self, *a):
        return self.losses.load_importance_loss(*a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare the reference and this repository live instead of writing the fixture")
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(REF, "tutel")):
        sys.exit(f"the reference tree is not at {REF} (set TUTEL_REFERENCE)")
    scores = C.score_inputs()
    ref = ReferenceImpl()
    obs = {**C.function_checks(ref, scores), **C.surface_checks(ref.moe.moe_layer)}
    rec = C.to_record(obs)
    for r, rr in C.run_net("reference").items():
        rec.update({f"net{r}:" + k: v for k, v in rr.items()})
    if args.check:
        stored = C.from_record(rec)
        mine = {**C.function_checks(C.OracleImpl(), scores), **C.surface_checks(C.product_build())}
        bad = [(n, C.compare(n, v, m, stored[n], live=True) if n in stored else "not observed with the reference") for n, (v, m) in mine.items()]
        bad = [b for b in bad if b[1]] + [(n, "missing") for n in stored if n not in mine]
        with tempfile.TemporaryDirectory() as tmp:
            np.savez(os.path.join(tmp, "ref.npz"), **rec)
            for r, (net_bad, n) in sorted(C.run_net("product", os.path.join(tmp, "ref.npz")).items()):
                bad += [(f"rank {r}: {b}", "") for b in net_bad]
                print(f"tutel.net rank {r}: {len(net_bad)} mismatches of {n}")
        for n, why in bad:
            print("MISMATCH:", n, why)
        print("reference checks: %d mismatches" % len(bad))
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **rec, **{"scores|" + k: np.array([C.digest(v)], dtype="S64") for k, v in scores.items()})
    print("wrote", OUT, len(obs), "observations")


if __name__ == "__main__":
    main()
