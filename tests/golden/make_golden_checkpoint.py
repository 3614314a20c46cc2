"""Generates tests/golden/checkpoint_reference_tools.npz by running the REFERENCE's own checkpoint CLI tools
(`python -m tutel.checkpoint.gather` / `.scatter` of the reference tree, TUTEL_REFERENCE) on the per-rank checkpoints of
tests/test_checkpoint_cpu.py::test_gather_scatter_round_trip_and_reference_tools: per case the full checkpoint the reference's
gather wrote and, where the test re-shards, the per-rank files its scatter wrote (namespace unwrapped), plus an input checksum.

    make -C oracle && python tests/golden/make_golden_checkpoint.py [--check]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TUTEL_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "checkpoint_reference_tools.npz")
CASES = [(4, 8, ""), (2, 2, "model/state"), (4, 2, "")]   # (size, E_global, namespace): the test's parametrization


def case_id(size, E_global, namespace):
    return f"{size}_{E_global}_{namespace.replace('/', '.') or '-'}"


def states_checksum(states):
    return float(sum(t.double().abs().sum() for sd in states for t in sd.values()))


def reference_case(size, E_global, namespace, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_checkpoint_cpu import _rank_states
    states = _rank_states(size, E_global)

    def wrap(sd):
        for package in reversed([p for p in namespace.split("/") if p]):
            sd = {package: sd}
        return sd

    def unwrap(obj):
        for package in namespace.split("/"):
            if package:
                obj = obj[package]
        return obj

    os.makedirs(os.path.join(tmp, "in"))
    inputs = os.path.join(tmp, "in", "r{rank}-of-{size}.pt")
    for r, sd in enumerate(states):
        torch.save(wrap(sd), inputs.format(rank=r, size=size))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REF, os.path.join(ROOT, "oracle", "_ref")]))
    full = os.path.join(tmp, "ref_full.pt")
    subprocess.check_call([sys.executable, "-m", "tutel.checkpoint.gather", f"--input_size={size}", f"--inputs={inputs}",
                           f"--output={full}", f"--namespace={namespace}"], env=env, cwd=tmp, stdout=subprocess.DEVNULL)
    p = case_id(size, E_global, namespace) + "|"
    out = {p + "in_checksum": np.array([states_checksum(states)])}
    out.update({p + "gather|" + k: v.numpy() for k, v in unwrap(torch.load(full)).items()})
    other = size // 2
    if E_global % other == 0:
        subprocess.check_call([sys.executable, "-m", "tutel.checkpoint.scatter", f"--output_size={other}", f"--input={full}",
                               f"--outputs={tmp}/refhalf/r{{rank}}-of-{{size}}.pt", f"--namespace={namespace}"],
                              env=env, cwd=tmp, stdout=subprocess.DEVNULL)
        for r in range(other):
            sd = unwrap(torch.load(f"{tmp}/refhalf/r{r}-of-{other}.pt"))
            out.update({p + f"scatter{r}|" + k: v.numpy() for k, v in sd.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute and compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(REF, "tutel")):
        sys.exit(f"the reference tree is not at {REF} (set TUTEL_REFERENCE)")
    out = {}
    for c in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            out.update(reference_case(*c, tmp))
    if args.check:
        z = np.load(OUT)
        bad = sorted(set(z.files) ^ set(out)) + [n for n in out if n in z.files and not np.array_equal(z[n], out[n])]
        print("checkpoint fixture: %d mismatches %s" % (len(bad), bad[:10]))
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
