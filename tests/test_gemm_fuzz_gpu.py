"""Seeded fuzzer of the padded grouped GEMM's gated form, tutel_amd_expert_gemm_glu (ops.expert_gemm(..., mul=G): the SwiGLU forward,
experts/llama_ffn.py, and the ReLU backward of padded ffn training, experts/ffn.py), of the fused gate/up kernel, and of the strided
[W, E_loc, C, .] all-to-all addressing of A, D and G -- element by element against float64 (tests/_gemm_fuzz.py: ref_glu, glu_bound),
through every forced kernel choice and store policy.  Beside the bound, checks that need no tolerance:
  mul_mask   G in {0, 1}: the gated output is the plain launch's where G = 1, bit for bit, and +-0 where G = 0
  mul_pow2   G = +-2^p, another value in every neighbouring row and column: the gated output is the plain launch's times G, exactly
             (fp16: where the pre-gating magnitude is at least 2^-13; at most 0.2 % of a case may lie below)
  forced     every forced (impl, tile, store) launch equals the automatic one bit for bit
  gate_up    the fused kernel equals expert_gemm(act) followed by expert_gemm(mul=...) bit for bit
  inplace    G == D gives the bits of the out-of-place launch
  sentinels  rows past ceil(count / row_align) * row_align and the gap rows of the `ep` layout keep their bytes; G holds NaN there
The default run takes 150 cases, --runslow 1500; `python tests/test_gemm_fuzz_gpu.py [cases] [seed]` runs any length and writes
glu_fuzz_<seed>.json beside the records of tests/test_fuzz_gpu.py (the repository's ignored `*_out/` directory).  A failure's tag names
its case and seed: run_glu_fuzz(case + 1, seed, which=[case]) runs it alone."""
import json
import os
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _gemm_fuzz as F   # noqa: E402

DEFAULT_CASES = 150
SEED = 7080
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _first(mask):
    i = mask.nonzero()[0]
    return tuple(int(v) for v in i)


def _same_bits(x, y, mask, what):
    """x, y logical [E, R, N]; mask [E, R, N] bool (None: everywhere)"""
    ne = _bits(x) != _bits(y)
    if mask is not None:
        ne &= mask
    if bool(ne.any()):
        e, r, n = _first(ne)
        raise AssertionError(f"{what}: {int(ne.sum())} elements differ, first [{e}][{r}][{n}]: {float(x[e, r, n])} vs {float(y[e, r, n])}")


def _run_case(ops, _lib, d, worst):
    dtype = F.DTYPES[d["dtype"]]
    E, R, N, W, form, km, act = d["E"], d["R"], d["N"], d["W"], d["form"], d["kmajor"], d["act"]
    ep = d["layout"] == "ep"
    a, w, bias, G, w_up = F.make_glu_inputs(d)
    limits = F.row_limits(d)
    kept = torch.zeros([E, R, 1], dtype=torch.bool)
    for e in range(E):
        kept[e, :limits[e]] = True
    kept = kept.expand(E, R, N)
    a_dev = (F.to_ep(a, W) if ep else a).cuda()
    a_layout, d_layout = F.ep_layouts(d) if ep else (None, (R * N, 0, R, N))
    phys = [W, E, R // W + 1, N] if ep else [E, R, N]
    wd, bd = w.cuda(), bias.cuda() if bias is not None else None
    counts = torch.tensor(d["row_counts"], dtype=torch.int32).cuda() if d["row_counts"] is not None else None
    G_dev = None
    if G is not None:
        Gn = G.clone()
        Gn[~kept] = NAN            # a kernel that consumes a row past the limit, or a gap row, shows up in a kept row
        G_dev = (F.to_ep(Gn, W, gap=1, fill=NAN) if ep else Gn).cuda()

    def split(p):
        return F.from_ep(p, W, gap=1) if ep else (p, None)

    def launch(mul=None, act_=act, weight=wd, bias_=bd, into=None, what=""):
        """one launch -> the logical [E, R, N] output on the host; every byte the launch must not write is checked against what the
        buffer held before"""
        if into is None and not ep and counts is None:
            return ops.expert_gemm(a_dev, weight, bias_, km, act=act_, mul=mul).cpu()
        if into is None:
            into = torch.full(phys, F.SENTINEL, dtype=dtype, device="cuda")
        before, gap_before = split(into.cpu())
        ops.expert_gemm(a_dev, weight, bias_, km, act=act_, E_loc=E, R=R, a_layout=a_layout, out=into, d_layout=d_layout, row_counts=counts,
                        row_align=d["row_align"], mul=mul)
        out, gap = split(into.cpu())
        _same_bits(out, before, ~kept, what + "rows past the aligned count were written")
        if ep:
            assert torch.equal(_bits(gap), _bits(gap_before)), what + "a gap row of the all-to-all layout was written"
        return out

    def main(what=""):
        if form == "gate_up":
            return ops.expert_gemm_gate_up(a_dev, wd, w_up.cuda(), act=act, row_counts=counts, row_align=d["row_align"]).cpu()
        return launch(mul=G_dev, what=what)

    auto = main("automatic kernel: ")
    for key, v in ((_lib.OPT_GEMM_IMPL, d["impl"]), (_lib.OPT_GEMM_TILE, d["tile"]), (_lib.OPT_GEMM_STORE, d["store"])):
        ops.set_option(key, v)
    forced = main("forced kernel: ")
    _same_bits(forced, auto, kept, "the forced kernel against the automatic one")
    if d["inplace"]:
        buf = G_dev.clone()
        _same_bits(launch(mul=buf, into=buf, what="in place: "), auto, kept, "G == D (in place) against the out-of-place launch")
    for key in (_lib.OPT_GEMM_IMPL, _lib.OPT_GEMM_TILE, _lib.OPT_GEMM_STORE):
        ops.set_option(key, -1)

    # ---- float64, every kept element ------------------------------------------------------------------------------------------------
    if form == "gate_up":
        Gb = F.ref_gate(a, w, act, dtype)
        ref, v = F.ref_glu(a, w_up, None, True, "none", Gb, dtype)
    else:
        Gb = G
        ref, v = F.ref_glu(a, w, bias, km, act, G, dtype)
    bound = F.glu_bound(ref, Gb, dtype)
    err = (auto.double() - ref).abs()
    over = ~(err <= bound) & kept       # (NaN-safe: a NaN fails the comparison)
    if bool(kept.any()):
        ratio = float(torch.nan_to_num((err / bound)[kept], nan=float("inf")).max())
        if ratio > worst[0]:
            worst[0], worst[1] = ratio, d["case"]
    if bool(over.any()):
        e, r, n = _first(over)
        raise AssertionError(f"[{e}][{r}][{n}]: {float(auto[e, r, n])} vs {float(ref[e, r, n])} (|err| {float(err[e, r, n]):.3e}, bound "
                             f"{float(bound[e, r, n]):.3e}; {int(over.sum())} elements beyond the bound)")

    # ---- exact --------------------------------------------------------------------------------------------------------------------
    if form in ("mul_mask", "mul_pow2"):
        plain = launch(mul=None, what="plain launch: ")
        if form == "mul_mask":
            _same_bits(auto, plain, kept & (G == 1), "G = 1: the gated output against the plain launch's")
            nz = ((_bits(auto) & 0x7fff) != 0) & kept & (G == 0)
            assert not bool(nz.any()), f"G = 0 did not give an exact zero at {_first(nz)}"
        else:
            left = F.pow2_left_out(v, dtype)
            share = float((left & kept).double().mean())
            assert share <= F.POW2_LEFT_OUT_CAP, f"{share:.3%} of the elements lie below 2^-13: the case leaves out more than the cap"
            _same_bits(auto, (plain.float() * G.float()).to(dtype), kept & ~left, "G = +-2^p: the gated output against the plain launch's times G")
    if form == "gate_up":
        g = launch(mul=None, bias_=None, what="act launch: ")
        two = launch(mul=g.cuda(), act_="none", weight=w_up.cuda(), bias_=None, what="gated launch: ")
        _same_bits(auto, two, kept, "the fused gate/up kernel against the act launch followed by the gated launch")


def run_glu_fuzz(n_cases, seed, which=None, verbose=False, stats=None):
    """-> list of failure descriptions.  which: the case numbers to run (None: all; the edge classes are then checked too)"""
    from tutel_amd import ops, _lib
    bad, seen, t0, worst = [], set(), time.time(), [0.0, -1]
    for d in F.gen_glu_cases(n_cases, seed):
        seen |= F.glu_classes(d)
        if which is not None and d["case"] not in which:
            continue
        try:
            _run_case(ops, _lib, d, worst)
        except Exception as ex:  # noqa: BLE001 -- the sweep reports every failing case
            bad.append(F.glu_tag(d) + " :: " + (str(ex) or type(ex).__name__)[:300].replace("\n", " "))
            if verbose:
                print("FAIL", bad[-1], flush=True)
        finally:
            for key in (_lib.OPT_GEMM_IMPL, _lib.OPT_GEMM_TILE, _lib.OPT_GEMM_STORE):
                ops.set_option(key, -1)
        if verbose and (d["case"] + 1) % 100 == 0:
            print(f"{d['case'] + 1} glu cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    if stats is not None:
        stats.update(worst_err_over_bound=worst[0], worst_case=worst[1], seconds=time.time() - t0)
    if which is None:
        F.check_promised("glu", seen, F.GLU_PROMISED, n_cases, DEFAULT_CASES)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_gated_gemm_and_strided_layouts_fuzz_vs_float64(n_cases):
    bad = run_glu_fuzz(n_cases, seed=SEED)
    assert not bad, "\n".join(bad[:20])


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10 * DEFAULT_CASES
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else SEED
    st = {}
    failed = run_glu_fuzz(n, sd, verbose=True, stats=st)
    # the run-record directory of tests/test_fuzz_gpu.py's driver: the `*_out/` entry of .gitignore
    out_dir = os.path.join(ROOT, next(ln.strip().rstrip("/") for ln in open(os.path.join(ROOT, ".gitignore")) if ln.strip().endswith("_out/")))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"glu_fuzz_{sd}.json"), "w") as f:
        json.dump(dict(source="tests/test_gemm_fuzz_gpu.py", cases=n, seed=sd, failed=failed, **st), f, indent=1)
    print("cases", n, "failed", len(failed), "worst |err| / bound %.3f (case %d)" % (st["worst_err_over_bound"], st["worst_case"]), "%.1f s" % st["seconds"])
    sys.exit(1 if failed else 0)
