"""TEST-ONLY pieces shared by the fuzzer of the padded grouped GEMM's gated form and strided layouts (tests/test_gemm_fuzz_gpu.py) and
its GPU-free checks (tests/test_gemm_fuzz_cpu.py): the seeded case generator, the edge classes it promises to draw, the inputs of a
case in their logical [E, R, .] form and in the [W, E, C, .] all-to-all addressing, and the float64 reference with its elementwise
bound, written from the operation's definition (include/tutel_amd.h: D = act(A op(W) + bias) * G, rounded once) and not from the
kernels.  Nothing here needs a GPU or the library."""
import math
import random

import torch

from _packed_fuzz import ACTS64, DTYPES, check_promised   # noqa: F401  (check_promised: re-exported for the two test modules)

SENTINEL = 3.0      # what an output buffer holds before the call (tests/test_fuzz_gpu.py::run_gemm_fuzz)
GLU_E = [1, 2, 3, 5]
GLU_R = [1, 31, 64, 127, 128, 129, 255, 256, 257, 300, 513]
GLU_N = [8, 24, 120, 128, 136, 248, 256, 264, 520]
GLU_K = [64, 128, 192, 320, 512]
GLU_ACT = ["none", "relu", "gelu", "silu"]
GLU_IMPL = [-1, 0, 1, 4]            # TUTEL_OPT_GEMM_IMPL
GLU_TILE = [-1, 0, 1, 2, 3, 4]      # TUTEL_OPT_GEMM_TILE
GLU_STORE = [-1, 0, 1, 2]           # TUTEL_OPT_GEMM_STORE
FORMS = ["plain", "mul_random", "mul_mask", "mul_pow2", "gate_up"]
GATED = ("mul_random", "mul_mask", "mul_pow2")     # the forms with a gating operand G (gate_up computes its own)
MAX_WORK = 1 << 28                  # E * R * N * K of a case
POW2_MIN = 2.0 ** -13               # fp16: the pow2 identity is asserted where the pre-gating magnitude is at least this
POW2_LEFT_OUT_CAP = 2e-3            # ... and at most this share of a case's elements may lie below it

GLU_PROMISED = ({"form=" + f for f in FORMS} | {"kmajor+mul", "nmajor+mul", "bias+mul", "ragged_N+mul", "N=8+mul", "R=1+mul", "R>256+mul",
                                                "R%128!=0+mul", "K=64+mul", "ep+mul", "ep+plain", "row_counts+mul", "inplace", "f16", "bf16"}
                | {"impl=%d+mul" % v for v in GLU_IMPL} | {"tile=%d+mul" % v for v in GLU_TILE} | {"store=%d+mul" % v for v in GLU_STORE})

# The fixed head of every case list: the smallest shapes that reach, WITH a gating operand, the kernel templates a random draw of
# the forced options seldom or never reaches (csrc/gemm_plan.hip):
#   the 128 x 256 ring      k-major, impl = 4, tile <= 0, R <= 128, N >= 256
#   the 256 x 128 rings     k-major, tile = 2 (two slots), tile = 3 (three slots, buffer path), tile = 3 with impl = 2 (three slots
#                           without the buffer path -- the only drawn-or-fixed case with an impl outside GLU_IMPL)
#   the plain 256 x 256     tile = 1, here with n-major weights (which never take the ping-pong kernel)
#   the 256 x 256 ping-pong k-major, tile = 4
_HEAD = [
    dict(E=2, R=127, N=264, K=128, kmajor=True, act="silu", dtype="bf16", bias=True, impl=4, tile=-1, store=-1, form="mul_random", W=0, rc=False, inplace=False),
    dict(E=2, R=129, N=136, K=64, kmajor=True, act="none", dtype="f16", bias=False, impl=-1, tile=2, store=0, form="mul_pow2", W=0, rc=False, inplace=False),
    dict(E=1, R=300, N=264, K=128, kmajor=True, act="relu", dtype="bf16", bias=True, impl=-1, tile=3, store=1, form="mul_mask", W=4, rc=False, inplace=False),
    dict(E=2, R=257, N=128, K=192, kmajor=True, act="gelu", dtype="f16", bias=False, impl=2, tile=3, store=-1, form="mul_random", W=0, rc=True, inplace=False),
    dict(E=2, R=256, N=248, K=64, kmajor=False, act="none", dtype="bf16", bias=True, impl=0, tile=1, store=2, form="mul_pow2", W=2, rc=False, inplace=True),
    dict(E=3, R=513, N=520, K=64, kmajor=True, act="none", dtype="bf16", bias=False, impl=1, tile=4, store=-1, form="mul_random", W=0, rc=True, inplace=True),
]


def _counts(rnd, E, R, case):
    """dropless row counts: random, one expert forced to 0 and (from two experts) another to R"""
    counts = [rnd.randint(0, R) for _ in range(E)]
    i0 = rnd.randrange(E)
    if E == 1:
        counts[0] = (0, R)[case % 2]
    else:
        counts[i0] = 0
        counts[(i0 + 1 + rnd.randrange(E - 1)) % E] = R
    return counts


def gen_glu_cases(n_cases, seed):
    """A deterministic list of cases (dicts).  One random.Random stream consumed case by case, so the first n cases do not depend on how
    many follow; cases [0, len(_HEAD)) are the fixed head."""
    rnd = random.Random(seed)
    out = []
    for case in range(n_cases):
        if case < len(_HEAD):
            d = dict(_HEAD[case])
            rc = d.pop("rc")
            d.update(case=case, layout="ep" if d["W"] else "contig", row_counts=_counts(rnd, d["E"], d["R"], case) if rc else None,
                     row_align=(1, 4, 32)[case % 3], seed=seed * 7919 + case)
            out.append(d)
            continue
        E, R, N, K = rnd.choice(GLU_E), rnd.choice(GLU_R), rnd.choice(GLU_N), rnd.choice(GLU_K)
        while E * R * N * K > MAX_WORK:
            if E > 1:
                E = GLU_E[GLU_E.index(E) - 1]
            else:
                K = GLU_K[GLU_K.index(K) - 1]
        kmajor = rnd.random() < 0.6
        act, dtype, bias = rnd.choice(GLU_ACT), rnd.choice(["bf16", "f16"]), rnd.random() < 0.5
        impl, tile, store = rnd.choice(GLU_IMPL), rnd.choice(GLU_TILE), rnd.choice(GLU_STORE)
        form = rnd.choice(FORMS)
        if form == "gate_up" and not (kmajor and not bias and act != "none"):
            form = rnd.choice(FORMS[:4])
        if form == "mul_pow2" and dtype == "f16" and act == "relu":
            # half of ReLU's outputs are zeros or next to it: they would all fall under POW2_MIN, beyond the cap on what the fp16 identity
            # may leave out.  bf16 (nothing left out) keeps relu x pow2, and mul_mask is the exact check of relu in fp16
            act = "none"
        W = rnd.choice([0, 0, 2, 4])
        # the strided addressing of ops.expert_gemm; ops.expert_gemm_gate_up takes the contiguous layout only
        if W and (R % W != 0 or form == "gate_up"):
            W = 0
        rc = rnd.randrange(3) == 0
        counts = _counts(rnd, E, R, case) if rc else None
        row_align = rnd.choice([1, 4, 32])
        inplace = form in GATED and rnd.random() < 0.3
        out.append(dict(case=case, E=E, R=R, N=N, K=K, kmajor=kmajor, act=act, dtype=dtype, bias=bias, impl=impl, tile=tile, store=store, form=form,
                        layout="ep" if W else "contig", W=W, row_counts=counts, row_align=row_align, inplace=inplace, seed=seed * 7919 + case))
    return out


def glu_tag(d):
    rc = "none" if d["row_counts"] is None else "%s/align%d" % (d["row_counts"], d["row_align"])
    return ("glu case {case}: E={E} R={R} N={N} K={K} kmajor={kmajor} act={act} {dtype} bias={bias} form={form} layout={layout} W={W} row_counts={rc} "
            "inplace={inplace} impl={impl} tile={tile} store={store} seed={seed}").format(rc=rc, **d)


def glu_classes(d):
    c = {"form=" + d["form"], d["dtype"]}
    gated = d["form"] in GATED
    for name, on in (("kmajor+mul" if d["kmajor"] else "nmajor+mul", gated), ("bias+mul", gated and d["bias"]),
                     ("ragged_N+mul", gated and d["N"] % 128 != 0), ("N=8+mul", gated and d["N"] == 8), ("R=1+mul", gated and d["R"] == 1),
                     ("R>256+mul", gated and d["R"] > 256), ("R%128!=0+mul", gated and d["R"] % 128 != 0), ("K=64+mul", gated and d["K"] == 64),
                     ("ep+mul", gated and d["layout"] == "ep"), ("ep+plain", d["form"] == "plain" and d["layout"] == "ep"),
                     ("row_counts+mul", gated and d["row_counts"] is not None), ("inplace", d["inplace"]),
                     ("impl=%d+mul" % d["impl"], gated), ("tile=%d+mul" % d["tile"], gated), ("store=%d+mul" % d["store"], gated)):
        if on:
            c.add(name)
    return c


def row_limits(d):
    """per expert: the rows the launch computes and writes -- min(R, ceil(count / row_align) * row_align), R without row counts"""
    if d["row_counts"] is None:
        return [d["R"]] * d["E"]
    return [min(d["R"], -(-c // d["row_align"]) * d["row_align"]) for c in d["row_counts"]]


# =================================================================================================================================
# inputs
# =================================================================================================================================
def pow2_gate(E, R, N):
    """G[e, r, n] = s * 2^p, p = (e + 3 r + 5 n) mod 3, s = -1 where r + n is odd: no two neighbouring rows or columns share a value
    (the row above has the other sign, the column to the left the other sign and another magnitude, the next expert another magnitude).
    Rows an even distance apart share their values: a G read from another rank's block of the `ep` layout is the random and the mask
    forms' to catch when C is even."""
    e = torch.arange(E).view(E, 1, 1)
    r = torch.arange(R).view(1, R, 1)
    n = torch.arange(N).view(1, 1, N)
    return torch.pow(2.0, ((e + 3 * r + 5 * n) % 3).double()) * (1 - 2 * ((r + n) % 2)).double()


def make_glu_inputs(d):
    """the case's CPU tensors in the logical form: a [E, R, K] ~ N(0, 1), w [E, N, K] | [E, K, N] ~ U(-1, 1) / sqrt(K) (asymmetric; the
    product's standard deviation is 0.58), bias [E, N] | None, G [E, R, N] | None, w_up (gate_up: w is the gate's weight) | None"""
    dtype = DTYPES[d["dtype"]]
    E, R, N, K = d["E"], d["R"], d["N"], d["K"]
    g = torch.Generator().manual_seed(d["seed"])
    shape = [E, N, K] if d["kmajor"] else [E, K, N]
    for _ in range(16):
        a = torch.randn([E, R, K], generator=g).to(dtype)
        w = ((torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(K)).to(dtype)
        bias = torch.randn([E, N], generator=g).to(dtype) if d["bias"] else None
        if not (d["form"] == "mul_pow2" and d["dtype"] == "f16"):
            break
        # the condition of the exact fp16 check (POW2_LEFT_OUT_CAP) is the generator's to meet: about 0.03 % of the elements lie below
        # POW2_MIN, but in a case of a few hundred elements ONE of them is more than the cap -- such a draw is repeated from the same stream
        _, v = ref_glu(a, w, bias, d["kmajor"], d["act"], None, dtype)
        if float(pow2_left_out(v, dtype).double().mean()) <= POW2_LEFT_OUT_CAP:
            break
    else:
        raise AssertionError("no draw of this case meets the cap on what the fp16 pow2 check leaves out")
    G = w_up = None
    if d["form"] == "mul_random":
        G = torch.randn([E, R, N], generator=g)
        G[torch.rand([E, R, N], generator=g) < 0.1] = 0
        G = G.to(dtype)
    elif d["form"] == "mul_mask":
        G = (torch.rand([E, R, N], generator=g) < 0.5).to(dtype)
    elif d["form"] == "mul_pow2":
        G = pow2_gate(E, R, N).to(dtype)
    elif d["form"] == "gate_up":
        w_up = ((torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(K)).to(dtype)
    return a, w, bias, G, w_up


def to_ep(t, W, gap=0, fill=0.0):
    """logical [E, R, X] -> the all-to-all addressing [W, E, C + gap, X], R = W * C: row r of expert e is row r % C of rank r // C;
    `gap` extra rows behind every rank's rows of an expert hold `fill`"""
    E, R, X = t.shape
    C = R // W
    out = torch.full([W, E, C + gap, X], fill, dtype=t.dtype)
    out[:, :, :C] = t.view(E, W, C, X).permute(1, 0, 2, 3)
    return out


def from_ep(p, W, gap=0):
    """the inverse: [W, E, C + gap, X] -> logical [E, R, X], and the gap rows [W, E, gap, X]"""
    _, E, Cg, X = p.shape
    C = Cg - gap
    return p[:, :, :C].permute(1, 0, 2, 3).reshape(E, W * C, X), p[:, :, C:]


def ep_layouts(d):
    """(a_layout, d_layout) of ops.expert_gemm for the case's `ep` form: (stride_e, stride_w, rows_per_w, ld); one gap row in D"""
    W, E, N, K = d["W"], d["E"], d["N"], d["K"]
    C = d["R"] // W
    return (C * K, E * C * K, C, K), ((C + 1) * N, E * (C + 1) * N, C, N)


# =================================================================================================================================
# reference and bound
# =================================================================================================================================
def ref_glu(a, w, bias, kmajor, act, G, dtype):
    """a [E, R, K], w [E, N, K] (kmajor) | [E, K, N], bias [E, N] | None, G [E, R, N] | None -> (ref, v): v = act(a op(w) + bias) in
    float64 on the rounded inputs, ref = v * G rounded ONCE to dtype (as float64)"""
    wd = w.double()
    v = torch.matmul(a.double(), wd.transpose(1, 2) if kmajor else wd)
    if bias is not None:
        v = v + bias.double().unsqueeze(1)
    v = ACTS64[act](v)
    y = v if G is None else v * G.double()
    return y.to(dtype).double(), v


def ref_gate(a, w_gate, act, dtype):
    """the gate of the fused gate/up form: act(a Wg^T) in float64, rounded to dtype"""
    return ACTS64[act](torch.matmul(a.double(), w_gate.double().transpose(1, 2))).to(dtype)


def glu_bound(ref, G, dtype):
    """The bar the project holds these kernels to (tests/test_ops_gpu.py::_gemm_tol, run_gemm_fuzz): eps = 2^-7, floor = 2e-3 in bf16;
    2^-10, 3e-4 in fp16.  The pre-gating value is within `floor` of exact before its rounding and gating scales that by |G|, so
    element by element the bound is eps * |ref| + floor * max(1, |G|)."""
    eps, floor = (2 ** -7, 2e-3) if dtype == torch.bfloat16 else (2 ** -10, 3e-4)
    scale = torch.ones_like(ref) if G is None else G.double().abs().clamp(min=1.0)
    return eps * ref.abs() + floor * scale


def pow2_left_out(v, dtype):
    """mask of the elements the exact pow2 identity leaves out: fp16 results that may round in the subnormal range; none in bf16"""
    if dtype == torch.bfloat16:
        return torch.zeros_like(v, dtype=torch.bool)
    return v.abs() < POW2_MIN
