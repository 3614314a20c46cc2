"""TEST-ONLY pieces shared by the fuzzers of the packed dropless kernels (tests/test_packed_fuzz_gpu.py) and their GPU-free checks
(tests/test_packed_fuzz_cpu.py): the seeded case generators, the edge classes each fuzzer promises to draw, and the references --
plain integer arithmetic for the layout, float64 for the GEMM / weight gradient / bias gradient, written from the layout's
definition (csrc/dropless.hip header comment) and not from the kernels; the guard bands (moated / moat_intact) that surround every
operand of the GEMM and gradient fuzzers.  Nothing here needs a GPU or the library."""
import math
import random

import numpy as np
import torch

TILE = 256          # rows per M-tile of the packed GEMM (tutel_amd_packed_plan_t.tile_rows)
SENTINEL = -777     # what the layout's output tensors hold before the call

E_CHOICES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 100, 127, 128, 129, 130, 192, 255, 256, 257, 300, 500, 512, 513, 1000,
             1024, 1025, 1500, 2048, 3000, 4095, 4096]      # tests/test_fuzz_gpu.py::E_CHOICES
ROW_CHOICES = [0, 1, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 700]
ACTS64 = {"none": lambda t: t, "relu": torch.relu, "gelu": torch.nn.functional.gelu, "silu": torch.nn.functional.silu}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def round_up(v, a):
    return -(-v // a) * a


# =================================================================================================================================
# references
# =================================================================================================================================
def ref_locations(idx, E):
    """idx [k, T] (numpy) -> loc [k, T], counts [E]: the stable rank of every valid entry inside its expert, entries ordered by
    (choice, token); a masked entry (id outside [0, E)) gets 0 and counts nowhere"""
    flat = np.asarray(idx, dtype=np.int64).reshape(-1)
    valid = (flat >= 0) & (flat < E)
    q = np.nonzero(valid)[0]
    e = flat[q]
    order = np.argsort(e, kind="stable")
    se = e[order]
    cnt = np.bincount(se, minlength=E).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    loc = np.zeros_like(flat)
    loc[q[order]] = np.arange(se.size) - start[se]
    return loc.reshape(np.shape(idx)).astype(np.int32), cnt.astype(np.int32)


def ref_layout(cnt, idx, loc, E, limit, align, rows_bound):
    """The packed layout of one routing: kept_e = min(count_e, L), L = round_up(limit, align) (none when limit == 0); rows_e =
    round_up(kept_e, align); offsets = exclusive prefix sum; capacity = max rows_e; one tile per started 256 rows of an expert,
    expert-major; slot[offsets[e] + loc] = j * T + t for every kept entry, -1 in every other row below rows_bound."""
    cnt = np.asarray(cnt, dtype=np.int64)
    L = round_up(limit, align) if limit > 0 else None
    kept = cnt if L is None else np.minimum(cnt, L)
    rows = (kept + align - 1) // align * align
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    tiles = [(e, int(off[e]) + r) for e in range(E) for r in range(0, int(rows[e]), TILE)]
    fi, fl = np.asarray(idx, dtype=np.int64).reshape(-1), np.asarray(loc, dtype=np.int64).reshape(-1)
    keep = (fi >= 0) & (fi < E) & (fl >= 0)
    if L is not None:
        keep &= fl < L
    slot = np.full([rows_bound], -1, dtype=np.int64)
    q = np.nonzero(keep)[0]
    slot[off[fi[q]] + fl[q]] = q
    return dict(offsets=off, capacity=int(rows.max()) if E else 0, ntiles=len(tiles), tiles=np.array(tiles, dtype=np.int64).reshape(-1, 2),
                slot=slot, keep=keep.reshape(np.shape(idx)), rows=rows, kept=kept, row_limit=L)


def ref_gemm(a_rows, w, bias, kmajor, act, mul, offsets, dtype):
    """fp64 product of the packed rows [0, offsets[E]) on the rounded inputs, rounded once to dtype: a_rows [>= offsets[E], K] (pad rows
    as the kernel sees them), w [E, N, K] or [E, K, N], bias [E, N] | None, mul [rows, N] | None"""
    E = w.shape[0]
    N = w.shape[1] if kmajor else w.shape[2]
    used = int(offsets[E])
    out = torch.zeros([used, N], dtype=torch.float64)
    for e in range(E):
        r0, r1 = int(offsets[e]), int(offsets[e + 1])
        if r1 == r0:
            continue
        we = w[e].double()
        y = a_rows[r0:r1].double() @ (we.t() if kmajor else we)
        if bias is not None:
            y = y + bias[e].double()
        y = ACTS64[act](y)
        if mul is not None:
            y = y * mul[r0:r1].double()
        out[r0:r1] = y
    return out.to(dtype).double()


def ref_wgrad(a_rows, b_rows, offsets):
    """per expert A^T B in fp64 and the bound operand |A|^T |B| -> [E, Na, Nb] each"""
    E = len(offsets) - 1
    out = torch.zeros([E, a_rows.shape[1], b_rows.shape[1]], dtype=torch.float64)
    bnd = torch.zeros_like(out)
    for e in range(E):
        r0, r1 = int(offsets[e]), int(offsets[e + 1])
        if r1 > r0:
            A, B = a_rows[r0:r1].double(), b_rows[r0:r1].double()
            out[e], bnd[e] = A.t() @ B, A.abs().t() @ B.abs()
    return out, bnd


def ref_bgrad(b_rows, offsets):
    """per expert column sums in fp64, the sums of magnitudes, and the row counts n_e -> [E, N], [E, N], [E]"""
    E = len(offsets) - 1
    out = torch.zeros([E, b_rows.shape[1]], dtype=torch.float64)
    mag = torch.zeros_like(out)
    n = torch.zeros([E], dtype=torch.float64)
    for e in range(E):
        r0, r1 = int(offsets[e]), int(offsets[e + 1])
        if r1 > r0:
            B = b_rows[r0:r1].double()
            out[e], mag[e], n[e] = B.sum(0), B.abs().sum(0), r1 - r0
    return out, mag, n


def wgrad_bound(ref, bnd, dtype):
    """the bar of tests/test_packed_train_gpu.py::test_wgrad_kernel_against_float64"""
    return 2 ** -8 * ref.abs() + 2 ** -12 * bnd + (2 ** -24 if dtype == torch.float16 else 0)


def bgrad_bound(ref, mag, n, dtype):
    """n_e rows summed in fp32 in order (each add within 2^-24 of a partial sum that is at most sum |B|), rounded once to the dtype
    (u = 2^-8 bf16, 2^-11 fp16; + 2^-24: one rounding in fp16's subnormal range)"""
    u = 2 ** -8 if dtype == torch.bfloat16 else 2 ** -11
    return u * ref.abs() + n.unsqueeze(1) * 2 ** -24 * mag + (2 ** -24 if dtype == torch.float16 else 0)


def gathered(x, slot):
    """rows read through a slot map: x[slot % T], the zero row where slot < 0"""
    T = x.shape[0]
    slot = torch.as_tensor(slot, dtype=torch.int64)
    rows = x[(slot.clamp(min=0) % T)]
    rows[slot < 0] = 0
    return rows


def padded_rows(buf, offsets, kept, C):
    """the kept rows of a packed buffer laid out [E, C, M] on the host (rows an expert does not keep: zeros)"""
    E = len(offsets) - 1
    out = torch.zeros([E, C, buf.shape[1]], dtype=buf.dtype)
    for e in range(E):
        n = int(kept[e])
        if n:
            out[e, :n] = buf[int(offsets[e]):int(offsets[e]) + n]
    return out


def ref_encode(x, slot, gates):
    """fast_encode through a slot map: out[r] = gates[q] * x[q % T] (one fp32 product, rounded once), zeros where slot < 0"""
    T = x.shape[0]
    slot = torch.as_tensor(slot, dtype=torch.int64)
    q = slot.clamp(min=0)
    rows = x.float()[q % T]
    if gates is not None:
        rows = rows * gates.reshape(-1).float()[q].unsqueeze(1)
    rows[slot < 0] = 0
    return rows.to(x.dtype)


# =================================================================================================================================
# layouts synthesised from per-expert row counts
# =================================================================================================================================
def rows_routing(rows, T=None, k=1):
    """idx, loc [k, T] int32 (CPU) of a routing whose expert e keeps rows[e] entries: entry q = (choice q // T, token q % T), the experts
    in order; the remaining entries are masked (-1)"""
    n = int(sum(rows))
    T = T or max(n, 1)
    assert k * T >= n
    idx = torch.full([k * T], -1, dtype=torch.int32)
    loc = torch.zeros([k * T], dtype=torch.int32)
    r = torch.tensor(rows, dtype=torch.int64)
    idx[:n] = torch.repeat_interleave(torch.arange(len(rows)), r).int()
    start = torch.cumsum(r, 0) - r
    loc[:n] = (torch.arange(n) - torch.repeat_interleave(start, r)).int()
    return idx.view(k, T), loc.view(k, T)


def layout_from_rows(rows, align=1, T=None, k=1):
    """a PackedLayout (built by the library on the GPU) whose expert e owns rows[e] kept rows -> (layout, idx, loc on the device)"""
    from tutel_amd import ops
    from tutel_amd.impls import ep_native
    idx, loc = rows_routing(rows, T, k)
    E, T = len(rows), idx.shape[1]
    idx, loc = idx.cuda(), loc.cuda()
    cnt = torch.tensor(rows, dtype=torch.int32, device="cuda")
    plan, why = ep_native.packed_plan(T, E, k, 128, 128, 128, torch.bfloat16, 0, align)
    assert plan is not None, why
    return ops.packed_layout(cnt, idx, loc, 0, align, plan["rows_bound"], plan["tiles_bound"], plan["row_limit"]), idx, loc


def offsets_from_rows(rows, align):
    r = [round_up(int(v), align) for v in rows]
    return [0] + list(np.cumsum(r))


# =================================================================================================================================
# generators: one random.Random stream, consumed case by case, so that the first n cases do not depend on how many follow
# =================================================================================================================================
# ---- a. layout -------------------------------------------------------------------------------------------------------------------
LAYOUT_T = [1, 2, 5, 63, 64, 65, 255, 256, 257, 300, 1000, 4097, 8192, 20000]
LAYOUT_ALIGN = [1, 2, 4, 8, 32, 128, 256]
LAYOUT_PROMISED = {"E=4096", "E>1024", "E=1", "k=16", "k=1", "T=1", "T=20000", "align>=128", "align=1", "limit=0", "limit=1", "limit_drops", "masked",
                   "all_on_k", "skewed", "empty_expert", "multi_tile_expert", "pad_rows", "rows_past_used"}


def gen_layout_cases(n_cases, seed):
    rnd = random.Random(seed)
    out = []
    for case in range(n_cases):
        E = rnd.choice(E_CHOICES + [4096, 4096, 2048, 1025, 1, 8, 64])
        k = min(E, rnd.choice([1, 2, 2, 3, 4, 8, 16, 16]))
        while k * E > 8192:
            k -= 1
        T = rnd.choice(LAYOUT_T)
        if k * T > 160000:
            T = 160000 // k
        align = rnd.choice(LAYOUT_ALIGN)
        base = k * (-(-T // E))
        limit = max(0, rnd.choice([0, 0, 0, 1, base, base - 1, base + 1, base // 2, base // 3 + 1, 2 * base, base // 4]))
        mode = rnd.choice(["random", "random", "skewed", "all_on_k"])
        mask_p = rnd.choice([0.0, 0.0, 0.1, 0.5, 0.95])
        out.append(dict(case=case, T=T, E=E, k=k, align=align, limit=limit, mode=mode, mask_p=mask_p, seed=seed * 100003 + case))
    return out


def make_routing(d):
    """the case's expert ids [k, T] int32 (numpy): k distinct experts per token, a share of the entries masked with -1"""
    g = np.random.default_rng(d["seed"])
    T, E, k = d["T"], d["E"], d["k"]
    offs = g.choice(E, size=k, replace=False).astype(np.int64)
    if d["mode"] == "all_on_k":
        base = np.zeros([T], dtype=np.int64)
    elif d["mode"] == "skewed":
        base = np.minimum((E * g.random(T) ** 3).astype(np.int64), E - 1)
    else:
        base = g.integers(0, E, size=T)
    idx = (base[None, :] + offs[:, None]) % E
    if d["mask_p"] > 0:
        idx[g.random([k, T]) < d["mask_p"]] = -1
    return idx.astype(np.int32)


def layout_tag(d):
    return "layout case {case}: T={T} E={E} k={k} align={align} limit={limit} {mode} mask={mask_p}".format(**d)


def layout_classes(d, ref, rows_bound, idx):
    c = set()
    E, k, T = d["E"], d["k"], d["T"]
    for name, on in (("E=4096", E == 4096), ("E>1024", E > 1024), ("E=1", E == 1), ("k=16", k == 16), ("k=1", k == 1), ("T=1", T == 1),
                     ("T=20000", T == 20000), ("align>=128", d["align"] >= 128), ("align=1", d["align"] == 1), ("limit=0", d["limit"] == 0),
                     ("limit=1", d["limit"] == 1), ("masked", d["mask_p"] > 0), ("all_on_k", d["mode"] == "all_on_k"),
                     ("skewed", d["mode"] == "skewed"), ("empty_expert", bool((ref["rows"] == 0).any())),
                     ("multi_tile_expert", bool((ref["rows"] > TILE).any())), ("pad_rows", bool((ref["rows"] > ref["kept"]).any())),
                     ("rows_past_used", int(ref["offsets"][-1]) < rows_bound)):
        if on:
            c.add(name)
    if ref["row_limit"] is not None and bool(((np.asarray(idx) >= 0) & ~ref["keep"]).any()):
        c.add("limit_drops")
    return c


# ---- b. grouped GEMM ---------------------------------------------------------------------------------------------------------------
GEMM_E = [1, 2, 3, 8, 17, 64, 128, 300]
GEMM_N = [8, 16, 24, 64, 72, 120, 128, 136, 192, 248, 256, 264, 328, 512, 520, 1024, 2048]
GEMM_K = [64, 128, 192, 256, 512, 1024, 2048]
GEMM_PROMISED = {"w_once_on", "w_once_off", "cap<256", "cap>=256", "act=none", "act=relu", "act=gelu", "act=silu", "nmajor", "kmajor", "gather", "mul",
                 "bias", "no_bias", "N<128_kmajor", "N<128_nmajor", "gather_pad_rows", "K=64", "ragged_N", "one_hot", "first_empty", "last_empty", "new_tile", "bf16", "f16", "E=300", "E=1",
                 "align>1", "pad_rows", "multi_tile_expert"}


def draw_rows(rnd, E, budget_rows):
    """per-expert kept rows and the name of the draw; the total is cut to budget_rows by replacing the largest draws with small ones"""
    mode = rnd.choice(["random", "random", "random", "one_hot", "first_empty", "last_empty", "new_tile"])
    if mode == "new_tile" and (E > 17 or 257 * E > budget_rows):
        mode = "random"
    if mode in ("first_empty", "last_empty") and E < 2:
        mode = "random"
    if mode == "one_hot":
        rows = [0] * E
        rows[rnd.randrange(E)] = rnd.choice(ROW_CHOICES[1:])
    elif mode == "new_tile":
        rows = [rnd.choice([257, 257, 513])] * E     # every expert one row into a new tile
    else:
        rows = [rnd.choice(ROW_CHOICES) for _ in range(E)]
        if mode == "first_empty":
            rows[0] = 0
        if mode == "last_empty":
            rows[-1] = 0
    while sum(rows) > budget_rows:
        rows[rows.index(max(rows))] = rnd.choice([0, 1, 7, 31, 33])
        if mode == "new_tile":
            mode = "random"
    return rows, mode


def gen_gemm_cases(n_cases, seed):
    rnd = random.Random(seed)
    out = []
    for case in range(n_cases):
        E = rnd.choice(GEMM_E)
        N, K = rnd.choice(GEMM_N), rnd.choice(GEMM_K)
        while E * N * K > (1 << 25):          # the weights stay below 64 MiB
            if K > 64:
                K = GEMM_K[GEMM_K.index(K) - 1]
            else:
                N = GEMM_N[GEMM_N.index(N) - 1]
        align = rnd.choice([1, 1, 4, 8, 128])
        rows, mode = draw_rows(rnd, E, max(1, (1 << 30) // (N * K * (2 if align == 128 else 1))))
        if align == 128:                       # pad rows are computed too: keep the padded total within the budget
            while sum(round_up(r, 128) for r in rows) * N * K > (1 << 31):
                rows[rows.index(max(rows))] = 0
        kmajor = rnd.random() < 0.7
        act = rnd.choice(["none", "relu", "gelu", "silu"]) if kmajor else rnd.choice(["none", "relu"])
        gather = kmajor and rnd.random() < 0.35
        out.append(dict(case=case, E=E, rows=rows, mode=mode, align=align, N=N, K=K, kmajor=kmajor, act=act, dtype=rnd.choice(["bf16", "f16"]),
                        bias=rnd.random() < 0.6, mul=kmajor and rnd.random() < 0.35, gather=gather, T=rnd.choice([1, 50, 1000]) if gather else 0,
                        seed=seed * 7919 + case))
    return out


def rows_brief(rows):
    return "[" + ",".join(str(r) for r in rows[:12]) + (",...x%d" % len(rows) if len(rows) > 12 else "") + "]"


def gemm_tag(d):
    return ("packed gemm case {case}: E={E} rows={r} ({mode}) align={align} N={N} K={K} kmajor={kmajor} act={act} {dtype} bias={bias} mul={mul} "
            "gather={gather} T={T}").format(r=rows_brief(d["rows"]), **d)


def rows_classes(d):
    c = {d["mode"]} & {"one_hot", "first_empty", "last_empty", "new_tile"}
    cap = max(round_up(r, d["align"]) for r in d["rows"])
    c.add("cap<256" if cap < 256 else "cap>=256")
    for name, on in (("align>1", d["align"] > 1), ("pad_rows", any(r % d["align"] for r in d["rows"])), ("multi_tile_expert", cap > TILE),
                     ("E=300", d["E"] == 300), ("E=1", d["E"] == 1), (d["dtype"], True)):
        if on:
            c.add(name)
    return c


def gemm_classes(d):
    c = rows_classes(d)
    if d["kmajor"]:
        c.add("w_once_on" if d["E"] * (-(-d["N"] // 256)) >= 256 else "w_once_off")
    for name, on in (("act=" + d["act"], True), ("kmajor" if d["kmajor"] else "nmajor", True), ("gather", d["gather"]), ("mul", d["mul"]),
                     ("bias" if d["bias"] else "no_bias", True), ("N<128_kmajor" if d["kmajor"] else "N<128_nmajor", d["N"] < 128),
                     ("gather_pad_rows", d["gather"] and d["align"] > 1 and any(r % d["align"] for r in d["rows"])), ("K=64", d["K"] == 64), ("ragged_N", d["N"] % 128 != 0)):
        if on:
            c.add(name)
    return c


# ---- c. weight / bias gradient -----------------------------------------------------------------------------------------------------
GRAD_N = [8, 16, 64, 120, 128, 136, 192, 256, 264, 512]
GRAD_PROMISED = {"gather=a", "gather=b", "gather=none", "N=8", "N>128", "ragged_N", "one_hot", "first_empty", "last_empty", "new_tile", "bf16", "f16",
                 "E=300", "E=1", "E=4096", "align>1", "pad_rows", "cap<256", "cap>=256", "rows%64!=0", "multi_tile_expert"}


def gen_grad_cases(n_cases, seed):
    rnd = random.Random(seed)
    out = []
    for case in range(n_cases):
        if case == 7:
            # the grid arithmetic at the layout's largest expert count: 4096 experts x one 128 x 128 tile each
            out.append(dict(case=case, E=4096, rows=[(e * 7) % 5 for e in range(4096)], mode="random", align=1, Na=128, Nb=128, gather="none", T=0,
                            dtype="bf16", seed=seed * 104729 + case))
            continue
        E = rnd.choice(GEMM_E)
        Na, Nb = rnd.choice(GRAD_N), rnd.choice(GRAD_N)
        while E * Na * Nb > (1 << 23):
            if Na >= Nb:
                Na = GRAD_N[GRAD_N.index(Na) - 1]
            else:
                Nb = GRAD_N[GRAD_N.index(Nb) - 1]
        align = rnd.choice([1, 1, 4, 8, 128])
        rows, mode = draw_rows(rnd, E, max(1, (1 << 29) // (Na * Nb)))
        if align == 128:
            while sum(round_up(r, 128) for r in rows) * max(Na, Nb) > (1 << 25):
                rows[rows.index(max(rows))] = 0
        gather = rnd.choice(["none", "none", "a", "b"])
        out.append(dict(case=case, E=E, rows=rows, mode=mode, align=align, Na=Na, Nb=Nb, gather=gather, T=rnd.choice([1, 50, 1000]) if gather != "none" else 0,
                        dtype=rnd.choice(["bf16", "f16"]), seed=seed * 104729 + case))
    return out


def grad_tag(d):
    return "packed grad case {case}: E={E} rows={r} ({mode}) align={align} Na={Na} Nb={Nb} gather={gather} T={T} {dtype}".format(r=rows_brief(d["rows"]), **d)


def grad_classes(d):
    c = rows_classes(d)
    for name, on in (("gather=" + d["gather"], True), ("N=8", 8 in (d["Na"], d["Nb"])), ("N>128", max(d["Na"], d["Nb"]) > 128),
                     ("ragged_N", d["Na"] % 128 != 0 or d["Nb"] % 128 != 0), ("E=4096", d["E"] == 4096),
                     ("rows%64!=0", any(round_up(r, d["align"]) % 64 for r in d["rows"]))):
        if on:
            c.add(name)
    return c


# ---- d. decode / gate gradient -------------------------------------------------------------------------------------------------------
DEC_M = [8, 40, 64, 100, 136, 256, 1024, 2048]
DEC_PROMISED = {"k=1", "k=2", "k=3", "k=4", "k=8", "k=16", "M%8!=0", "M>=1024", "M=8", "bf16", "f16", "gates=f32", "gates=row", "gates=none", "limit_drops",
                "masked", "align>1", "all_on_k", "T=1", "rows_past_used"}


def gen_decode_cases(n_cases, seed):
    rnd = random.Random(seed)
    out = []
    for case in range(n_cases):
        E = rnd.choice([2, 3, 8, 17, 64, 128, 300, 16, 32, 1])
        k = min(E, rnd.choice([1, 2, 2, 3, 4, 8, 16]))
        T = rnd.choice([1, 2, 63, 64, 65, 300, 1000, 2048])
        align = rnd.choice([1, 1, 4, 8])
        base = k * (-(-T // E))
        limit = max(0, rnd.choice([0, 0, base, base // 2, base // 3 + 1, 1, base + 1]))
        mode = rnd.choice(["random", "random", "skewed", "all_on_k"])
        out.append(dict(case=case, T=T, E=E, k=k, align=align, limit=limit, mode=mode, mask_p=rnd.choice([0.0, 0.0, 0.1, 0.5]), M=rnd.choice(DEC_M),
                        dtype=rnd.choice(["bf16", "f16"]), gates=rnd.choice(["f32", "row", "none"]), seed=seed * 15485863 + case))
    return out


def decode_M(d, E, C):
    """the case's M, lowered until the host's padded copy [E, C, M] stays below 2^25 elements"""
    M = d["M"]
    while E * C * M > (1 << 25) and M > DEC_M[0]:
        M = DEC_M[DEC_M.index(M) - 1]
    return M


def decode_tag(d):
    return "packed decode case {case}: T={T} E={E} k={k} M={M} align={align} limit={limit} {mode} mask={mask_p} {dtype} gates={gates}".format(**d)


def decode_classes(d, ref, rows_bound, M, idx):
    c = layout_classes(d, ref, rows_bound, idx) &{"limit_drops", "masked", "all_on_k", "T=1", "rows_past_used"}
    for name, on in (("k=%d" % d["k"], d["k"] in (1, 2, 3, 4, 8, 16)), ("M%8!=0", M % 8 != 0), ("M>=1024", M >= 1024), ("M=8", M == 8), (d["dtype"], True),
                     ("gates=" + d["gates"], True), ("align>1", d["align"] > 1)):
        if on:
            c.add(name)
    return c


# ---- e. whole packed layers ------------------------------------------------------------------------------------------------------
LAYER_T = [1, 3, 64, 100, 127, 128, 129, 500, 1000, 1024, 2000, 4096, 5000, 7680, 7681, 8192]      # tests/test_fuzz_gpu.py::run_layer_fuzz
LAYER_PROMISED = {"cf=0", "cf<0", "megablocks=0", "megablocks=1", "megablocks=2", "megablocks=4", "act=relu", "act=gelu", "act=silu", "graph", "eager",
                  "fp32_gate", "gate_in_dtype", "experts=ffn", "experts=swiglu", "swiglu_w_once_on", "swiglu_w_once_off", "bf16", "f16", "E=256", "E=1"}


def gen_layer_cases(n_cases, seed):
    """dropless layers the packed forward covers (ep_native.packed_unsupported: 16-bit, is_postscore, M and H multiples of 64 from 128,
    k <= min(E, 16); SwiGLU experts: eval, a recognised gate activation, no biases)"""
    rnd = random.Random(seed)
    out = []
    for case in range(n_cases):
        E = rnd.choice([1, 2, 3, 4, 8, 16, 32, 64, 64, 128, 256])
        T = rnd.choice(LAYER_T)
        k = min(E, rnd.choice([1, 2, 2, 2, 3, 4]))
        M, H = rnd.choice([128, 128, 192, 256, 512, 1024]), rnd.choice([128, 256, 256, 320, 512, 1024])
        cf = rnd.choice([0.0, 0.0, -1.0, -1.5, -2.0])
        mega = rnd.choice([0, 0, 1, 2, 4])
        dtype = rnd.choice(["bf16", "f16"])
        act = rnd.choice(["relu", "gelu", "silu"])
        fp32_gate, norm = rnd.random() < 0.5, rnd.random() < 0.7
        experts = rnd.choice(["ffn", "swiglu"])
        if experts == "swiglu" and rnd.random() < 0.7:
            act = "silu"
        while k * max(1, (T + E - 1) // E) * 2 * E * M * H * (1.5 if experts == "swiglu" else 1) > (1 << 32):   # the CPU side of a case near a second
            T = max(1, T // 2)
        out.append(dict(case=case, T=T, M=M, H=H, E=E, k=k, cf=cf, mega=mega, dtype=dtype, act=act, fp32_gate=fp32_gate, norm=norm, experts=experts,
                        graph=case % 4 == 0, seed=seed * 31 + case))
    return out


def layer_tag(d):
    return ("packed layer case {case}: T={T} M={M} H={H} E={E} k={k} cf={cf} {dtype} experts={experts} act={act} fp32_gate={fp32_gate} norm={norm} "
            "megablocks={mega} graph={graph}").format(**d)


def layer_limit_alignment(d):
    """the row limit and alignment the layer hands the packed plan (moe_layer.py: k * int(-cf * ceil(T / E)); megablocks_size where live)"""
    spe = -(-d["T"] // d["E"])
    return (d["k"] * int(-d["cf"] * spe) if d["cf"] < 0 else 0), (d["mega"] if (d["mega"] > 0 and d["E"] > 1) else 1)


def layer_classes(d):
    c = {"cf=0" if d["cf"] == 0 else "cf<0", "megablocks=%d" % d["mega"], "act=" + d["act"], "graph" if d["graph"] else "eager",
         "fp32_gate" if d["fp32_gate"] else "gate_in_dtype", "experts=" + d["experts"], d["dtype"]}
    if d["experts"] == "swiglu":   # the fused gate/up GEMM streams its weights once from E * ceil(H / 128) >= 256
        c.add("swiglu_w_once_on" if d["E"] * (-(-d["H"] // 128)) >= 256 else "swiglu_w_once_off")
    for name, on in (("E=256", d["E"] == 256), ("E=1", d["E"] == 1)):
        if on:
            c.add(name)
    return c


# =================================================================================================================================
# guard bands: an operand in the middle of a larger buffer, so that a read or a store next to it shows in an assertion
# =================================================================================================================================
MOAT_ROWS = 64        # rows of the operand's own width on each side, at least
MOAT_BYTES = 4096     # and never less than this on each side
OUT_FILL = -777.0     # the band around an output (the view itself is pre-filled by the caller)
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def moated(t, fill=None, rows=MOAT_ROWS, device=None):
    """a contiguous tensor of t's shape, values and dtype in the middle of a larger buffer on `device` (t's own by default): at least
    `rows` rows of t's width and at least 4 KiB of `fill` before and after it, the band a multiple of 16 bytes so that the view is
    aligned as a fresh allocation is.  fill: NaN for a floating tensor, SENTINEL for an integer one, unless given (an index table takes
    an in-range index: a kernel that reads past the table must not get a wild address out of it)."""
    if fill is None:
        fill = float("nan") if t.dtype.is_floating_point else SENTINEL
    es = t.element_size()
    width = int(np.prod(t.shape[1:])) if t.dim() > 1 else 1
    band = round_up(max(rows * width * es, MOAT_BYTES), 16) // es
    assert (band * es) % 16 == 0
    n = t.numel()
    buf = torch.empty([2 * band + n], dtype=t.dtype, device=device if device is not None else t.device)
    buf.fill_(fill)
    view = buf[band:band + n].view(t.shape)
    view.copy_(t)
    view._moat = (buf, band, torch.full([1], fill, dtype=t.dtype).view(_INT_VIEW[es]).item())
    return view


def moat_intact(view, what="operand"):
    """the band around a moated() view still holds its fill, bit for bit"""
    buf, band, bits = view._moat
    raw = buf.view(_INT_VIEW[buf.element_size()])
    n = view.numel()
    assert view.data_ptr() == buf.data_ptr() + band * buf.element_size() and raw.numel() == 2 * band + n, "not the view moated() returned"
    for name, part in (("before", raw[:band]), ("after", raw[band + n:])):
        ne = (part != bits).nonzero()
        assert ne.numel() == 0, f"the band {name} {what} was written: {ne.numel()} elements, the first {int(ne[0])} elements into it"


def free_token(slot, T):
    """the largest token row that no live row of a slot map names (q % T for every q >= 0), or None"""
    slot = np.asarray(slot, dtype=np.int64)
    named = np.zeros([T], dtype=bool)
    named[slot[slot >= 0] % T] = True
    free = np.nonzero(~named)[0]
    return int(free[-1]) if free.size else None


# =================================================================================================================================
# row-sampled float64 reference of the grouped GEMM (the large fixed cases: every row is compared bit for bit with a second launch,
# float64 on the first and last row of every tile and two random rows of it)
# =================================================================================================================================
def tile_sample_rows(tiles, offsets, seed, per_tile=2):
    """sorted unique rows: of every tile (e, start) its first row, its last live row (below offsets[e + 1]) and per_tile random ones"""
    g = np.random.default_rng(seed)
    rows = []
    for e, start in np.asarray(tiles, dtype=np.int64).reshape(-1, 2):
        end = min(int(start) + TILE, int(offsets[e + 1]))
        rows += [int(start), end - 1] + [int(v) for v in g.integers(int(start), end, size=per_tile)]
    return np.unique(np.array(rows, dtype=np.int64))


def ref_gemm_rows(a_rows, w, bias, kmajor, act, mul, offsets, dtype, rows):
    """ref_gemm on the packed rows `rows` only (sorted, below offsets[E]) -> (the product rounded once to dtype, the exact fp64 value
    before the rounding, |a| |W| + |b| of the same element), each [len(rows), N]"""
    E = w.shape[0]
    N = w.shape[1] if kmajor else w.shape[2]
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    exact = torch.zeros([rows.numel(), N], dtype=torch.float64)
    mag = torch.zeros_like(exact)
    owner = np.searchsorted(np.asarray(offsets, dtype=np.int64), rows.numpy(), side="right") - 1
    for e in np.unique(owner):
        sel = torch.from_numpy(np.nonzero(owner == e)[0])
        r = rows[sel]
        we = w[e].double()
        we = we.t() if kmajor else we
        A = a_rows[r].double()
        y, m = A @ we, A.abs() @ we.abs()
        if bias is not None:
            y, m = y + bias[e].double(), m + bias[e].double().abs()
        y = ACTS64[act](y)
        if mul is not None:
            y, m = y * mul[r].double(), m * mul[r].double().abs()
        exact[sel], mag[sel] = y, m
    return exact.to(dtype).double(), exact, mag


def nmajor_bound(exact, mag, K, dtype):
    """the bar of tests/test_packed_nmajor_gather_gpu.py: one rounding of an fp32 sum over K"""
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    return 1.01 * u * exact.abs() + K * 2.0 ** -24 * mag + 2.0 ** -24


# =================================================================================================================================
# f. the forms a SwiGLU training step on the packed layout relies on: the n-major GEMM with gathered rows, the k-major
# ping-pong kernel as a plain product on both sides of its weights-streamed-once switch, the weight gradient with gathered operands
# at wide N_a, N_b -- over layouts of REAL routings (k choices per token, distinct, a share masked; slot values up to k T - 1)
# =================================================================================================================================
TRAIN_T = [1, 50, 1000, 4096]
TRAIN_ALIGN = [1, 8, 128]
NM_N = [8, 120, 128, 136, 264, 1024, 2048]
NM_K = [64, 192, 1024, 2048]
WG_N = [8, 136, 512, 1024, 2048]
F64_BUDGET = 1 << 30      # multiply-adds of one float64 reference; a GEMM above it is checked on sampled rows (tile_sample_rows)
TRAIN_PROMISED = (
    {"nm:act=none", "nm:act=relu", "nm:bias", "nm:no_bias", "nm:bf16", "nm:f16", "nm:rot_on", "nm:rot_off", "nm:entries>=96", "nm:entries>256",
     "nm:many_entries_empty_between", "nm:expert>256", "nm:one_row_in_new_tile", "nm:pad_rows_align8", "nm:pad_rows_align128", "nm:slot>=T",
     "nm:N=K=2048", "nm:N=K=2048:entries>=96", "nm:masked", "nm:T=4096"}
    | {"nm:N=%d" % n for n in NM_N} | {"nm:K=%d" % k for k in NM_K}
    | {"pp:once_%s:%s:%s" % (s, g, m) for s in ("on", "off") for g in ("gather", "packed") for m in ("mul", "no_mul")}
    | {"pp:once_on:expert>256", "pp:once_off:expert>256", "pp:E=128,N=512,K=64", "pp:E=256,N=256", "pp:N=K=2048:entries>=96", "pp:slot>=T", "pp:bf16",
       "pp:f16", "pp:pad_rows", "pp:T=4096"}
    | {"wg:gather=a", "wg:gather=b", "wg:gather=none", "wg:2048x2048", "wg:16bit:gathered", "wg:f32:gathered", "wg:acc:gathered", "wg:T=4096:slot>=T",
       "wg:empty_between", "wg:bf16", "wg:f16", "wg:pad_rows"}
    | {"wg:N=%d" % n for n in WG_N})


def _routing_fields(rnd, E, t_choices=TRAIN_T + [1000, 4096]):
    T = rnd.choice(t_choices)
    return dict(T=T, k=min(E, rnd.choice([1, 2, 4])), align=rnd.choice(TRAIN_ALIGN), mode=rnd.choice(["random", "random", "skewed"]),
                mask_p=0.0 if T == 1 else rnd.choice([0.1, 0.5, 0.9]), rows=None)


def _gen_nmajor(rnd, j):
    d = dict(act=["none", "relu"][j & 1], bias=bool((j >> 1) & 1), dtype=["bf16", "f16"][(j >> 2) & 1], gather=True, mul=False)
    N, K = NM_N[j % len(NM_N)], NM_K[j % len(NM_K)]
    small_n, small_k = rnd.choice([8, 120, 128, 136]), rnd.choice([64, 192])
    E = rnd.choice([2, 3, 8, 17, 64])
    r = _routing_fields(rnd, E)
    live = [rnd.choice([1, 2, 7, 9]) for _ in range(100)]
    if j == 0:      # more than 256 tile-table entries: many experts, a few rows each
        E, N, K, r = 512, small_n, small_k, dict(T=1000, k=2, align=1, mode="random", mask_p=0.0, rows=None)
    elif j == 1:    # at least 96 entries with an empty expert between every two live ones
        E, N, K = 200, small_n, small_k
        r = dict(T=1000, k=2, align=8, mode="rows", mask_p=0.0, rows=[live[e // 2] if e % 2 == 0 else 0 for e in range(E)])
    elif j == 2:
        E, N, K, r = 3, 2048, 2048, dict(T=50, k=2, align=1, mode="random", mask_p=0.1, rows=None)
    elif j == 3:    # one row into a second and a third tile; an empty expert between live ones
        E, r = 4, dict(T=1000, k=2, align=1, mode="rows", mask_p=0.0, rows=[257, 0, 300, 513])
    elif j == 4:
        E, r = 16, dict(T=4096, k=4, align=128, mode="random", mask_p=0.5, rows=None)
    elif j == 5:
        E, N, K, r = 2, 2048, 2048, dict(T=4096, k=2, align=8, mode="random", mask_p=0.9, rows=None)
    while E * N * K > (1 << 25) and r["rows"] is None:       # the weights stay below 64 MiB: fewer experts, the same N and K
        E = max(1, E // 2)
    r["k"] = min(r["k"], E)
    return dict(d, E=E, N=N, K=K, **r)


def _gen_pp(rnd, j):
    once, gather, mul, big = bool(j & 1), bool((j >> 1) & 1), bool((j >> 2) & 1), bool((j >> 3) & 1)
    if once:        # E * ceil(N / 256) >= 256 at its smallest shapes
        E, N, K = (256, 256, 64) if (j >> 1) % 3 == 0 else (128, 512, rnd.choice([64, 64, 192]))
    else:
        E, N, K = rnd.choice([1, 2, 3, 8, 17]), rnd.choice([8, 120, 256, 264, 512, 1024, 2048]), rnd.choice(NM_K)
        while E * N * K > (1 << 25):
            E = max(1, E // 2)
    r = _routing_fields(rnd, E, [50, 1000, 4096])
    small = [rnd.choice([0, 1, 2, 7]) for _ in range(E)]
    at, rows = rnd.randrange(E), rnd.choice([257, 300, 513])
    if big:
        small[at] = rows
        r = dict(T=1000, k=min(E, 4), align=rnd.choice(TRAIN_ALIGN), mode="rows", mask_p=0.0, rows=small)
    return dict(act="none", bias=False, dtype=rnd.choice(["bf16", "f16"]), gather=gather, mul=mul, E=E, N=N, K=K, **r)


def _gen_wgrad(rnd, j):
    gather, form = ["a", "b", "none"][j % 3], ["16", "f32", "acc"][(j // 3) % 3]
    Na, Nb = WG_N[j % len(WG_N)], WG_N[(j + j // len(WG_N)) % len(WG_N)]
    E = rnd.choice([1, 2, 3, 8, 17, 64])
    r = _routing_fields(rnd, E)
    if j == 0:      # 16 x 16 output tiles per expert
        E, Na, Nb, r = 2, 2048, 2048, dict(T=4096, k=2, align=1, mode="rows", mask_p=0.0, rows=[150, 140])
    elif j == 1:
        E, r = 5, dict(T=1000, k=2, align=8, mode="rows", mask_p=0.0, rows=[70, 0, 257, 0, 3])
    elif j == 2:
        E, r = 8, dict(T=4096, k=4, align=1, mode="random", mask_p=0.9, rows=None)
    elif j == 3:
        E, r = 4, dict(T=4096, k=2, align=128, mode="random", mask_p=0.9, rows=None)
    while E * Na * Nb > (1 << 23) and r["rows"] is None:
        E = max(1, E // 2)
    r["k"] = min(r["k"], E)
    while r["rows"] is None and r["k"] * r["T"] * (1 - r["mask_p"]) * Na * Nb > F64_BUDGET:     # the float64 product of all rows: mask more tokens, T stays
        r["mask_p"] = 1 - (1 - r["mask_p"]) / 2
    return dict(gather=gather, form=form, dtype=rnd.choice(["bf16", "f16"]), E=E, Na=Na, Nb=Nb, **r)


def gen_train_form_cases(n_cases, seed):
    """cases 0 and 1: K = N = 2048 over 96 tile-table entries in one launch, n-major gathered and through the k-major ping-pong kernel
    (3 experts of 8192 rows: 8193 tokens, one of them masked, every other one choosing all three experts); then the three kinds in
    turn, the j-th case of a kind cycling through that kind's classes"""
    rnd = random.Random(seed)
    out, count = [], {"nmajor": 0, "pp": 0, "wgrad": 0}
    for case in range(n_cases):
        if case < 2:
            kind = ("nmajor", "pp")[case]
            d = dict(act="none", bias=case == 0, dtype="bf16", gather=True, mul=False, E=3, N=2048, K=2048, T=8193, k=3, align=1, mode="all3", mask_p=0.0, rows=None)
        else:
            kind = ("nmajor", "pp", "wgrad")[(case - 2) % 3]
            d = {"nmajor": _gen_nmajor, "pp": _gen_pp, "wgrad": _gen_wgrad}[kind](rnd, count[kind])
            count[kind] += 1
        out.append(dict(d, case=case, kind=kind, seed=seed * 1299709 + case))
    return out


def train_routing(d):
    """the case's expert ids [k, T] int32 (numpy): the choices of a token distinct, a share of the entries masked with -1, and (T > 1)
    one token without any live choice: the row of the token array that holds NaN and that the slot map's guard band names"""
    g = np.random.default_rng(d["seed"])
    T, E, k = d["T"], d["E"], d["k"]
    if d["mode"] == "all3":
        idx = (np.arange(T)[None, :] + np.arange(k)[:, None]) % E
        idx[:, T // 2] = -1
    elif d["mode"] == "rows":      # expert e gets rows[e] entries, spread over all tokens but one and over the k choices
        rows = np.asarray(d["rows"], dtype=np.int64)
        Tu = max(T - 1, 1)
        n = int(rows.sum())
        assert int(rows.max()) <= Tu and n <= k * Tu, "an expert is chosen at most once by a token"
        perm = g.permutation(T)
        i = np.arange(n)
        idx = np.full([k, T], -1, dtype=np.int64)
        idx[i // Tu, perm[i % Tu]] = np.repeat(np.arange(E), rows)
        idx = np.take_along_axis(idx, np.argsort(g.random([k, T]), axis=0), 0)
    else:
        idx = make_routing(d).astype(np.int64)
        if T > 1:
            idx[:, int(g.integers(T))] = -1
    return idx.astype(np.int32)


def train_tag(d):
    if d["kind"] == "wgrad":
        s = "wgrad Na={Na} Nb={Nb} gather={gather} form={form}".format(**d)
    else:
        s = "{kind} N={N} K={K} act={act} bias={bias} mul={mul} gather={gather}".format(**d)
    return ("train form case {case}: " + s + " {dtype} T={T} E={E} k={k} align={align} {mode} mask={mask_p}").format(s=s, **{**d, "mask_p": round(d["mask_p"], 4)})


def train_classes(d, ref):
    """the classes of a case and its reference layout (ref_layout of train_routing(d))"""
    E, T, align = d["E"], d["T"], d["align"]
    rows, kept, ntiles = ref["rows"], ref["kept"], ref["ntiles"]
    live = np.nonzero(rows > 0)[0]
    between = bool(live.size >= 2 and (rows[live[0]:live[-1]] == 0).any())
    slot_hi = bool((ref["slot"] >= T).any())
    pad = bool((rows > kept).any())
    big = bool((rows > TILE).any())
    masked = bool((train_routing(d) < 0).any())
    c = set()
    if d["kind"] == "wgrad":
        gathered_ = d["gather"] != "none"
        on = [("gather=" + d["gather"], True), ("2048x2048", d["Na"] == 2048 and d["Nb"] == 2048 and E <= 2 and int(ref["offsets"][-1]) <= 300),
              ({"16": "16bit", "f32": "f32", "acc": "acc"}[d["form"]] + ":gathered", gathered_), ("T=4096:slot>=T", T == 4096 and slot_hi and gathered_),
              ("empty_between", between), (d["dtype"], True), ("pad_rows", pad), ("N=%d" % d["Na"], True), ("N=%d" % d["Nb"], True)]
        return {"wg:" + n for n, v in on if v}
    N, K = d["N"], d["K"]
    if d["kind"] == "nmajor":
        on = [("act=" + d["act"], True), ("bias" if d["bias"] else "no_bias", True), (d["dtype"], True), ("N=%d" % N, True), ("K=%d" % K, True),
              ("rot_on" if ref["capacity"] < 256 else "rot_off", True), ("entries>=96", ntiles >= 96), ("entries>256", ntiles > 256),
              ("many_entries_empty_between", ntiles >= 96 and between), ("expert>256", big), ("one_row_in_new_tile", bool((rows % TILE == 1).any() and big)),
              ("pad_rows_align8", pad and align == 8), ("pad_rows_align128", pad and align == 128), ("slot>=T", slot_hi), ("N=K=2048", N == 2048 and K == 2048),
              ("N=K=2048:entries>=96", N == 2048 and K == 2048 and ntiles >= 96), ("masked", masked), ("T=4096", T == 4096)]
        return {"nm:" + n for n, v in on if v}
    once = "once_on" if E * (-(-N // 256)) >= 256 else "once_off"
    on = [("%s:%s:%s" % (once, "gather" if d["gather"] else "packed", "mul" if d["mul"] else "no_mul"), True), (once + ":expert>256", big),
          ("E=128,N=512,K=64", (E, N, K) == (128, 512, 64)), ("E=256,N=256", (E, N) == (256, 256)), ("N=K=2048:entries>=96", N == 2048 and K == 2048 and ntiles >= 96),
          ("slot>=T", slot_hi and d["gather"]), (d["dtype"], True), ("pad_rows", pad), ("T=4096", T == 4096)]
    return {"pp:" + n for n, v in on if v}


def check_promised(what, seen, promised, n_cases, default_n):
    """at the default length (and beyond: the first cases are the same) every promised edge class was drawn"""
    if n_cases >= default_n:
        missing = sorted(promised - seen)
        assert not missing, f"{what}: edge classes never drawn in {n_cases} cases: {missing}"
