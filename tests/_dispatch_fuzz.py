"""TEST-ONLY pieces shared by the fuzzers of csrc/dispatch.hip (tests/test_dispatch_fuzz_gpu.py: fast_encode, fast_decode in its four launch
shapes and the any-k kernel, the padded gate gradient) and their GPU-free checks (tests/test_dispatch_fuzz_cpu.py): the seeded case
generators, the edge classes each fuzzer promises to draw, and the references.  The references are written from the operations'
definitions (the header comment of csrc/dispatch.hip, the docstrings of ops.fast_encode / ops.fast_decode / ops.gate_grad), in numpy fp32
for encode and decode and in float64 for the gate gradient -- not from the kernels.  What IS taken from the kernels is the list of places
where they branch (the row lengths, the thresholds of the launch shapes, the names of the classes): that is what a fuzzer has to reach.
Nothing here needs a GPU or the library.

  decode   out[t] = cast(sum_j fp32(gate[j, t] * buf[row(idx[j, t], loc[j, t])])), the k products added left to right in fp32; a choice with
           idx < 0 or loc >= C contributes 0.f
  encode   out[row(e, l)] = cast(fp32(gate[q] * x[q % T])) for the entry q = j * T + t kept at (e, l); a copy without gates; zeros elsewhere
  row(e, l) plain e * C + l; chunk-major [C/c][E][c]; expert-sliced [E_loc/s][W][s][C] (rank w owns the experts [w * E_loc, (w + 1) * E_loc))
  gate gradient   ggate[j, t] = <buf[e * C + l], x[t]> in float64; exactly 0.0 for a dropped or masked entry"""
import random

import numpy as np
import torch

import _packed_fuzz as F

# ---- the dimensions the issue of this fuzzer sets ------------------------------------------------------------------------------------
V_CHOICES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 385, 448, 449, 512, 513, 577, 641, 1030]   # 16-byte vectors per row
TAIL_M = {"16": [1, 7, 50, 100, 1023, 1028, 4100], "32": [1, 7, 50, 515, 1023]}        # rows that are no whole number of vectors
SPLIT_EDGE_M = {"16": [1016, 1024], "32": [508, 512]}                                  # 2032 / 2048 bytes: the split's threshold from both sides
T_CHOICES = [1, 2, 3, 4, 5, 63, 64, 65, 130]
E_CHOICES = [1, 2, 3, 8, 16, 24, 32]
K_CHOICES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 24]
K_WEIGHTED = [1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4] + K_CHOICES          # the unrolled loops are longest at small k
SCALES = [1e-3, 1.0, 8.0]
ROW_DTYPES = ["bf16", "f16", "f32"]
GATE_KINDS = ["none", "f32", "bf16", "f16"]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
LAYOUTS = ["plain", "chunk", "sliced"]
CAP_MODES = ["largest", "largest", "half", "half", "one", "zero"]
BUDGET = 1 << 23          # elements of the largest operand of a case: rows * M, by construction
GRID_ROWS = 8192          # wave-rows of the largest grid (256 CUs x 8 blocks x 4 waves): beyond it a wave strides
SPLIT_BYTES = 2048        # rows at least this long are split over two waves when TUTEL_OPT_DECODE has bit 0


def vec_elems(dtype):
    return 4 if dtype == "f32" else 8


def width(dtype):
    return "32" if dtype == "f32" else "16"


def row_lengths(dtype):
    """every row length (in elements) a fuzzer sweeps for this row dtype"""
    lens = [v * vec_elems(dtype) for v in V_CHOICES] + TAIL_M[width(dtype)]
    return lens + [m for m in SPLIT_EDGE_M[width(dtype)] if m not in lens]       # (127 and 128 vectors: already there)


def short_lengths(dtype):
    return [m for m in row_lengths(dtype) if m <= 64]


# =================================================================================================================================
# the routing of a case and its capacity
# =================================================================================================================================
def routing(d):
    """-> idx, loc [k, T] int32 (numpy), counts [E], C: k distinct expert ids per token drawn directly (F.make_routing: the routing kernels stop
    at k = 16), a share masked with -1; locations = the stable rank inside the expert (F.ref_locations); C from the case's capacity mode,
    lowered where E * C * M would pass the budget (a lower capacity only drops more)"""
    idx = F.make_routing(d)
    loc, cnt = F.ref_locations(idx, d["E"])
    top = int(cnt.max()) if cnt.size else 0
    C = {"largest": top, "half": max(1, (top + 1) // 2) if top else 0, "one": min(1, top), "zero": 0}[d["cap"]]
    C = min(C, BUDGET // (d["E"] * d["M"]))
    return idx, loc, cnt, C


def keep_mask(idx, loc, C):
    return (idx >= 0) & (loc >= 0) & (loc < C)


def row_order(E, C, layout, chunk=0, s=0, W=1):
    """order[pos] = the plain row e * C + l that stands at row pos of the buffer: the definition of the two bucket orders of the overlapped
    all-to-all as reshapes of the plain [E, C] table"""
    plain = np.arange(E * C, dtype=np.int64).reshape(E, C)
    if layout == "chunk":
        assert chunk >= 1 and C % chunk == 0
        return plain.reshape(E, C // chunk, chunk).transpose(1, 0, 2).reshape(-1)          # [C/c][E][c]
    if layout == "sliced":
        assert s >= 1 and E % W == 0 and (E // W) % s == 0
        return plain.reshape(W, E // W // s, s, C).transpose(1, 0, 2, 3).reshape(-1)       # [E_loc/s][W][s][C]
    return plain.reshape(-1)


def _divisors(n):
    return [v for v in range(1, n + 1) if n % v == 0]


def layout_args(d, C):
    """the case's bucket order -> (layout, chunk_rows, expert_slice, ep_world); a capacity of 0 has no rows to order"""
    g = random.Random(d["seed"] + 17)
    E = d["E"]
    if C == 0 or d["layout"] == "plain":
        return "plain", 0, 0, 1
    if d["layout"] == "chunk":
        return "chunk", g.choice(_divisors(C)), 0, 1
    W = g.choice(_divisors(E))
    return "sliced", 0, g.choice(_divisors(E // W)), W


# =================================================================================================================================
# references
# =================================================================================================================================
def _f32(t):
    return t.float().numpy()


def ref_decode(buf, idx, loc, gates, C):
    """buf [E * C, M] in PLAIN order (torch, the row dtype), idx / loc [k, T] (numpy), gates [k, T] (torch) | None -> [T, M] in buf's dtype"""
    k, T = idx.shape
    b = _f32(buf)
    acc = None
    for j in range(k):
        keep = keep_mask(idx[j], loc[j], C)
        f = np.zeros([T, buf.shape[1]], dtype=np.float32)
        rows = b[idx[j][keep].astype(np.int64) * C + loc[j][keep]]
        if gates is not None:
            rows = _f32(gates[j])[keep][:, None] * rows          # one fp32 product
        f[keep] = rows
        acc = f if acc is None else acc + f                      # left to right, in fp32
    assert acc.dtype == np.float32
    return torch.from_numpy(acc).to(buf.dtype)


def ref_slot_map(idx, loc, E, C):
    """[E * C] int64, plain order: the entry q = j * T + t kept at row e * C + l, -1 for an empty slot"""
    keep = keep_mask(idx, loc, C).reshape(-1)
    q = np.nonzero(keep)[0]
    slot = np.full([E * C], -1, dtype=np.int64)
    rows = idx.reshape(-1)[q].astype(np.int64) * C + loc.reshape(-1)[q]
    assert np.unique(rows).size == rows.size, "two entries in one slot"
    slot[rows] = q
    return slot


def ref_encode(x, idx, loc, gates, E, C):
    """x [T, M] (torch), gates [k, T] (torch) | None -> [E * C, M] in PLAIN order, x's dtype"""
    T, M = x.shape
    slot = ref_slot_map(idx, loc, E, C)
    live = slot >= 0
    q = slot[live]
    rows = _f32(x)[q % T]
    if gates is not None:
        rows = _f32(gates.reshape(-1))[q][:, None] * rows        # one fp32 product
    out = np.zeros([E * C, M], dtype=np.float32)
    out[live] = rows
    return torch.from_numpy(out).to(x.dtype)


def ref_gate_grad(x, buf, idx, loc, C):
    """-> (ggate [k, T] float64, sum |row_i x_i| [k, T] float64, keep [k, T]): zeros where the entry was dropped or masked"""
    k, T = idx.shape
    keep = keep_mask(idx, loc, C)
    ref, mag = torch.zeros([k, T], dtype=torch.float64), torch.zeros([k, T], dtype=torch.float64)
    x64, b64 = x.double(), buf.double()
    for j in range(k):
        m = torch.from_numpy(keep[j])
        rows = torch.from_numpy(idx[j][keep[j]].astype(np.int64) * C + loc[j][keep[j]])
        p = b64[rows] * x64[m]
        ref[j, m], mag[j, m] = p.sum(1), p.abs().sum(1)
    return ref, mag, torch.from_numpy(keep)


def gate_grad_bound(mag, M):
    """a chain of at most M / 64 + 8 fp32 terms per lane, six butterfly adds and the rounding of each product, every one within 2^-24 of a
    partial sum of magnitude at most sum |row_i x_i|"""
    return 1.01 * (M / 64 + 16) * 2.0 ** -24 * mag


def emulate_gate_grad(x, buf, idx, loc, C, dtype):
    """the summation order of a wave in numpy fp32: lane L owns the 16-byte vectors L, L + 64, ... of the row (the elements L, L + 64, ...
    where the row is no whole number of vectors) and adds their products in order; the 64 lane sums meet in a six-step butterfly (lane
    L adds lane L ^ 32, then ^ 16, ... ^ 1) -> [k, T] fp32 (0 for a dropped entry)"""
    k, T = idx.shape
    M = x.shape[1]
    vn = vec_elems(dtype) if M % vec_elems(dtype) == 0 else 1
    keep = keep_mask(idx, loc, C).reshape(-1)
    q = np.nonzero(keep)[0]
    out = np.zeros([k * T], dtype=np.float32)
    if q.size:
        rows = idx.reshape(-1)[q].astype(np.int64) * C + loc.reshape(-1)[q]
        p = _f32(buf)[rows] * _f32(x)[q % T]                     # products rounded to fp32
        per = 64 * vn
        passes = -(-M // per)
        p = np.concatenate([p, np.zeros([q.size, passes * per - M], dtype=np.float32)], axis=1).reshape(q.size, passes, 64, vn)
        acc = np.zeros([q.size, 64], dtype=np.float32)
        for i in range(passes):
            for u in range(vn):
                acc = acc + p[:, i, :, u]
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ o]
        assert acc.dtype == np.float32
        out[q] = acc[:, 0]
    return torch.from_numpy(out.reshape(k, T))


# =================================================================================================================================
# generators: one random.Random stream, consumed case by case, so that the first n cases do not depend on how many follow.  Case i sweeps
# the row dtypes (i % 3) and, within a dtype, the row lengths in order: 96 cases hold every length in every dtype, and six grid-stride cases.
# =================================================================================================================================
SWEEP, PERIOD = 90, 96       # of every 96 cases the first 90 sweep the (at most 30) row lengths of 3 dtypes, the last 6 are the grid_stride class


def is_stride_case(case):
    return case % PERIOD >= SWEEP


def _dims(rnd, case, seed, mult, k_choices=K_WEIGHTED, stride_T=(8200,), stride_k=None):
    dtype = ROW_DTYPES[case % 3]
    lens = row_lengths(dtype)
    assert 3 * len(lens) <= SWEEP
    M = lens[(case % PERIOD) // 3 % len(lens)]
    k = rnd.choice(k_choices)
    T = rnd.choice(T_CHOICES)
    cap = rnd.choice(CAP_MODES)
    mask_p = rnd.choice([0.0, 0.0, 0.1, 0.5])
    short = rnd.choice(short_lengths(dtype))
    if is_stride_case(case):    # the grid_stride class: more rows than the largest grid has waves, short rows
        j = (case // PERIOD) * (PERIOD - SWEEP) + case % PERIOD - SWEEP
        T = stride_T[j % len(stride_T)]
        M = SPLIT_EDGE_M[width(dtype)][1] if T == 4100 else short
        if T == 4100:           # (two waves per token there: 8200 wave-rows; small k keeps the buffer inside the budget)
            k = rnd.choice([1, 2])
        elif stride_k:
            k = rnd.choice(stride_k)
        cap, mask_p = rnd.choice(["largest", "half"]), rnd.choice([0.0, 0.1])
    E = rnd.choice([e for e in E_CHOICES if e >= k])
    assert T * M <= BUDGET
    return dict(case=case, T=T, E=E, k=k, M=M, dtype=dtype, cap=cap, mask_p=mask_p, mode=rnd.choice(["random", "random", "skewed", "all_on_k"]),
                scale=rnd.choice(SCALES), gates=rnd.choice(GATE_KINDS), layout=rnd.choice(LAYOUTS), seed=seed * mult + case)


def _values(d, shape, g, integer=False):
    if integer:
        return torch.randint(-3, 4, shape, generator=g).to(DTYPES[d["dtype"]])
    return (torch.randn(shape, generator=g) * d["scale"]).to(DTYPES[d["dtype"]])


def _gates(d, g):
    """fp32 with full mantissas (signed), or rounded to a 16-bit type; None for the plain sum / copy"""
    if d["gates"] == "none":
        return None
    return (torch.rand([d["k"], d["T"]], generator=g) * 2 - 1).to(DTYPES[d["gates"]])


def _common_classes(d, idx, loc, C):
    c = {"%s:gates=%s" % (d["dtype"], d["gates"]), "k=%d" % d["k"]}
    valid = idx >= 0
    for name, on in (("C=0", C == 0), ("masked", bool((~valid).any())), ("drops", C > 0 and bool((valid & (loc >= C)).any())),
                     ("nothing_dropped", C > 0 and not bool((valid & (loc >= C)).any())), ("T=1", d["T"] == 1),
                     ("scalar_tail", d["M"] % vec_elems(d["dtype"]) != 0)):
        if on:
            c.add(name)
    return c


# ---- a. decode ---------------------------------------------------------------------------------------------------------------------
def kmax_of(k):
    return k if k <= 8 else (12 if k <= 12 else 16)


def unr_of(kmax, split):
    return 1 if kmax * split >= 8 else 8 // (kmax * split)


def wave_trace(lo, hi, unr):
    """the largest number of unrolled passes (unr vectors per lane each) and of single-vector passes after them that a lane of the wave
    over the vectors [lo, hi) makes"""
    passes = rem = 0
    for lane in range(64):
        i, p, r = lo + lane, 0, 0
        while i + 64 * (unr - 1) < hi:
            i, p = i + 64 * unr, p + 1
        while i < hi:
            i, r = i + 64, r + 1
        passes, rem = max(passes, p), max(rem, r)
    return passes, rem


def split_per(nvec):
    return -(-(-(-nvec // 2)) // 64) * 64        # round_up_64(ceil(nvec / 2))


# (UNR = 1 has no "rem" class: its unrolled loop IS the single-vector loop, nothing is left for the one after it)
DECODE_PROMISED = ({"mode=%d" % m for m in range(4)} | {"UNR=%d:%s" % (u, r) for u in (8, 4, 2) for r in ("exact", "rem")}
                   | {"UNR=1", "UNR=4:two_passes+rem", "split:UNR=4:exact", "split:UNR=4:rem", "split:UNR=2:exact", "split:UNR=2:rem", "split:second_wave_one_vector",
                      "split_requested_but_short", "scalar_tail_with_split", "scalar_tail", "C=0", "masked", "drops", "nothing_dropped", "grid_stride",
                      "grid_stride_split", "T=1", "just_below_split", "at_split"}
                   | {"KMAX=%d" % kmax_of(k) for k in K_CHOICES if k <= 16} | {"k=%d" % k for k in K_CHOICES}
                   | {"anyk:%s:%s" % (lay, w) for lay in LAYOUTS for w in ("16", "32")}
                   | {"layout=" + lay for lay in LAYOUTS}
                   | {"%s:gates=%s" % (r, g) for r in ROW_DTYPES for g in GATE_KINDS})


# row lengths (in vectors) that take a fixed k: the passes of the most unrolled loops come out whole (512 at UNR = 8, 256 at UNR = 4, 128
# at UNR = 2) or leave a remainder, without the split and (1030, 513, 257 at k = 1 and 2) with it
UNROLL_K = {512: 1, 513: 1, 449: 1, 1030: 1, 641: 1, 256: 2, 257: 2, 320: 2, 128: 3, 129: 4}


def gen_decode_cases(n_cases, seed):
    rnd = random.Random(seed)
    out, anyk, free = [], {"16": 0, "32": 0}, 0
    reg = [k for k in K_CHOICES if k <= 16]
    for case in range(n_cases):
        d = _dims(rnd, case, seed, 32452843, stride_T=(8200, 4100))
        v = d["M"] // vec_elems(d["dtype"])
        if is_stride_case(case):
            pass
        elif d["M"] % vec_elems(d["dtype"]) == 0 and v in UNROLL_K:
            d["k"], d["cap"], d["mask_p"] = UNROLL_K[v], rnd.choice(["largest", "half"]), rnd.choice([0.0, 0.1])
        elif case % 4 == 1:     # the any-k kernel in every bucket order, in both widths
            w = width(d["dtype"])
            d["k"], d["layout"], d["cap"], d["T"] = rnd.choice([17, 24]), LAYOUTS[anyk[w] % 3], rnd.choice(["largest", "half"]), max(d["T"], 2)
            anyk[w] += 1
        else:                   # every register-resident instantiation in turn
            d["k"] = reg[free % len(reg)]
            free += 1
        d["E"] = rnd.choice([e for e in E_CHOICES if e >= d["k"]])
        out.append(d)
    return out


def decode_case(d):
    """the case's operands on the CPU: buf in the case's bucket order (at least one row: NaN where E * C = 0, a row nothing may read), the
    routing, the gates, and the reference"""
    g = torch.Generator().manual_seed(d["seed"])
    idx, loc, cnt, C = routing(d)
    E, M = d["E"], d["M"]
    layout, chunk, s, W = layout_args(d, C)
    plain = _values(d, [E * C, M], g)
    gates = _gates(d, g)
    want = ref_decode(plain, idx, loc, gates, C)
    buf = plain[torch.from_numpy(row_order(E, C, layout, chunk, s, W))] if E * C else torch.full([1, M], float("nan"), dtype=plain.dtype)
    return dict(idx=idx, loc=loc, C=C, layout=layout, chunk=chunk, s=s, W=W, plain=plain, buf=buf, gates=gates, want=want)


def decode_tag(d, c=None):
    s = "dispatch decode case {case}: T={T} E={E} k={k} M={M} {dtype} gates={gates} cap={cap} mask={mask_p} {mode} scale={scale}".format(**d)
    return s + (" C={C} {layout} chunk={chunk} slice={s} W={W}".format(**c) if c else "")


def decode_classes(d, c):
    idx, loc, C = c["idx"], c["loc"], c["C"]
    T, k, M, dtype = d["T"], d["k"], d["M"], d["dtype"]
    vn = vec_elems(dtype)
    cls = _common_classes(d, idx, loc, C) | {"layout=" + c["layout"]}
    if k > 16:
        if C > 0:
            cls.add("anyk:%s:%s" % (c["layout"], width(dtype)))
        return cls
    cls.add("KMAX=%d" % kmax_of(k))
    if C == 0:
        return cls
    cls |= {"mode=%d" % m for m in range(4)}
    long_row = M * (4 if dtype == "f32" else 2) >= SPLIT_BYTES
    for name, on in (("split_requested_but_short", not long_row), ("scalar_tail_with_split", long_row and M % vn != 0),
                     ("grid_stride", T > GRID_ROWS), ("grid_stride_split", long_row and GRID_ROWS // 2 < T <= GRID_ROWS),
                     ("just_below_split", M == SPLIT_EDGE_M[width(dtype)][0]), ("at_split", M == SPLIT_EDGE_M[width(dtype)][1])):
        if on:
            cls.add(name)
    if M % vn == 0:
        nvec = M // vn
        waves = [("", 1, 0, nvec)]
        if long_row:
            per = split_per(nvec)
            waves += [("split:", 2, p * per, min(nvec, (p + 1) * per)) for p in range(2)]
            if nvec - per == 1:
                cls.add("split:second_wave_one_vector")
        for pre, split, lo, hi in waves:
            unr = unr_of(kmax_of(k), split)
            passes, rem = wave_trace(lo, hi, unr)
            if unr == 1:
                cls.add("UNR=1")
            elif passes:
                for p in {pre, ""}:
                    cls.add("%sUNR=%d:%s" % (p, unr, "rem" if rem else "exact"))
                    if passes >= 2 and rem:
                        cls.add("%sUNR=%d:two_passes+rem" % (p, unr))
    return cls


# ---- b. encode ---------------------------------------------------------------------------------------------------------------------
ENCODE_PROMISED = ({"%s:%s" % (lay, g) for lay in LAYOUTS for g in ("copy", "gated")} | {"V>192", "copy:unrolled:exact", "copy:unrolled:rem", "gated:V>64",
                   "scalar_tail", "C=0", "masked", "drops", "nothing_dropped", "grid_stride", "T=1", "empty_slots", "no_empty_slot"}
                   | {"%s:gates=%s" % (r, g) for r in ROW_DTYPES for g in GATE_KINDS} | {"k=%d" % k for k in K_CHOICES})


def gen_encode_cases(n_cases, seed):
    rnd = random.Random(seed)
    return [_dims(rnd, case, seed, 49979687, k_choices=K_CHOICES + [1, 2, 2], stride_k=[2, 3]) for case in range(n_cases)]


def encode_case(d):
    """the case's operands on the CPU: x, the plain slot map (at least one entry: -1 where E * C = 0), the gates, and the reference in the
    case's output order"""
    g = torch.Generator().manual_seed(d["seed"])
    idx, loc, cnt, C = routing(d)
    if is_stride_case(d["case"]):     # the grid_stride class: the largest count as the capacity, so that n_slots = E * C > 8192 rows
        C = min(int(cnt.max()), BUDGET // (d["E"] * d["M"]))
    E, T, M = d["E"], d["T"], d["M"]
    layout, chunk, s, W = layout_args(d, C)
    x = _values(d, [T, M], g)
    gates = _gates(d, g)
    plain = ref_encode(x, idx, loc, gates, E, C)
    slot = ref_slot_map(idx, loc, E, C)
    want = plain[torch.from_numpy(row_order(E, C, layout, chunk, s, W))]
    return dict(idx=idx, loc=loc, C=C, layout=layout, chunk=chunk, s=s, W=W, x=x, gates=gates, slot=slot, plain=plain, want=want)


def encode_tag(d, c=None):
    s = "dispatch encode case {case}: T={T} E={E} k={k} M={M} {dtype} gates={gates} cap={cap} mask={mask_p} {mode} scale={scale}".format(**d)
    return s + (" C={C} {layout} chunk={chunk} slice={s} W={W}".format(**c) if c else "")


def encode_classes(d, c):
    idx, loc, C = c["idx"], c["loc"], c["C"]
    M, dtype = d["M"], d["dtype"]
    vn = vec_elems(dtype)
    cls = _common_classes(d, idx, loc, C)
    if C == 0:
        return cls
    kind = "copy" if d["gates"] == "none" else "gated"
    cls.add("%s:%s" % (c["layout"], kind))
    live = c["slot"] >= 0
    cls.add("empty_slots" if not bool(live.all()) else "no_empty_slot")
    if d["E"] * C > GRID_ROWS:
        cls.add("grid_stride")
    if M % vn == 0 and bool(live.any()):
        nvec = M // vn
        if nvec > 192:
            cls.add("V>192")
            if kind == "copy":
                cls.add("copy:unrolled:" + ("rem" if wave_trace(0, nvec, 4)[1] else "exact"))
        if kind == "gated" and nvec > 64:
            cls.add("gated:V>64")
    return cls


# ---- c. gate gradient --------------------------------------------------------------------------------------------------------------------
GGRAD_PROMISED = ({"%s:%s" % (r, p) for r in ROW_DTYPES for p in ("vector", "scalar_tail", "integer")}
                  | {"C=0", "masked", "drops", "nothing_dropped", "grid_stride", "T=1", "passes>1", "partial_last_pass", "whole_passes", "M=1"}
                  | {"k=%d" % k for k in K_CHOICES})


def gen_ggrad_cases(n_cases, seed):
    rnd = random.Random(seed)
    out = []
    for case in range(n_cases):
        d = _dims(rnd, case, seed, 67867967, k_choices=K_CHOICES + [1, 2, 2])
        d["gates"], d["layout"] = "none", "plain"
        d["integer"] = case % 4 == 1        # operands from {-3 ... 3}: every partial sum is exact in fp32
        out.append(d)
    return out


def ggrad_case(d):
    g = torch.Generator().manual_seed(d["seed"])
    idx, loc, cnt, C = routing(d)
    E, T, M = d["E"], d["T"], d["M"]
    x = _values(d, [T, M], g, d["integer"])
    buf = _values(d, [max(E * C, 1), M], g, d["integer"])
    if E * C == 0:
        buf.fill_(float("nan"))             # (a row nothing may read)
    ref, mag, keep = ref_gate_grad(x, buf, idx, loc, C)
    return dict(idx=idx, loc=loc, C=C, x=x, buf=buf, ref=ref, mag=mag, keep=keep)


def ggrad_tag(d, c=None):
    s = "dispatch gate-grad case {case}: T={T} E={E} k={k} M={M} {dtype} cap={cap} mask={mask_p} {mode} scale={scale} integer={integer}".format(**d)
    return s + (" C=%d" % c["C"] if c else "")


def ggrad_classes(d, c):
    idx, loc, C = c["idx"], c["loc"], c["C"]
    M, dtype = d["M"], d["dtype"]
    vn = vec_elems(dtype)
    cls = {n for n in _common_classes(d, idx, loc, C) if ":gates=" not in n and n != "scalar_tail"}
    if d["k"] * d["T"] > GRID_ROWS:
        cls.add("grid_stride")
    if C == 0 or not bool(c["keep"].any()):
        return cls
    cls.add("%s:%s" % (dtype, "vector" if M % vn == 0 else "scalar_tail"))
    if d["integer"]:
        cls.add("%s:integer" % dtype)
    per = 64 * (vn if M % vn == 0 else 1)
    for name, on in (("passes>1", M > per), ("partial_last_pass", M % per != 0), ("whole_passes", M % per == 0), ("M=1", M == 1)):
        if on:
            cls.add(name)
    return cls


check_promised = F.check_promised
