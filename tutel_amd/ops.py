"""Tensor-level wrappers over the C ABI (include/tutel_amd.h).

PyTorch is plumbing here: it owns the HBM allocations and the current HIP stream; every op
below hands raw device pointers + sizes + that stream to libtutel_amd.so.  All ops require HIP
device tensors and raise otherwise -- there is no CPU or eager implementation behind them.
"""
import ctypes

import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
ACT_CODES = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU, "silu": _lib.ACT_SILU}


def _code(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise _lib.TutelAmdError(f"tutel_amd: dtype {t.dtype} is not supported by the HIP kernels") from None


def _dev(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.TutelAmdError(
                "tutel_amd: the MoE hot path runs on the HIP device only (got a CPU tensor); "
                "there is no CPU fallback.")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _a16(t):
    """an ACTIVATION operand at a 16-byte aligned address: the kernels fetch rows as 16-byte vectors, upstream's take any contiguous
    tensor -- an offset view (a slice of a larger buffer) is copied into a fresh allocation instead of failing the call.  (Weights are
    not copied per call: a misaligned parameter tensor fails loudly in the C ABI.)"""
    if t is None or t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream (raw getter: ~0.3 us instead of ~10 us for the Stream object)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def supported_dtype(dtype):
    return dtype in _DT


def routing_dtype(dtype):
    """dtypes the top-k kernel takes natively (fp64 scores are compared and normalised in fp64)."""
    return dtype in _DT or dtype == torch.float64


# ---------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------
def routing_workspace(T, E, k, device):
    n = _lib.lib().tutel_amd_routing_workspace_bytes(T, E, k)
    return torch.empty([max(int(n), 4)], dtype=torch.uint8, device=device)


def gate_topk(inp, k, apply_softmax=False, normalize_gate=True, want_scores=False, ws=None, clear=None):
    """inp [T,E] scores (or logits with apply_softmax) -> idx [k,T] i32, gates [k,T], ws, scores|None.
    clear: optional int32 tensor this launch also fills with -1 (the slot_map of the next call)."""
    _dev(inp)
    assert inp.dim() == 2
    inp = inp.contiguous()
    T, E = inp.shape
    k = min(int(k), E)
    idx = torch.empty([k, T], dtype=torch.int32, device=inp.device)
    gates = torch.empty([k, T], dtype=inp.dtype, device=inp.device)
    scores = torch.empty_like(inp) if (want_scores and apply_softmax) else None
    if ws is None:
        ws = routing_workspace(T, E, k, inp.device)
    L = _lib.lib()
    code = _lib.F64 if inp.dtype == torch.float64 else _code(inp)
    _lib.check(L.tutel_amd_gate_topk(_ptr(inp), code, int(bool(apply_softmax)), T, E, k,
                                     int(bool(normalize_gate)), _ptr(scores), _ptr(idx), _ptr(gates),
                                     _ptr(ws), ws.numel(), _ptr(clear), clear.numel() if clear is not None else 0,
                                     _stream()), "tutel_amd_gate_topk")
    return idx, gates, ws, (scores if apply_softmax else inp)


def gate_proj_splits(T, M, E, dtype):
    """split count of the native gate projection for this shape (0: not covered -> F.linear + gate_topk)"""
    if dtype not in (torch.bfloat16, torch.float16):
        return 0
    return int(_lib.lib().tutel_amd_gate_proj_splits(int(T), int(M), int(E), _lib.BF16 if dtype == torch.bfloat16 else _lib.F16))


def gate_proj(x, wg, partials=None):
    """x [T, M], wg [E, M] (16-bit) -> fp32 partial sums [S, T, E] of x @ wg^T (split-K, csrc/gate_proj.hip); None when the shape is
    not covered.  gate_topk_partials() adds them in split order and rounds once to x.dtype."""
    _dev(x)
    assert x.dim() == 2 and wg.dim() == 2 and x.shape[1] == wg.shape[1] and x.dtype == wg.dtype
    T, M = x.shape
    E = wg.shape[0]
    S = gate_proj_splits(T, M, E, x.dtype)
    if S == 0 or T == 0:
        return None
    x, wg = x.contiguous(), wg.contiguous()
    if partials is None:
        partials = torch.empty([S, T, E], dtype=torch.float32, device=x.device)
    assert partials.numel() >= S * T * E and partials.dtype == torch.float32
    _lib.check(_lib.lib().tutel_amd_gate_proj(_ptr(x), _ptr(wg), _code(x), T, M, E, _ptr(partials), partials.numel() * 4, _stream()),
               "tutel_amd_gate_proj")
    return partials


def gate_proj_f32w_splits(T, M, E, dtype):
    """split count of the fp32-weight gate projection (fp32 gate over tokens of `dtype`) for this shape; 0: not covered"""
    if dtype not in (torch.bfloat16, torch.float16):
        return 0
    return int(_lib.lib().tutel_amd_gate_proj_f32w_splits(int(T), int(M), int(E), _DT[dtype]))


def gate_proj_f32w_ranges(T, M, E, dtype):
    """the ordering contract of gate_proj_f32w (include/tutel_amd.h): [(m_begin, m_end)] per split -- split s accumulates
    fmaf(float(x[t, m]), wg[e, m], acc) over its range in ascending m, from 0"""
    S = gate_proj_f32w_splits(T, M, E, dtype)
    if S == 0:
        return []
    L = 64 * -(-(M // 64) // S)
    return [(s * L, min(M, (s + 1) * L)) for s in range(S)]


def gate_proj_f32w(x, wg, partials=None):
    """x [T, M] bf16 / fp16, wg [E, M] fp32 -> fp32 partial sums [S, T, E] of x.float() @ wg^T on the exact-f32 MFMA (split-K,
    csrc/gate_proj.hip); None when the shape is not covered.  gate_topk_partials(.., torch.float32, ..) adds them in split order."""
    _dev(x, wg)
    assert x.dim() == 2 and wg.dim() == 2 and x.shape[1] == wg.shape[1] and wg.dtype == torch.float32
    T, M = x.shape
    E = wg.shape[0]
    S = gate_proj_f32w_splits(T, M, E, x.dtype)
    if S == 0 or T == 0:
        return None
    x, wg = x.contiguous(), wg.contiguous()
    if partials is None:
        partials = torch.empty([S, T, E], dtype=torch.float32, device=x.device)
    assert partials.numel() >= S * T * E and partials.dtype == torch.float32
    _lib.check(_lib.lib().tutel_amd_gate_proj_f32w(_ptr(x), _ptr(wg), _code(x), T, M, E, _ptr(partials), partials.numel() * 4, _stream()),
               "tutel_amd_gate_proj_f32w")
    return partials


def gate_topk_partials(partials, dtype, k, normalize_gate=True, want_logits=False, want_scores=False, ws=None, clear=None):
    """partials [S, T, E] fp32 (gate_proj / gate_proj_f32w) -> idx [k,T] i32, gates [k,T] dtype, ws, logits|None, scores|None:
    softmax + top-k on logits = dtype(sum_s partials[s]), exactly as gate_topk(logits, apply_softmax=True).  dtype float32 (the
    partial sums of gate_proj_f32w): the fp32 sum in split order is the logit."""
    _dev(partials)
    assert partials.dim() == 3 and partials.dtype == torch.float32 and partials.is_contiguous()
    S, T, E = partials.shape
    k = min(int(k), E)
    dev = partials.device
    idx = torch.empty([k, T], dtype=torch.int32, device=dev)
    gates = torch.empty([k, T], dtype=dtype, device=dev)
    logits = torch.empty([T, E], dtype=dtype, device=dev) if want_logits else None
    scores = torch.empty([T, E], dtype=dtype, device=dev) if want_scores else None
    if ws is None:
        ws = routing_workspace(T, E, k, dev)
    code = _DT[dtype]
    _lib.check(_lib.lib().tutel_amd_gate_topk_partials(_ptr(partials), S, code, T, E, k, int(bool(normalize_gate)), _ptr(logits),
                                                       _ptr(scores), _ptr(idx), _ptr(gates), _ptr(ws), ws.numel(), _ptr(clear),
                                                       clear.numel() if clear is not None else 0, _stream()),
               "tutel_amd_gate_topk_partials")
    return idx, gates, ws, logits, scores


def gate_logits(x, wg):
    """x @ wg^T through the split-K kernel, in wg's dtype: the SAME logits, bit for bit, that the one-call path routes on (its top-k
    kernel adds the same partial sums in the same order) -- so that a layer's routing does not depend on which path its planner
    picks.  wg in x's 16-bit dtype, or fp32 over 16-bit tokens (an fp32 gate: fp32 logits).  None when the shape is not covered."""
    mixed = wg.dtype == torch.float32 and x.dtype != torch.float32
    part = gate_proj_f32w(x, wg) if mixed else gate_proj(x, wg)
    if part is None:
        return None
    return gate_topk_partials(part, wg.dtype, 1, want_logits=True)[3]


def cache_warm(t, chunk_bytes=None, n_chunks=1, stride_bytes=0, blocks=0, offset=0):
    """plain loads over n_chunks ranges of chunk_bytes (stride_bytes apart) of tensor t, from byte `offset` (memory-side cache
    warm-up on the current stream, csrc/gate_proj.hip)"""
    _dev(t)
    total = t.numel() * t.element_size()
    chunk_bytes = total - offset if chunk_bytes is None else int(chunk_bytes)
    assert offset + (n_chunks - 1) * stride_bytes + chunk_bytes <= total
    _lib.check(_lib.lib().tutel_amd_cache_warm(t.data_ptr() + offset, chunk_bytes, int(n_chunks), int(stride_bytes), int(blocks), None, _stream()),
               "tutel_amd_cache_warm")


def compute_location(idx, E, ws=None, capacity=0, want_l_aux=False, l_aux_dtype=torch.float32, cleared_slot_map=None):
    """idx [k,T] -> loc [k,T], dispatch_count [E], stats [1] (max count), l_aux [1]|None, slot_map|None.
    cleared_slot_map: an [E*capacity] int32 tensor already filled with -1 (see gate_topk(clear=...))."""
    _dev(idx)
    assert idx.dtype == torch.int32 and idx.dim() == 2 and idx.is_contiguous()
    k, T = idx.shape
    dev = idx.device
    hist_ready = ws is not None
    if ws is None:
        ws = routing_workspace(T, E, k, dev)
    loc = torch.empty_like(idx)
    cnt = torch.empty([E], dtype=torch.int32, device=dev)
    stats = torch.empty([1], dtype=torch.int32, device=dev)
    l_aux = torch.empty([1], dtype=l_aux_dtype, device=dev) if (want_l_aux and hist_ready) else None
    smap = None
    if capacity > 0:
        if cleared_slot_map is not None:
            assert cleared_slot_map.numel() == E * capacity and cleared_slot_map.dtype == torch.int32
            smap = cleared_slot_map
        else:
            smap = torch.empty([E * capacity], dtype=torch.int32, device=dev)
    L = _lib.lib()
    _lib.check(L.tutel_amd_compute_location(_ptr(idx), T, E, k, int(hist_ready), _ptr(ws), ws.numel(),
                                            _ptr(loc), _ptr(cnt), _ptr(stats), _ptr(l_aux),
                                            _code(l_aux) if l_aux is not None else 0,
                                            int(capacity), _ptr(smap), int(cleared_slot_map is not None), _stream()),
               "tutel_amd_compute_location")
    return loc, cnt, stats, l_aux, smap


def slot_map(idx, loc, E, capacity):
    _dev(idx, loc)
    assert idx.dtype == torch.int32 and loc.dtype == torch.int32
    assert idx.is_contiguous() and loc.is_contiguous() and idx.shape == loc.shape
    k, T = idx.shape
    smap = torch.empty([E * capacity], dtype=torch.int32, device=idx.device)
    _lib.check(_lib.lib().tutel_amd_slot_map(_ptr(idx), _ptr(loc), T, E, k, int(capacity), _ptr(smap),
                                             _stream()), "tutel_amd_slot_map")
    return smap


def cumsum_sub_one(mask):
    _dev(mask)
    m = mask.to(torch.int32).contiguous()
    out = torch.empty_like(m)
    _lib.check(_lib.lib().tutel_amd_cumsum_sub_one(_ptr(m), _ptr(out), m.shape[0], m.shape[1], _stream()),
               "tutel_amd_cumsum_sub_one")
    return out


# ---------------------------------------------------------------------------------------------
# dispatch / combine
# ---------------------------------------------------------------------------------------------
def fast_encode(x, smap, gates, n_slots, capacity=0, num_experts=0, chunk_rows=0, expert_slice=0, ep_world=1):
    """x [T,M] -> [n_slots, M]; gates [k,T] or None (is_postscore).  smap is always in plain bucket order;
    chunk_rows / expert_slice select the order of the OUTPUT rows (see fast_decode)."""
    _dev(x, smap, gates)
    assert x.dim() == 2 and x.is_contiguous() and smap.dtype == torch.int32 and smap.numel() == n_slots
    x = _a16(x)
    T, M = x.shape
    out = torch.empty([n_slots, M], dtype=x.dtype, device=x.device)
    if gates is not None:
        assert gates.is_contiguous()
    _lib.check(_lib.lib().tutel_amd_fast_encode(_ptr(x), _code(x), _ptr(smap), _ptr(gates),
                                                _code(gates) if gates is not None else 0, T, M,
                                                int(n_slots), int(capacity), int(num_experts), int(chunk_rows),
                                                int(expert_slice), int(ep_world), _ptr(out), _stream()),
               "tutel_amd_fast_encode")
    return out


def fast_decode(buf, idx, loc, gates, capacity, num_experts=0, chunk_rows=0, expert_slice=0, ep_world=1):
    """buf [E*C, M] -> [T, M]; gates [k,T] or None (= ones).
    chunk_rows > 0: buf is chunk-major [C/chunk_rows, E, chunk_rows, M]; expert_slice = s > 0: buf is
    expert-sliced [E_loc/s, W, s, C, M] (the two layouts of the overlapped all-to-all)."""
    _dev(buf, idx, loc, gates)
    assert buf.dim() == 2 and buf.is_contiguous()
    buf = _a16(buf)
    assert idx.dtype == torch.int32 and loc.dtype == torch.int32 and idx.is_contiguous() and loc.is_contiguous()
    k, T = idx.shape
    M = buf.shape[1]
    out = torch.empty([T, M], dtype=buf.dtype, device=buf.device)
    if gates is not None:
        assert gates.is_contiguous() and gates.shape == idx.shape
    _lib.check(_lib.lib().tutel_amd_fast_decode(_ptr(buf), _code(buf), _ptr(idx), _ptr(loc), _ptr(gates),
                                                _code(gates) if gates is not None else 0, T, M, k,
                                                int(capacity), int(num_experts), int(chunk_rows), int(expert_slice), int(ep_world),
                                                _ptr(out), _stream()),
               "tutel_amd_fast_decode")
    return out


def gate_grad(x, buf, idx, loc, capacity):
    """ggate [k,T] fp32 = <buf[slot(j,t)], x[t]>."""
    _dev(x, buf, idx, loc)
    assert x.is_contiguous() and buf.is_contiguous() and x.dtype == buf.dtype
    x, buf = _a16(x), _a16(buf)
    k, T = idx.shape
    M = x.shape[1]
    out = torch.empty([k, T], dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tutel_amd_gate_grad(_ptr(x), _ptr(buf), _code(x), _ptr(idx), _ptr(loc), T, M, k,
                                              int(capacity), _ptr(out), _stream()), "tutel_amd_gate_grad")
    return out


# ---------------------------------------------------------------------------------------------
# expert grouped GEMM
# ---------------------------------------------------------------------------------------------
def gemm_supported(dtype, N, K):
    return dtype in (torch.bfloat16, torch.float16) and K % 64 == 0 and N % 8 == 0


def expert_gemm(a, w, bias, w_kmajor, act="none", E_loc=None, R=None, a_layout=None, out=None,
                d_layout=None, row_counts=None, row_align=1, mul=None):
    """D[e,r,:] = act(A[e,r,:] @ op(W[e]) + bias[e]) [* mul[e,r,:]].

    a: [E_loc, R, K] contiguous, or any buffer described by a_layout=(stride_e, stride_w, rows_per_w, lda)
    w: [E_loc, N, K] (w_kmajor) or [E_loc, K, N]; bias [E_loc, N] or None.
    out/d_layout likewise (default: new contiguous [E_loc, R, N]); mul (GLU gating operand) has
    the output's layout and dtype."""
    _dev(a, w, bias, out, row_counts, mul)
    assert w.dim() == 3 and w.is_contiguous()
    if w_kmajor:
        El, N, K = w.shape
    else:
        El, K, N = w.shape
    E_loc = El if E_loc is None else E_loc
    if a_layout is None:
        assert a.dim() == 3 and a.is_contiguous() and a.shape[0] == E_loc and a.shape[2] == K
        a = _a16(a)
        R = a.shape[1]
        a_layout = (R * K, 0, R, K)
    assert R is not None
    default_out = out is None
    if default_out:
        out = torch.empty([E_loc, R, N], dtype=a.dtype, device=a.device)
        d_layout = (R * N, 0, R, N)
    assert d_layout is not None
    if bias is not None:
        assert bias.is_contiguous() and bias.shape[-1] == N and bias.dtype == a.dtype
    assert w.dtype == a.dtype
    if mul is not None:
        assert mul.dtype == a.dtype
        if default_out:
            assert mul.is_contiguous() and mul.numel() == E_loc * R * N
        else:
            # the kernel addresses G through d_layout exactly as it addresses `out` (G may be `out` itself): same extent, same strides
            assert mul.shape == out.shape and mul.stride() == out.stride(), "mul must have the layout of out"
        _lib.check(_lib.lib().tutel_amd_expert_gemm_glu(
            _ptr(a), a_layout[0], a_layout[1], a_layout[2], a_layout[3],
            _ptr(w), int(bool(w_kmajor)), w.stride(0), w.stride(1),
            _ptr(bias), (bias.stride(0) if bias is not None else 0), _ptr(mul),
            _ptr(out), d_layout[0], d_layout[1], d_layout[2], d_layout[3],
            E_loc, R, N, K, _code(a), ACT_CODES[act],
            _ptr(row_counts), int(row_align), _stream()), "tutel_amd_expert_gemm_glu")
        return out
    _lib.check(_lib.lib().tutel_amd_expert_gemm(
        _ptr(a), a_layout[0], a_layout[1], a_layout[2], a_layout[3],
        _ptr(w), int(bool(w_kmajor)), w.stride(0), w.stride(1),
        _ptr(bias), (bias.stride(0) if bias is not None else 0),
        _ptr(out), d_layout[0], d_layout[1], d_layout[2], d_layout[3],
        E_loc, R, N, K, _code(a), ACT_CODES[act],
        _ptr(row_counts), int(row_align), _stream()), "tutel_amd_expert_gemm")
    return out


def expert_gemm_gate_up(a, w_gate, w_up, act="silu", row_counts=None, row_align=1):
    """SwiGLU gate and up products in ONE launch: D[e,r,:] = act(A[e,r,:] @ Wg[e]^T) * (A[e,r,:] @ Wu[e]^T), the activation rounded
    to the dtype before the product and the result rounded once -- the bits of expert_gemm(a, w_gate, None, True, act=act) followed by
    expert_gemm(a, w_up, None, True, mul=<that>).  a [E, R, K]; w_gate, w_up k-major [E, N, K] -> [E, R, N].  Rows past
    ceil(row_counts[e] / row_align) * row_align are left unwritten, as there.  act: relu, gelu or silu."""
    _dev(a, w_gate, w_up, row_counts)
    assert a.dim() == 3 and a.is_contiguous() and w_gate.dim() == 3 and w_gate.is_contiguous()
    assert w_up.shape == w_gate.shape and w_up.is_contiguous() and w_gate.dtype == a.dtype and w_up.dtype == a.dtype
    E, N, K = w_gate.shape
    assert a.shape[0] == E and a.shape[2] == K
    a = _a16(a)
    R = a.shape[1]
    out = torch.empty([E, R, N], dtype=a.dtype, device=a.device)
    _lib.check(_lib.lib().tutel_amd_expert_gemm_gate_up(
        _ptr(a), R * K, 0, R, K, _ptr(w_gate), _ptr(w_up), w_gate.stride(0), w_gate.stride(1),
        _ptr(out), R * N, 0, R, N, E, R, N, K, _code(a), ACT_CODES[act],
        _ptr(row_counts), int(row_align), _stream()), "tutel_amd_expert_gemm_gate_up")
    return out


_zero_rows = {}


def zero_row(n, dtype, device):
    """the process's cached zero row of (device, dtype), at least n elements: what a gathering GEMM reads for a slot without a token.
    Allocated max(n, 8192) long and replaced by a longer one when too short (earlier holders keep theirs alive).  Not for a tensor
    made inside a captured training step: a process-wide cache must not hold memory of a graph's pool (impls/packed_train.py)."""
    z = _zero_rows.get((device, dtype))
    if z is None or z.numel() < n:
        z = _zero_rows[(device, dtype)] = torch.zeros([max(n, 8192)], dtype=dtype, device=device)
    return z


def expert_gemm_gather(x, smap, w, bias, w_kmajor, act, R, row_counts=None, row_align=1):
    """fc1 with fast_encode fused: D[e,r,:] = act(x[smap[e*R+r] % T] @ op(W[e]) + bias[e]), zero row where smap < 0."""
    _dev(x, smap, w, bias, row_counts)
    assert x.dim() == 2 and x.is_contiguous() and w.dim() == 3 and w.is_contiguous() and w.dtype == x.dtype
    E_loc, N, K = (w.shape if w_kmajor else (w.shape[0], w.shape[2], w.shape[1]))
    assert x.shape[1] == K and smap.dtype == torch.int32 and smap.numel() == E_loc * R
    x = _a16(x)
    z = zero_row(K, x.dtype, x.device)
    out = torch.empty([E_loc, R, N], dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tutel_amd_expert_gemm_gather(
        _ptr(x), x.stride(0), _ptr(smap), x.shape[0], _ptr(z), _ptr(w), int(bool(w_kmajor)), w.stride(0), w.stride(1),
        _ptr(bias), (bias.stride(0) if bias is not None else 0), _ptr(out), R * N, N, E_loc, R, N, K, _code(x),
        ACT_CODES[act], _ptr(row_counts), int(row_align), _stream()), "tutel_amd_expert_gemm_gather")
    return out


def _a_rows(a, E_loc, K, slot_map, R, a_layout):
    """where a grouped GEMM's A rows come from -> (a at a 16-byte aligned address, R, a_layout, T, zero row): the token array [T, K]
    gathered through slot_map [E_loc * R], any buffer described by a_layout with R, or [E_loc, R, K] contiguous"""
    if slot_map is not None:
        assert a.dim() == 2 and a.is_contiguous() and a.shape[1] == K and a_layout is None and R is not None
        assert slot_map.dtype == torch.int32 and slot_map.numel() == E_loc * R
        a = _a16(a)
        return a, R, (0, 0, 1, a.stride(0)), a.shape[0], zero_row(K, a.dtype, a.device)
    if a_layout is None:
        assert a.dim() == 3 and a.is_contiguous() and a.shape[0] == E_loc and a.shape[2] == K
        a = _a16(a)
        R = a.shape[1]
        a_layout = (R * K, 0, max(R, 1), K)
    assert R is not None
    return a, R, a_layout, 0, None


def _unless_notsup(rc, what, out):
    """the end of a call that may refuse: None where the library answered ENOTSUP (nothing was enqueued), any other failure raises"""
    if rc == _lib.ENOTSUP:
        return None
    _lib.check(rc, what)
    return out


def gemm_f32_supported(N, K):
    """shapes the fp32 grouped GEMM (tutel_amd_expert_gemm_f32) takes: K % 32 == 0, N % 4 == 0 -- the library's own answer"""
    return bool(_lib.lib().tutel_amd_expert_gemm_f32_supported(int(N), int(K)))


def expert_gemm_f32(a, w, bias, w_kmajor, act="none", slot_map=None, R=None, a_layout=None, out=None, d_layout=None):
    """fp32 experts on the exact-f32 MFMA: D[e,r,n] = act(chain + bias[e,n]), chain the k-ascending fmaf chain from 0.f over
    A[e,r,:] and column n of op(W[e]) (the contract of include/tutel_amd.h: bit for bit replayable on a CPU).

    a: [E_loc, R, K] contiguous, any buffer described by a_layout=(stride_e, stride_w, rows_per_w, lda) with R, or -- with
    slot_map [E_loc * R] -- the token array [T, K] whose rows fc1 gathers (fast_encode fused; negative slots read the zero row).
    w: [E_loc, N, K] (w_kmajor) or [E_loc, K, N], as stored; bias [E_loc, N] or None, its rows may be strided (b2[:, :output_dim]).
    out / d_layout as in expert_gemm.  Returns None when the library answers ENOTSUP (nothing was enqueued)."""
    _dev(a, w, bias, out, slot_map)
    assert w.dim() == 3 and w.is_contiguous() and a.dtype == torch.float32 and w.dtype == torch.float32
    E_loc, N, K = (w.shape if w_kmajor else (w.shape[0], w.shape[2], w.shape[1]))
    a, R, a_layout, T, z = _a_rows(a, E_loc, K, slot_map, R, a_layout)
    if out is None:
        out = torch.empty([E_loc, R, N], dtype=torch.float32, device=a.device)
        d_layout = (R * N, 0, max(R, 1), N)
    assert d_layout is not None and out.dtype == torch.float32
    if bias is not None:
        assert bias.dim() == 2 and bias.shape == (E_loc, N) and bias.stride(1) == 1 and bias.dtype == torch.float32
    rc = _lib.lib().tutel_amd_expert_gemm_f32(
        _ptr(a), a_layout[0], a_layout[1], a_layout[2], a_layout[3],
        _ptr(w), int(bool(w_kmajor)), w.stride(0), w.stride(1),
        _ptr(bias), (bias.stride(0) if bias is not None else 0),
        _ptr(out), d_layout[0], d_layout[1], d_layout[2], d_layout[3],
        E_loc, R, N, K, ACT_CODES[act], _ptr(slot_map), T, _ptr(z), _stream())
    return _unless_notsup(rc, "tutel_amd_expert_gemm_f32", out)


def gemm_w8_supported(dtype, N, K):
    """shapes the W8A16 grouped GEMM (tutel_amd_expert_gemm_w8) takes: bf16 / fp16 activations, K % 64 == 0, N % 32 == 0 -- the
    library's own answer"""
    if dtype not in _DT:
        return False
    return bool(_lib.lib().tutel_amd_expert_gemm_w8_supported(_DT[dtype], int(N), int(K)))


def expert_gemm_w8(a, image, scale, bias, N, K, act="none", slot_map=None, R=None, out=None, row_counts=None):
    """W8A16: D[e,r,n] = act(acc * scale[e,n] + bias[e,n]) rounded once to a.dtype, acc the fp32 sum over k of a[e,r,k] times the exact
    value of the e4m3 code of weight (e, n, k) (the contract of include/tutel_amd.h).

    a: [E_loc, R, K] contiguous bf16 / fp16, or -- with slot_map [E_loc * R] -- the token array [T, K] whose rows fc1 gathers (negative
    slots read the zero row).  image: experts/w8.py::pack's uint8 image of the [E_loc, N, K] codes; scale [E_loc, N] fp32; bias [E_loc, N]
    in a.dtype or None, its rows may be strided.  Returns None when the library answers ENOTSUP (nothing was enqueued)."""
    _dev(a, image, scale, bias, out, slot_map, row_counts)
    assert image.dtype == torch.uint8 and image.is_contiguous() and scale.dtype == torch.float32 and scale.is_contiguous()
    E_loc = image.shape[0]
    assert scale.shape == (E_loc, N) and image.numel() % max(E_loc, 1) == 0
    a, R, a_layout, T, z = _a_rows(a, E_loc, K, slot_map, R, None)
    if out is None:
        out = torch.empty([E_loc, R, N], dtype=a.dtype, device=a.device)
    assert out.dtype == a.dtype and out.is_contiguous() and out.shape == (E_loc, R, N)
    if bias is not None:
        assert bias.dim() == 2 and bias.shape == (E_loc, N) and bias.stride(1) == 1 and bias.dtype == a.dtype
    rc = _lib.lib().tutel_amd_expert_gemm_w8(
        _ptr(a), a_layout[0], a_layout[1], a_layout[2], a_layout[3],
        _ptr(image), image.numel() // max(E_loc, 1), _ptr(scale),
        _ptr(bias), (bias.stride(0) if bias is not None else 0),
        _ptr(out), R * N, 0, max(R, 1), N,
        E_loc, R, N, K, _DT.get(a.dtype, -1), ACT_CODES[act], _ptr(row_counts), _ptr(slot_map), T, _ptr(z), _stream())
    return _unless_notsup(rc, "tutel_amd_expert_gemm_w8", out)


def gemm_w8_glu_supported(dtype, H, K):
    """shapes the W8A16 gate / up GEMM (tutel_amd_expert_gemm_w8_glu) takes: bf16 / fp16 activations, K % 64 == 0, H % 16 == 0 -- the
    library's own answer"""
    if dtype not in _DT:
        return False
    return bool(_lib.lib().tutel_amd_expert_gemm_w8_glu_supported(_DT[dtype], int(H), int(K)))


def expert_gemm_w8_glu(a, image, scale, H, K, act="silu", slot_map=None, R=None, out=None, row_counts=None):
    """W8A16 gate and up products of a SwiGLU expert in ONE launch: D[e,r,n] = round(round(act(gacc * scale_gate[e,n])) * (uacc *
    scale_up[e,n])), gacc / uacc the fp32 sums over k of a[e,r,k] times the exact values of the gate / up e4m3 codes (the contract of
    include/tutel_amd.h; expert_gemm_gate_up over FP8 weights).

    a: [E_loc, R, K] contiguous bf16 / fp16, or -- with slot_map [E_loc * R] -- the token array [T, K] whose rows are gathered.  image,
    scale: experts/w8.py::prepare_gate_up's uint8 image of the interleaved [E_loc, 2 H, K] codes and its [E_loc, 2 H] fp32 scales.
    -> [E_loc, R, H].  Returns None when the library answers ENOTSUP (nothing was enqueued)."""
    _dev(a, image, scale, out, slot_map, row_counts)
    assert image.dtype == torch.uint8 and image.is_contiguous() and scale.dtype == torch.float32 and scale.is_contiguous()
    E_loc = image.shape[0]
    assert scale.shape == (E_loc, 2 * H) and image.numel() % max(E_loc, 1) == 0
    a, R, a_layout, T, z = _a_rows(a, E_loc, K, slot_map, R, None)
    if out is None:
        out = torch.empty([E_loc, R, H], dtype=a.dtype, device=a.device)
    assert out.dtype == a.dtype and out.is_contiguous() and out.shape == (E_loc, R, H)
    rc = _lib.lib().tutel_amd_expert_gemm_w8_glu(
        _ptr(a), a_layout[0], a_layout[1], a_layout[2], a_layout[3],
        _ptr(image), image.numel() // max(E_loc, 1), _ptr(scale),
        _ptr(out), R * H, 0, max(R, 1), H,
        E_loc, R, H, K, _DT.get(a.dtype, -1), ACT_CODES[act], _ptr(row_counts), _ptr(slot_map), T, _ptr(z), _stream())
    return _unless_notsup(rc, "tutel_amd_expert_gemm_w8_glu", out)


def gemm_w4_supported(dtype, N, K):
    """shapes the W4A16 grouped GEMM (tutel_amd_expert_gemm_w4) takes: bf16 / fp16 activations, K % 64 == 0, N % 32 == 0 -- the
    library's own answer"""
    if dtype not in _DT:
        return False
    return bool(_lib.lib().tutel_amd_expert_gemm_w4_supported(_DT[dtype], int(N), int(K)))


def _w4_image(codes, scales):
    """the checks the two W4A16 wrappers share -> (E_loc, an expert's code bytes, an expert's scale bytes)"""
    assert codes.dtype == torch.uint8 and codes.is_contiguous() and scales.dtype == torch.uint8 and scales.is_contiguous()
    E_loc = codes.shape[0]
    assert scales.shape[0] == E_loc and codes.numel() % max(E_loc, 1) == 0 and scales.numel() % max(E_loc, 1) == 0
    return E_loc, codes.numel() // max(E_loc, 1), scales.numel() // max(E_loc, 1)


def expert_gemm_w4(a, codes, scales, bias, N, K, act="none", slot_map=None, R=None, out=None, row_counts=None):
    """W4A16: D[e,r,n] = act(acc + bias[e,n]) rounded once to a.dtype, acc the fp32 sum over k of a[e,r,k] times the exact value of the
    MXFP4 weight (e, n, k) -- its e2m1 code times its block's power-of-two scale (the contract of include/tutel_amd.h).

    a: [E_loc, R, K] contiguous bf16 / fp16, or -- with slot_map [E_loc * R] -- the token array [T, K] whose rows fc1 gathers (negative
    slots read the zero row).  codes, scales: experts/w4.py::pack's uint8 images of the [E_loc, N, K] weights; bias [E_loc, N] in
    a.dtype or None, its rows may be strided.  Returns None when the library answers ENOTSUP (nothing was enqueued)."""
    _dev(a, codes, scales, bias, out, slot_map, row_counts)
    E_loc, wb, sb = _w4_image(codes, scales)
    a, R, a_layout, T, z = _a_rows(a, E_loc, K, slot_map, R, None)
    if out is None:
        out = torch.empty([E_loc, R, N], dtype=a.dtype, device=a.device)
    assert out.dtype == a.dtype and out.is_contiguous() and out.shape == (E_loc, R, N)
    if bias is not None:
        assert bias.dim() == 2 and bias.shape == (E_loc, N) and bias.stride(1) == 1 and bias.dtype == a.dtype
    rc = _lib.lib().tutel_amd_expert_gemm_w4(
        _ptr(a), a_layout[0], a_layout[1], a_layout[2], a_layout[3],
        _ptr(codes), wb, _ptr(scales), sb,
        _ptr(bias), (bias.stride(0) if bias is not None else 0),
        _ptr(out), R * N, 0, max(R, 1), N,
        E_loc, R, N, K, _DT.get(a.dtype, -1), ACT_CODES[act], _ptr(row_counts), _ptr(slot_map), T, _ptr(z), _stream())
    return _unless_notsup(rc, "tutel_amd_expert_gemm_w4", out)


def gemm_w4_glu_supported(dtype, H, K):
    """shapes the W4A16 gate / up GEMM (tutel_amd_expert_gemm_w4_glu) takes: bf16 / fp16 activations, K % 64 == 0, H % 16 == 0 -- the
    library's own answer"""
    if dtype not in _DT:
        return False
    return bool(_lib.lib().tutel_amd_expert_gemm_w4_glu_supported(_DT[dtype], int(H), int(K)))


def expert_gemm_w4_glu(a, codes, scales, H, K, act="silu", slot_map=None, R=None, out=None, row_counts=None):
    """W4A16 gate and up products of a SwiGLU expert in ONE launch: D[e,r,n] = round(float(round(act(gacc))) * uacc), gacc / uacc the
    fp32 sums over k of a[e,r,k] times the exact values of the gate / up MXFP4 weights (the contract of include/tutel_amd.h).

    a: [E_loc, R, K] contiguous bf16 / fp16, or -- with slot_map [E_loc * R] -- the token array [T, K] whose rows are gathered.  codes,
    scales: experts/w4.py::prepare_gate_up's uint8 images of the interleaved [E_loc, 2 H, K] weights.  -> [E_loc, R, H].  Returns None
    when the library answers ENOTSUP (nothing was enqueued)."""
    _dev(a, codes, scales, out, slot_map, row_counts)
    E_loc, wb, sb = _w4_image(codes, scales)
    a, R, a_layout, T, z = _a_rows(a, E_loc, K, slot_map, R, None)
    if out is None:
        out = torch.empty([E_loc, R, H], dtype=a.dtype, device=a.device)
    assert out.dtype == a.dtype and out.is_contiguous() and out.shape == (E_loc, R, H)
    rc = _lib.lib().tutel_amd_expert_gemm_w4_glu(
        _ptr(a), a_layout[0], a_layout[1], a_layout[2], a_layout[3],
        _ptr(codes), wb, _ptr(scales), sb,
        _ptr(out), R * H, 0, max(R, 1), H,
        E_loc, R, H, K, _DT.get(a.dtype, -1), ACT_CODES[act], _ptr(row_counts), _ptr(slot_map), T, _ptr(z), _stream())
    return _unless_notsup(rc, "tutel_amd_expert_gemm_w4_glu", out)


INT32_MAX = 2 ** 31 - 1


def quantize_w8_supported(dtype, N, K, channel_map=None):
    """shapes the HIP quantiser (tutel_amd_quantize_w8) takes -- the library's own answer.  channel_map: (image_channels, group,
    group_stride, group_offset), default the plain map (N, N, N, 0)"""
    if dtype not in _DT:
        return False
    C, g, gs, go = (N, N, N, 0) if channel_map is None else channel_map
    return bool(_lib.lib().tutel_amd_quantize_w8_supported(_DT[dtype], int(N), int(K), int(C), int(g), int(gs), int(go)))


def quantize_w8(w, w_kmajor, image=None, scale=None, channel_map=None, check_only=False):
    """The FP8 weight image and scales of one parameter, written by the HIP quantiser straight from the parameter as stored: bit for
    bit experts/w8.py::prepare (the contract of include/tutel_amd.h).

    w: [E, N, K] (w_kmajor) or [E, K, N], bf16 / fp16 / fp32; the last dimension contiguous, rows and experts may be strided.
    channel_map = (image_channels, group, group_stride, group_offset): source channel n goes to image channel
    (n / group) * group_stride + group_offset + n % group; default the plain map.  A SwiGLU gate / up pair is two calls into one
    image [E, 2 H / 32, K / 32, 64, 16]: (2 H, 16, 32, 0) for the gate, (2 H, 16, 32, 16) with image= and scale= for the up.
    image / scale: written in place when given (uint8 with image_channels * K bytes per expert, fp32 [E, image_channels]), else
    allocated.  check_only: nothing is written but the finiteness check runs.
    -> (image, scale); None where the library does not cover the call (nothing was enqueued).  A non-finite weight raises the torch
    quantiser's ValueError, naming the same channel (this reads one word back: a synchronisation, the quantiser is a cold path)."""
    _dev(w, image, scale)
    assert w.dim() == 3 and w.stride(2) == 1
    E = w.shape[0]
    N, K = (w.shape[1], w.shape[2]) if w_kmajor else (w.shape[2], w.shape[1])
    C, g, gs, go = (N, N, N, 0) if channel_map is None else (int(v) for v in channel_map)
    if w.dtype not in _DT or not quantize_w8_supported(w.dtype, N, K, (C, g, gs, go)):
        return None
    if not check_only:
        if image is None:
            image = torch.empty([E, C // 32, K // 32, 64, 16], dtype=torch.uint8, device=w.device)
        if scale is None:
            scale = torch.empty([E, C], dtype=torch.float32, device=w.device)
        assert image.dtype == torch.uint8 and image.is_contiguous() and image.numel() == E * C * K
        assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.shape == (E, C)
    status = torch.full([1], INT32_MAX, dtype=torch.int32, device=w.device)
    rc = _lib.lib().tutel_amd_quantize_w8(
        _ptr(w), _DT[w.dtype], int(bool(w_kmajor)), w.stride(0) if E > 1 else max(w.stride(0), w.shape[1] * w.stride(1)), w.stride(1),
        E, N, K, None if check_only else _ptr(image), C * K, None if check_only else _ptr(scale), C, C, g, gs, go,
        _ptr(status), _stream())
    if _unless_notsup(rc, "tutel_amd_quantize_w8", True) is None:
        return None
    bad = int(status.item())
    if bad != INT32_MAX:
        raise ValueError(f"quantize_e4m3: channel (expert {bad // N}, output {bad % N}) holds a non-finite weight")
    return image, scale


def expert_ffn(x, w1, b1, w2_kmajor, b2, act, R=None, smap=None, hid=None):
    """fc1 -> activation -> fc2 of every local expert in ONE persistent launch (tutel_amd_expert_ffn, csrc/expert_ffn.hip):
    x [E_loc, R, M] -- or the token array [T, M] with smap [E_loc * R] (fast_encode fused) -- w1 [E_loc, H, M], w2_kmajor
    [E_loc, M_out, H] (the k-major copy of batched_fc2_w) -> [E_loc, R, M_out].  Returns None when the library answers ENOTSUP
    (shape / layout not covered, or TUTEL_OPT_FFN_FUSED at its default: the persistent launch is opt-in, the two launches measured
    faster): the caller then runs two expert_gemm launches -- same bits."""
    _dev(x, w1, b1, w2_kmajor, b2, smap)
    assert w1.dim() == 3 and w2_kmajor.dim() == 3 and w1.is_contiguous() and w2_kmajor.is_contiguous() and w1.dtype == x.dtype == w2_kmajor.dtype
    E_loc, H, M = w1.shape
    M_out = w2_kmajor.shape[1]
    assert w2_kmajor.shape == (E_loc, M_out, H)
    x, R, (xs, _, _, ldx), T, z = _a_rows(x, E_loc, M, smap, R, None)
    if hid is None:
        hid = torch.empty([E_loc, R, H], dtype=x.dtype, device=x.device)
    out = torch.empty([E_loc, R, M_out], dtype=x.dtype, device=x.device)
    rc = _lib.lib().tutel_amd_expert_ffn(_ptr(x), xs, ldx, _ptr(smap), T, _ptr(z), _ptr(w1), w1.stride(0), w1.stride(1), _ptr(b1),
                                         (b1.stride(0) if b1 is not None else 0), _ptr(hid), R * H, H, _ptr(w2_kmajor), w2_kmajor.stride(0),
                                         w2_kmajor.stride(1), _ptr(b2), (b2.stride(0) if b2 is not None else 0), _ptr(out), R * M_out, M_out,
                                         E_loc, R, M, H, M_out, _code(x), ACT_CODES[act], _stream())
    return _unless_notsup(rc, "tutel_amd_expert_ffn", out)


_OPT_ENV = {_lib.OPT_GEMM_IMPL: "TUTEL_AMD_GEMM_IMPL", _lib.OPT_GEMM_TILE: "TUTEL_AMD_GEMM_BIG", _lib.OPT_DECODE: "TUTEL_AMD_DECODE",
            _lib.OPT_EP_STAGE_GRID: "TUTEL_AMD_EP_STAGE_GRID", _lib.OPT_GEMM_PERSIST: "TUTEL_AMD_GEMM_PERSIST", _lib.OPT_EP_STREAMS: "TUTEL_AMD_EP_STREAMS",
            _lib.OPT_EP_CANARY: "TUTEL_AMD_EP_CANARY", _lib.OPT_GEMM_SPLITK: "TUTEL_AMD_GEMM_SPLITK", _lib.OPT_GEMM_STORE: "TUTEL_AMD_GEMM_STORE",
            _lib.OPT_GEMM_GATHER: "TUTEL_AMD_GEMM_GATHER", _lib.OPT_FUSED_LOCATION: "TUTEL_AMD_FUSED_LOCATION", _lib.OPT_TIE_RULE: "TUTEL_AMD_TIE_RULE", _lib.OPT_FFN_FUSED: "TUTEL_AMD_FFN_FUSED"}
_opts = {}


# ---------------------------------------------------------------------------------------------
# packed dropless layout: the launches of a training step (include/tutel_amd.h, "training on the packed layout")
# ---------------------------------------------------------------------------------------------
class PackedLayout:
    """Device tables of one packed layout (tutel_amd_packed_layout), sized by the host bounds: offsets [E + 1], tiles [2 * tiles_bound],
    ntiles [1], capacity [1] (max rows of an expert), slot_map [rows_bound]; row_limit = L (0: none)."""

    def __init__(self, E, rows_bound, tiles_bound, row_limit, device):
        self.E, self.rows_bound, self.tiles_bound, self.row_limit = int(E), int(rows_bound), int(tiles_bound), int(row_limit)
        self.offsets = torch.empty([E + 1], dtype=torch.int32, device=device)
        self.tiles = torch.empty([2 * max(tiles_bound, 1)], dtype=torch.int32, device=device)
        self.ntiles = torch.empty([1], dtype=torch.int32, device=device)
        self.capacity = torch.empty([1], dtype=torch.int32, device=device)
        self.slot_map = torch.empty([max(rows_bound, 1)], dtype=torch.int32, device=device)

    @property
    def decode_limit(self):
        """the row limit the packed decode / gate gradient take (none: INT_MAX)"""
        return self.row_limit if self.row_limit > 0 else 0x7fffffff


def packed_layout(dispatch_count, idx, loc, capacity_limit, alignment, rows_bound, tiles_bound, row_limit, out=None):
    """tutel_amd_packed_layout: dispatch_count [E], idx / loc [k, T] int32 -> PackedLayout (written into `out` when given)."""
    _dev(dispatch_count, idx, loc)
    k, T = idx.shape
    E = dispatch_count.numel()
    lay = out if out is not None else PackedLayout(E, rows_bound, tiles_bound, row_limit, idx.device)
    _lib.check(_lib.lib().tutel_amd_packed_layout(_ptr(dispatch_count), _ptr(idx), _ptr(loc), T, E, k, int(capacity_limit), int(alignment),
                                                  lay.rows_bound, lay.tiles_bound, _ptr(lay.offsets), _ptr(lay.tiles), _ptr(lay.ntiles),
                                                  _ptr(lay.capacity), _ptr(lay.slot_map), _stream()), "tutel_amd_packed_layout")
    return lay


def expert_gemm_packed(a, w, bias, w_kmajor, layout, act="none", gather=None, zero_row=None, mul=None, out=None):
    """Packed rows: D[r] = act(A[r] @ op(W[e]) + bias[e]) [* mul[r]] for the rows r of expert e -> [rows_bound, N].
    a [rows_bound, K], or with gather=True the token array [T, K] read through layout.slot_map (zero_row for pad rows);
    w [E, N, K] (w_kmajor) or [E, K, N] as stored; N any multiple of 8.  Rows past layout.offsets[E] are left unwritten
    (out: a contiguous [rows_bound, N] tensor to write into instead of a fresh one)."""
    _dev(a, w, bias, mul)
    assert a.dim() == 2 and a.is_contiguous() and w.dim() == 3 and w.is_contiguous() and w.dtype == a.dtype
    E, N, K = (w.shape[0], w.shape[1], w.shape[2]) if w_kmajor else (w.shape[0], w.shape[2], w.shape[1])
    assert a.shape[1] == K and E == layout.E
    if bias is not None:
        assert bias.is_contiguous() and bias.shape[-1] == N and bias.dtype == a.dtype
    if mul is not None:
        assert mul.shape == (layout.rows_bound, N) and mul.is_contiguous() and mul.dtype == a.dtype
    a = _a16(a)
    if out is None:
        out = torch.empty([layout.rows_bound, N], dtype=a.dtype, device=a.device)
    else:
        _dev(out)
        assert out.shape == (layout.rows_bound, N) and out.is_contiguous() and out.dtype == a.dtype
    _lib.check(_lib.lib().tutel_amd_expert_gemm_packed(
        _ptr(a), K, _ptr(layout.slot_map) if gather else None, a.shape[0] if gather else 0, _ptr(zero_row) if gather else None,
        _ptr(w), int(bool(w_kmajor)), w.stride(0), w.stride(1), _ptr(bias), (bias.stride(0) if bias is not None else 0), _ptr(mul),
        _ptr(out), N, E, layout.rows_bound, N, K, _code(a), ACT_CODES[act], _ptr(layout.offsets), _ptr(layout.tiles), _ptr(layout.ntiles),
        _ptr(layout.capacity), layout.tiles_bound, _stream()), "tutel_amd_expert_gemm_packed")
    return out


def _w8_packed_operands(a, image, scale, channels, N, K, layout, gather, zero_row, out):
    """the operand checks the two packed W8A16 wrappers share -> (a at a 16-byte aligned address, out [rows_bound, N], a_rows, T, zero row)"""
    _dev(a, image, scale, out, zero_row)
    assert image.dtype == torch.uint8 and image.is_contiguous() and scale.dtype == torch.float32 and scale.is_contiguous()
    E = image.shape[0]
    assert E == layout.E and scale.shape == (E, channels) and image.numel() % max(E, 1) == 0
    assert a.dim() == 2 and a.is_contiguous() and a.shape[1] == K
    a = _a16(a)
    if gather:
        assert zero_row is not None and zero_row.dtype == a.dtype and zero_row.numel() >= K
    else:
        assert a.shape[0] >= layout.rows_bound
    if out is None:
        out = torch.empty([layout.rows_bound, N], dtype=a.dtype, device=a.device)
    assert out.shape == (layout.rows_bound, N) and out.is_contiguous() and out.dtype == a.dtype
    return a, out, (_ptr(layout.slot_map) if gather else None), (a.shape[0] if gather else 0), (_ptr(zero_row) if gather else None)


def expert_gemm_w8_packed(a, image, scale, bias, N, K, layout, act="none", gather=None, zero_row=None, out=None):
    """expert_gemm_w8 over the packed dropless layout: D[r] = act(acc * scale[e] + bias[e]) for the packed rows r of expert e
    -> [rows_bound, N], bit for bit what expert_gemm_w8 writes for the same row and expert (the contract of include/tutel_amd.h).
    a [rows_bound, K] bf16 / fp16, or with gather=True the token array [T, K] read through layout.slot_map (zero_row, >= K zeros,
    for pad rows); image / scale / bias as expert_gemm_w8's.  Rows past layout.offsets[E] are left unwritten.  Returns None when
    the library answers ENOTSUP (nothing was enqueued)."""
    a, out, rows, T, z = _w8_packed_operands(a, image, scale, N, N, K, layout, gather, zero_row, out)
    if bias is not None:
        _dev(bias)
        assert bias.dim() == 2 and bias.shape == (layout.E, N) and bias.stride(1) == 1 and bias.dtype == a.dtype
    rc = _lib.lib().tutel_amd_expert_gemm_w8_packed(
        _ptr(a), K, rows, T, z, _ptr(image), image.numel() // max(layout.E, 1), _ptr(scale),
        _ptr(bias), (bias.stride(0) if bias is not None else 0), _ptr(out), N, layout.E, layout.rows_bound, N, K,
        _DT.get(a.dtype, -1), ACT_CODES[act], _ptr(layout.offsets), _ptr(layout.tiles), _ptr(layout.ntiles), layout.tiles_bound, _stream())
    return _unless_notsup(rc, "tutel_amd_expert_gemm_w8_packed", out)


def expert_gemm_w8_glu_packed(a, image, scale, H, K, layout, act="silu", gather=None, zero_row=None, out=None):
    """expert_gemm_w8_glu over the packed dropless layout -> [rows_bound, H], bit for bit what expert_gemm_w8_glu writes for the same
    row and expert.  a, gather, zero_row as expert_gemm_w8_packed's; image / scale: the interleaved gate / up image and its
    [E, 2 H] scales.  Returns None when the library answers ENOTSUP (nothing was enqueued)."""
    a, out, rows, T, z = _w8_packed_operands(a, image, scale, 2 * H, H, K, layout, gather, zero_row, out)
    rc = _lib.lib().tutel_amd_expert_gemm_w8_glu_packed(
        _ptr(a), K, rows, T, z, _ptr(image), image.numel() // max(layout.E, 1), _ptr(scale),
        _ptr(out), H, layout.E, layout.rows_bound, H, K,
        _DT.get(a.dtype, -1), ACT_CODES[act], _ptr(layout.offsets), _ptr(layout.tiles), _ptr(layout.ntiles), layout.tiles_bound, _stream())
    return _unless_notsup(rc, "tutel_amd_expert_gemm_w8_glu_packed", out)


def _grad_out_dtype(out_dtype, operand_dtype):
    """out_dtype of the packed gradients: None -> the operands' dtype (the 16-bit entry points), torch.float32 -> the *_f32 ones"""
    if out_dtype is None or out_dtype == operand_dtype:
        return operand_dtype, ""
    if out_dtype == torch.float32:
        return torch.float32, "_f32"
    raise _lib.TutelAmdError(f"tutel_amd: the packed gradients come in the operands' dtype or torch.float32, not {out_dtype}")


def _grad_acc_target(acc, numel, out_dtype, device, what):
    """accumulate_into of the packed gradients: a contiguous fp32 tensor of `numel` elements on `device`, checked before any launch"""
    if out_dtype is not None and out_dtype != torch.float32:
        raise _lib.TutelAmdError(f"tutel_amd: {what}: accumulate_into is an fp32 sum, it does not go with out_dtype={out_dtype}")
    if not isinstance(acc, torch.Tensor) or acc.dtype != torch.float32:
        raise _lib.TutelAmdError(f"tutel_amd: {what}: accumulate_into must be a torch.float32 tensor, not "
                                 f"{acc.dtype if isinstance(acc, torch.Tensor) else type(acc).__name__}")
    if acc.numel() != numel:
        raise _lib.TutelAmdError(f"tutel_amd: {what}: accumulate_into has {acc.numel()} elements, the gradient {numel}")
    if not acc.is_contiguous():
        raise _lib.TutelAmdError(f"tutel_amd: {what}: accumulate_into must be contiguous")
    if acc.device != device:
        raise _lib.TutelAmdError(f"tutel_amd: {what}: accumulate_into is on {acc.device}, the operands on {device}")
    return acc


def expert_wgrad_packed(a, b, layout, gather=None, zero_row=None, out_dtype=None, accumulate_into=None):
    """Weight gradient over the packed rows: D[e] = A[rows(e)]^T @ B[rows(e)] -> [E, N_a, N_b], fp32 sums in a fixed order.
    a [rows_bound, N_a], b [rows_bound, N_b]; gather="a" or "b": that operand is the token array [T, *] read through
    layout.slot_map (zero_row, >= 8 zeros, for pad rows).  out_dtype: None (the operands' dtype, rounded once) or torch.float32
    (the same sums left unrounded: fp32 master weights under autocast).  accumulate_into: a contiguous fp32 tensor of E * N_a * N_b
    elements on the operands' device (a main_grad): D += the fp32 sums in the kernel's epilogue, in place, and D is returned; an
    expert without rows leaves its part untouched.  Not with a 16-bit out_dtype."""
    if accumulate_into is not None:
        assert a.dim() == 2 and b.dim() == 2
        _grad_acc_target(accumulate_into, layout.E * a.shape[1] * b.shape[1], out_dtype, a.device, "expert_wgrad_packed")
    _dev(a, b)
    assert a.dim() == 2 and b.dim() == 2 and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype
    assert gather in (None, "a", "b")
    dt, sfx = _grad_out_dtype(out_dtype, a.dtype) if accumulate_into is None else (torch.float32, "_acc_f32")
    a, b = _a16(a), _a16(b)
    Na, Nb = a.shape[1], b.shape[1]
    g = {None: 0, "a": 1, "b": 2}[gather]
    T = (a if gather == "a" else b).shape[0] if gather else 0
    out = torch.empty([layout.E, Na, Nb], dtype=dt, device=a.device) if accumulate_into is None else accumulate_into
    what = "tutel_amd_expert_wgrad_packed" + sfx
    _lib.check(getattr(_lib.lib(), what)(
        _ptr(a), Na, _ptr(b), Nb, _ptr(layout.slot_map) if g else None, g, T, _ptr(zero_row) if g else None,
        _ptr(out), layout.E, layout.rows_bound, Na, Nb, _code(a), _ptr(layout.offsets), _stream()), what)
    return out


def expert_bgrad_packed(b, layout, out_dtype=None, accumulate_into=None):
    """Bias gradient over the packed rows: D[e] = sum of b[rows(e)] -> [E, N] (out_dtype and accumulate_into, here E * N fp32
    elements, as expert_wgrad_packed's)."""
    if accumulate_into is not None:
        assert b.dim() == 2
        _grad_acc_target(accumulate_into, layout.E * b.shape[1], out_dtype, b.device, "expert_bgrad_packed")
    _dev(b)
    assert b.dim() == 2 and b.is_contiguous()
    dt, sfx = _grad_out_dtype(out_dtype, b.dtype) if accumulate_into is None else (torch.float32, "_acc_f32")
    out = torch.empty([layout.E, b.shape[1]], dtype=dt, device=b.device) if accumulate_into is None else accumulate_into
    what = "tutel_amd_expert_bgrad_packed" + sfx
    _lib.check(getattr(_lib.lib(), what)(_ptr(b), b.shape[1], _ptr(out), layout.E, b.shape[1], _code(b), _ptr(layout.offsets), _stream()), what)
    return out


def gate_grad_packed(x, buf, idx, loc, layout):
    """ggate [k, T] fp32 = <x[t], buf[off[e] + loc]> (0 for an entry dropped by the row limit)."""
    _dev(x, buf, idx, loc)
    assert x.is_contiguous() and buf.is_contiguous() and x.dtype == buf.dtype
    x, buf = _a16(x), _a16(buf)
    k, T = idx.shape
    out = torch.empty([k, T], dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tutel_amd_gate_grad_packed(_ptr(x), _ptr(buf), _code(x), _ptr(idx), _ptr(loc), T, x.shape[1], k, layout.decode_limit,
                                                     _ptr(layout.offsets), _ptr(out), _stream()), "tutel_amd_gate_grad_packed")
    return out


def fast_decode_packed(buf, idx, loc, gates, layout):
    """out[t] = sum_j g[j, t] * buf[off[idx] + loc] (gates None: 1) -> [T, M]."""
    _dev(buf, idx, loc, gates)
    assert buf.is_contiguous()
    buf = _a16(buf)
    k, T = idx.shape
    M = buf.shape[1]
    out = torch.empty([T, M], dtype=buf.dtype, device=buf.device)
    if gates is not None:
        assert gates.is_contiguous() and gates.shape == (k, T)
    _lib.check(_lib.lib().tutel_amd_fast_decode_packed(_ptr(buf), _code(buf), _ptr(idx), _ptr(loc), _ptr(gates),
                                                       _code(gates) if gates is not None else 0, T, M, k, layout.decode_limit,
                                                       _ptr(layout.offsets), _ptr(out), _stream()), "tutel_amd_fast_decode_packed")
    return out


def set_option(key, value):
    """Tuning knob (_lib.OPT_*): -1 automatic, 0 / 1 forced.  For A/B runs and tests."""
    _lib.check(_lib.lib().tutel_amd_set_option(int(key), int(value)), "tutel_amd_set_option")
    _opts[int(key)] = int(value)


def get_option(key):
    """the knob's current value as the host code sees it (the library seeds its own copy from the same environment variable)"""
    import os
    if int(key) in _opts:
        return _opts[int(key)]
    try:
        return int(os.environ.get(_OPT_ENV[int(key)], "-1"))
    except ValueError:
        return -1


def gemm_plain(value=-2):
    """The PLAIN form of the 128 x 256 ring GEMM kernel (include/tutel_amd.h): -1 automatic / 1 = wherever a launch admits it, 0 = never;
    -2 only asks.  Returns the previous value (seeded from TUTEL_AMD_GEMM_PLAIN)."""
    return _lib.lib().tutel_amd_gemm_plain(int(value))


def expert_gemm_last_form():
    """(_lib.GEMM_FORM_* of the last grouped GEMM this thread launched -- NONE before the first --, [launches so far in the GENERAL form,
    in the PLAIN form])"""
    n = (ctypes.c_int * 2)()
    form = _lib.lib().tutel_amd_expert_gemm_last_form(ctypes.byref(n))
    return form, [n[0], n[1]]


def probe_tr16():
    out = torch.empty([256], dtype=torch.int16, device="cuda")
    _lib.check(_lib.lib().tutel_amd_probe_tr16(_ptr(out), _stream()), "tutel_amd_probe_tr16")
    return out


def stage_timing(mode):
    """0 off; 1 HIP events around every kernel launch of the C ABI from now on; 2 around the two expert GEMMs only
    (measurement only; see include/tutel_amd.h)."""
    _lib.check(_lib.lib().tutel_amd_stage_timing(int(mode)), "tutel_amd_stage_timing")


def stage_report():
    """{stage: (total_us, launches)} of the launches recorded since the last report (waits for them)."""
    import ctypes
    n = len(_lib.STAGES)
    tot, cnt = (ctypes.c_double * n)(), (ctypes.c_int * n)()
    _lib.check(_lib.lib().tutel_amd_stage_report(tot, cnt, n), "tutel_amd_stage_report")
    return {name: (float(tot[i]), int(cnt[i])) for i, name in enumerate(_lib.STAGES)}


def mark():
    """record a step mark on the current stream (see tutel_amd_mark)"""
    _lib.check(_lib.lib().tutel_amd_mark(_stream()), "tutel_amd_mark")


def marks_reserve(n):
    _lib.check(_lib.lib().tutel_amd_marks_reserve(int(n)), "tutel_amd_marks_reserve")


def marks_report(n):
    """milliseconds between consecutive marks recorded since the last report"""
    import ctypes
    buf = (ctypes.c_double * max(n, 1))()
    m = _lib.lib().tutel_amd_marks_report(buf, int(n))
    return [buf[i] * 1e-3 for i in range(m)]
