"""What the grouped-GEMM entry points refuse before any HIP call, without a GPU: status and tutel_amd_last_error() text per case, so that
the host plumbing between the C ABI and the kernels (one problem description, one set of checks in tutel_gemm_args) can be reworked
without a refusal changing its order, its code or its words.  The same for the pipeline entry points that fill such problems themselves
(tutel_amd_ep_forward, tutel_amd_moe_forward, the packed forwards).  Pointers are aligned integers that are never dereferenced."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


P, P2, P3, P4 = 1 << 20, 2 << 20, 3 << 20, 4 << 20      # "device pointers": every call below returns before a launch
E, R, N, K = 2, 128, 128, 128
F32, BF16 = 0, 2
NONE, RELU, GELU = 0, 1, 2
ENOTSUP = 1001


def gemm(A=P, lda=K, D=P3, E_loc=E, N=N, K=K, dtype=BF16, row_counts=None, row_align=1):
    return ("tutel_amd_expert_gemm", (A, R * K, 0, R, lda, P2, 1, N * K, K, None, 0, D, R * N, 0, R, N, E_loc, R, N, K, dtype, RELU,
                                      row_counts, row_align, None))


def glu(G):
    return ("tutel_amd_expert_gemm_glu", (P, R * K, 0, R, K, P2, 1, N * K, K, None, 0, G, P3, R * N, 0, R, N, E, R, N, K, BF16, RELU, None, 1, None))


def gather(slot_map=P4, zero_row=P4):
    return ("tutel_amd_expert_gemm_gather", (P, K, slot_map, 64, zero_row, P2, 1, N * K, K, None, 0, P3, R * N, N, E, R, N, K, BF16, RELU, None, 1,
                                             None))


def gate_up(act=RELU, W_up=P4, ldd=N, R=R, lda=K):
    return ("tutel_amd_expert_gemm_gate_up", (P, 0, 0, R, lda, P2, W_up, N * K, K, P3, 0, 0, R, ldd, 1, R, N, K, BF16, act, None, 1, None))


def packed(a_rows=None, T=0, w_kmajor=1, mul=None, D=P3, K=K, dtype=BF16, act=RELU, offsets=P4):
    return ("tutel_amd_expert_gemm_packed", (P, K, a_rows, T, None, P2, w_kmajor, N * K, K, None, 0, mul, D, N, E, 512, N, K, dtype, act,
                                             offsets, P4, P4, P4, 2, None))


def ffn(M=128, dtype=BF16):
    H = 128
    return ("tutel_amd_expert_ffn", (P, R * M, M, None, 0, None, P2, H * M, M, None, 0, P3, R * H, H, P4, M * H, H, None, 0, P3 + (1 << 19), R * M,
                                     M, E, R, M, H, M, dtype, RELU, None))


# ---- the pipeline entry points (ep.hip, dropless.hip): the same kind of table over their argument structs ------------------------------
Q = [i << 20 for i in range(1, 40)]                       # distinct 1 MiB-aligned "device pointers"


def _fill(struct, fields):
    for name, value in fields.items():
        setattr(struct, name, value)
    return struct


def ep_args(**kw):
    from tutel_amd import _lib
    d = dict(T=64, M=128, H=128, M_out=128, num_experts=2, world=1, k=1, capacity=128, degree=1, allow_sliced=1, dtype=BF16, gate_dtype=BF16,
             act=RELU, is_postscore=1, w2_kmajor=1, fuse_encode=1, x=Q[0], slot_map=Q[1], idx=Q[2], loc=Q[3], gates=Q[4], w1=Q[5], w2=Q[6],
             hid=Q[7], send=Q[8], zero_row=Q[9], y=Q[10], row_align=1)
    d.update(kw)
    return _fill(_lib.EpArgs(), d)


def moe_args(ep=None, **kw):
    from tutel_amd import _lib
    d = dict(ep=ep_args(**(ep or {})), logits=Q[12], logits_dtype=BF16, normalize_gate=1, ws=Q[13], ws_bytes=1 << 20, dispatch_count=Q[14],
             stats=Q[15], l_aux=Q[16], capacity_limit=0, alignment=1, max_capacity=128)
    d.update(kw)
    return _fill(_lib.MoeArgs(), d)


def ep(**kw):
    return ("tutel_amd_ep_forward", (None, ctypes.byref(ep_args(**kw)), None))


def moe(ep=None, **kw):
    return ("tutel_amd_moe_forward", (None, ctypes.byref(moe_args(ep, **kw)), None))


PROJECT = dict(logits=None, gate_w=Q[17])                  # the gate projection inside the call
BIG = dict(T=256, M=2048, num_experts=64)                 # a shape the in-call projection covers (16 splits)
FL = dict(fl_ws=Q[18], fl_ws_bytes=1 << 16)               # what makes tutel_amd_moe_forward take the fused-location route


def packed_fwd(ep=None, pk=None, w_up=False, **kw):
    from tutel_amd import _lib
    m = moe_args(dict(dict(capacity=0), **(ep or {})), **kw)
    p = _fill(_lib.PackedArgs(), dict(dict(ws=Q[20], ws_bytes=1 << 30, offsets=Q[30], capacity=Q[31]), **(pk or {})))
    if w_up is False:
        return ("tutel_amd_moe_forward_packed", (None, ctypes.byref(m), ctypes.byref(p), None))
    return ("tutel_amd_moe_forward_packed_glu", (None, ctypes.byref(m), ctypes.byref(p), w_up, None))


PIPELINE_CASES = [
    (("tutel_amd_ep_forward", (None, None, None)), -1, "tutel_amd_ep_forward: null arguments"),
    (ep(k=0), -1, "tutel_amd_ep_forward: bad sizes"),
    (ep(world=2), -1, "tutel_amd_ep_forward: communicator world size does not match (2)"),
    (ep(dtype=F32), -1, "tutel_amd_ep_forward: bf16 / fp16 experts only (got dtype 0)"),
    (ep(w1=None), -1, "tutel_amd_ep_forward: null pointer"),
    (ep(gates=None), -1, "tutel_amd_ep_forward: null gates"),
    (ep(row_counts=Q[11], degree=2), -1, "tutel_amd_ep_forward: row counts (megablocks) need a single rank"),
    (ep(hid=None), -1, "tutel_amd_ep_forward: null workspace"),
    (ep(fuse_encode=0), -1, "tutel_amd_ep_forward: null workspace"),                            # the staged route's buffers
    (ep(M=96), -1, "tutel_amd_expert_gemm: K=96 must be a multiple of 64"),                     # fc1's own check, through the expert stage
    (("tutel_amd_moe_forward", (None, None, None)), -1, "tutel_amd_moe_forward: null arguments"),
    (moe(ws=None), -1, "tutel_amd_moe_forward: null pointer"),
    (moe(logits_dtype=1, **PROJECT), -1, "tutel_amd_moe_forward: the in-call gate projection needs the gate in the token dtype (1 vs 2)"),
    (moe(BIG, **PROJECT), -1, "tutel_amd_moe_forward: gate_partials must hold 16 x 256 x 64 floats"),
    (moe(dict(idx=None)), -1, "tutel_amd_moe_forward: null routing buffers"),
    (moe(dict(capacity=0), stats=None), -1, "tutel_amd_moe_forward: dropless routing needs a single rank, stats, capacity_out and max_capacity"),
    (moe(dict(k=3), **FL), -1, "tutel_amd_moe_forward: need 1 <= k <= E (got k=3, E=2)"),
    (moe(ws_bytes=4, **FL), -1, "tutel_amd_moe_forward: routing workspace too small (4 bytes, need 16)"),
    (("tutel_amd_moe_forward_packed", (None, None, None, None)), -1, "tutel_amd_moe_forward_packed: null arguments"),
    (packed_fwd(dict(world=2)), -1, "tutel_amd_moe_forward_packed: single rank only (comm must be NULL, world 1)"),
    (packed_fwd(dict(M=96)), ENOTSUP, "tutel_amd_packed_plan: not covered: M and H must be multiples of 64"),
    (packed_fwd(dict(is_postscore=0)), ENOTSUP,
     "tutel_amd_moe_forward_packed: not covered: needs is_postscore (gates in the decode) and k-major fc2 weights"),
    (packed_fwd(pk=dict(offsets=None)), -1, "tutel_amd_moe_forward_packed: null pointer"),
    (packed_fwd(pk=dict(ws_bytes=16)), -1, "tutel_amd_moe_forward_packed: packed workspace too small or misaligned (16 bytes, need 33536)"),
    (packed_fwd(logits=None), -1, "tutel_amd_moe_forward_packed: null logits"),
    (packed_fwd(dict(zero_row=None)), -1, "tutel_amd_moe_forward_packed: null pointer"),
    (packed_fwd(logits_dtype=3), -1, "tutel_amd_moe_forward_packed: bad logits dtype 3"),
    (packed_fwd(ws_bytes=4), -1, "tutel_amd_moe_forward_packed: routing workspace too small (4 bytes, need 16)"),
    (packed_fwd(dict(act=7)), -1, "tutel_amd_moe_forward_packed: unknown activation 7"),
    (packed_fwd(dict(x=Q[0] + 8)), -1, "tutel_amd_moe_forward_packed: x / weights / y / zero_row must be 16-byte aligned (biases 8-byte)"),
    (packed_fwd(BIG, **PROJECT), -1, "tutel_amd_moe_forward_packed: gate_partials must hold 16 x 256 x 64 floats"),
    (packed_fwd(w_up=None), -1, "tutel_amd_moe_forward_packed_glu: null w_up"),
    (packed_fwd(dict(b1=Q[32]), w_up=Q[33]), -1,
     "tutel_amd_moe_forward_packed_glu: SwiGLU experts take no biases, and w_up must be 16-byte aligned"),
    (packed_fwd(dict(act=NONE), w_up=Q[33]), ENOTSUP,
     "tutel_amd_moe_forward_packed_glu: not covered: the gate activation must be relu, gelu or silu"),
]

# (entry point and arguments, expected status, expected tutel_amd_last_error(); None: the call sets no error)
CASES = [
    (gemm(dtype=F32), -1, "tutel_amd_expert_gemm: dtype must be bf16 or fp16 (got 0)"),
    (gemm(K=96), -1, "tutel_amd_expert_gemm: K=96 must be a multiple of 64"),
    (gemm(N=12), -1, "tutel_amd_expert_gemm: N=12 must be a multiple of 8"),
    (gemm(K=96, N=12), -1, "tutel_amd_expert_gemm: K=96 must be a multiple of 64"),          # two faults: the first check answers
    (gemm(E_loc=0), 0, None),
    (gemm(E_loc=0, A=None), 0, None),                                                          # an empty problem is not looked at further
    (gemm(A=None), -1, "tutel_amd_expert_gemm: null pointer"),
    (gemm(lda=4), -1, "tutel_amd_expert_gemm: leading dimensions / strides must keep rows 16-byte aligned"),
    (gemm(A=P + 8), -1, "tutel_amd_expert_gemm: pointers must be 16-byte aligned"),
    (gemm(row_counts=P4, row_align=0), -1, "tutel_amd_expert_gemm: row_align must be >= 1"),
    (glu(None), -1, "tutel_amd_expert_gemm_glu: null gating operand"),
    (glu(P4 + 4), -1, "tutel_amd_expert_gemm_glu: gating operand must be 8-byte aligned"),
    (gather(slot_map=None), -1, "tutel_amd_expert_gemm_gather: need a slot map and T >= 1"),
    (gather(zero_row=None), -1, "tutel_amd_expert_gemm_gather: need a_rows_mod >= 1 and a 16-byte aligned zero row"),
    (gate_up(act=NONE), ENOTSUP, "tutel_amd_expert_gemm_gate_up: not covered: the gate activation must be relu, gelu or silu"),
    (gate_up(act=NONE, W_up=None), ENOTSUP, "tutel_amd_expert_gemm_gate_up: not covered: the gate activation must be relu, gelu or silu"),
    (gate_up(W_up=None), -1, "tutel_amd_expert_gemm_gate_up: W_up must be a 16-byte aligned pointer"),
    (gate_up(ldd=4), ENOTSUP, "tutel_amd_expert_gemm_gate_up: not covered: output rows must be 16-byte aligned"),
    (gate_up(R=1 << 20, lda=2048), ENOTSUP, "tutel_amd_expert_gemm_gate_up: not covered: operands past 2 GiB"),
    (packed(dtype=F32), ENOTSUP, "tutel_amd_expert_gemm_packed: not covered: 16-bit operands only"),
    (packed(w_kmajor=0, act=GELU), ENOTSUP, "tutel_amd_expert_gemm_packed: not covered: n-major weights take act none or relu"),
    (packed(w_kmajor=0, mul=P4), ENOTSUP, "tutel_amd_expert_gemm_packed: not covered: the gated form takes k-major weights"),
    (packed(offsets=None), -1, "tutel_amd_expert_gemm_packed: null pointer"),
    (packed(D=P3 + 8), -1, "tutel_amd_expert_gemm_packed: D and mul must be 16-byte aligned, ldd a multiple of 8"),
    # past the public checks: the internal entry point's own, then the GEMM's
    (packed(a_rows=P4, T=0), -1, "tutel_expert_gemm_packed: bad arguments"),
    (packed(K=96), -1, "tutel_amd_expert_gemm: K=96 must be a multiple of 64"),
    (packed(a_rows=P4, T=64), -1, "tutel_amd_expert_gemm_gather: need a_rows_mod >= 1 and a 16-byte aligned zero row"),
    (ffn(dtype=F32), -1, "tutel_amd_expert_ffn: dtype must be bf16 or fp16 (got 0)"),
    (ffn(), ENOTSUP, None),                                                                     # the option's default: the two launches
]
# with TUTEL_OPT_FFN_FUSED = 1 the persistent launch builds both GEMMs' argument blocks before it answers
FFN_FUSED_CASES = [
    (ffn(M=96), -1, "tutel_amd_expert_gemm: K=96 must be a multiple of 64"),
    (ffn(), ENOTSUP, None),                                                                     # valid, but not a shape the kernel covers
]


def _run(L, cases):
    marker = "tutel_amd_set_option: unknown key 99"
    for (name, args), status, text in cases:
        assert L.tutel_amd_set_option(99, 0) == -1                       # a known last error: a case that sets none leaves it standing
        assert getattr(L, name)(*args) == status, (name, args)
        assert L.tutel_amd_last_error().decode() == (marker if text is None else text), (name, args)


def test_refused_before_any_launch(L):
    _run(L, CASES)


def test_pipelines_refused_before_any_launch(L):
    _run(L, PIPELINE_CASES)


def test_fused_ffn_refused_before_any_launch(L):
    from tutel_amd import _lib
    assert L.tutel_amd_set_option(_lib.OPT_FFN_FUSED, 1) == 0
    try:
        _run(L, FFN_FUSED_CASES)
    finally:
        assert L.tutel_amd_set_option(_lib.OPT_FFN_FUSED, -1) == 0
