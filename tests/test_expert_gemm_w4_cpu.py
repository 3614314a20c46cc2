"""W4A16 (csrc/expert_gemm_w4.hip, tutel_amd_expert_gemm_w4 / _w4_glu; tutel_amd/experts/w4.py) without a GPU: the e2m1 grid and the
admitted scale bytes, the quantiser's rounding and scale rule, its derived error bound and idempotence in value, the weight image's
round trip with hand-computed bytes, the scale check, the refusals of the C ABI before any HIP call, and the order of the W4 ladder."""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BF16, F16 = torch.bfloat16, torch.float16
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _w4():
    from tutel_amd.experts import w4
    return w4


def _codes_of(values, dtype=BF16, scale_from=None):
    """quantise ONE block [1, 1, 32] holding `values` (padded with zeros) -> (the codes as a list, one per element, the scale byte)"""
    w4 = _w4()
    w = torch.zeros([1, 1, 32])
    w[0, 0, :len(values)] = torch.tensor(values, dtype=torch.float32)
    codes, scales = w4.quantize_mxfp4(w, True, dtype)
    return w4.unpack_nibbles(codes)[0, 0, :len(values)].tolist(), int(scales[0, 0, 0])


# ---- 1. the grid ------------------------------------------------------------------------------------------------------------------
def test_all_sixteen_codes_dequantise_to_the_e2m1_values():
    w4 = _w4()
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)            # one block of 32: every code twice
    packed = (codes[0::2] | (codes[1::2] << 4)).view(1, 1, 16)
    dq = w4.dequantize(packed, torch.tensor([[[127]]], dtype=torch.uint8))
    assert dq[0, 0, :16].tolist() == GRID + [-v for v in GRID]
    assert torch.equal(dq[0, 0, 16:], dq[0, 0, :16])
    assert torch.equal(w4.dequantize(packed, torch.tensor([[[130]]], dtype=torch.uint8)), dq * 8)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_every_value_under_every_admitted_exponent_is_a_normal_number_of_the_dtype(dtype):
    w4 = _w4()
    lo, hi = w4.SCALE_RANGE[dtype]
    assert (lo, hi) == ((2, 252) if dtype == BF16 else (114, 140))
    fi = torch.finfo(dtype)
    vals = torch.tensor(GRID[1:], dtype=torch.float64)

    def representable(s):   # every non-zero value times 2^(s - 127): finite, normal and exact in the dtype
        x = vals * 2.0 ** (s - 127)
        r = x.to(dtype)
        return bool(torch.isfinite(r).all() and (r.double() == x).all() and (r.double().abs() >= fi.smallest_normal).all())

    for s in range(lo, hi + 1):
        assert representable(s), s
    assert not representable(lo - 1), "0.5 * 2^e leaves the normal range one step below"
    assert not representable(hi + 1), "6 * 2^e overflows one step above"
    assert 0.5 * 2.0 ** (lo - 127) == fi.smallest_normal and 6 * 2.0 ** (hi + 1 - 127) > fi.max


# ---- 2. rounding ------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_even_neighbour_and_the_rest_to_the_nearer():
    # amax 6 -> e = 0: the codes are those of the values themselves
    ties = {0.25: 0, 0.75: 2, 1.25: 2, 1.75: 4, 2.5: 4, 3.5: 6, 5.0: 6}       # tie -> the code with mantissa bit 0
    below = {0.25: 0, 0.75: 1, 1.25: 2, 1.75: 3, 2.5: 4, 3.5: 5, 5.0: 6}
    for t, code in ties.items():
        got, s = _codes_of([6.0, t, -t, t * (1 - 2.0 ** -20), t * (1 + 2.0 ** -20), -t * (1 + 2.0 ** -20)])
        assert s == 127
        assert got[0] == 7 and got[1] == code and got[2] == (code | 8 if code else 0), (t, got)
        assert got[3] == below[t] and got[4] == below[t] + 1 and got[5] == (below[t] + 1) | 8, (t, got)
    for v in GRID:
        assert _codes_of([6.0, v])[0][1] == GRID.index(v)


def test_saturation_and_signs():
    w4 = _w4()
    # a block whose exponent is clamped at the top of fp16's range: amax 2^18 wants e = 16, gets 13 -> 6.5 * 2^13 and 7.99 * 2^13 saturate
    hi = 2.0 ** 13
    got, s = _codes_of([2.0 ** 18, 6.5 * hi, 7.99 * hi, -6.5 * hi, 6.0 * hi, 5.5 * hi], F16)
    assert s == 140 and got == [7, 7, 7, 15, 7, 7]
    # signs are kept; a value that rounds to zero gets code 0x0 whatever its sign -- -0 included: the image holds no negative zero
    got, _ = _codes_of([6.0, -6.0, -0.5, -0.0, 0.0, -0.2, 0.2, -0.26])
    assert got == [7, 15, 9, 0, 0, 0, 0, 9]
    codes, scales = w4.quantize_mxfp4(torch.full([1, 1, 32], -0.0), True, BF16)
    assert int(scales[0, 0, 0]) == 127 and not bool(codes.any())


# ---- 3. the scale rule ------------------------------------------------------------------------------------------------------------
def test_scale_byte_is_floor_log2_amax_minus_two():
    for j in (-100, -14, -3, 0, 1, 5, 14, 100):
        for m in (1.0, 1.99, 6.0):
            # 6 * 2^j = 1.5 * 2^(j + 2): the rule's floor(log2) is j + 2 there
            want = (j + 2 if m == 6.0 else j) - 2 + 127
            assert _codes_of([m * 2.0 ** j, -0.3 * 2.0 ** j])[1] == want, (j, m)
    assert _codes_of([0.0])[1] == 127
    got, s = _codes_of([2.0 ** -20, -(2.0 ** -20)], F16)
    assert s == 114 and got == [0, 0], "below fp16's range: the byte is clamped and the codes underflow to zero"
    assert _codes_of([2.0 ** -140], BF16)[1] == 2, "an fp32 subnormal amax: clamped to the bottom"


def test_non_finite_weights_raise_naming_their_channel():
    w4 = _w4()
    for bad in (float("inf"), float("-inf"), float("nan")):
        w = torch.ones([3, 4, 64])
        w[2, 1, 40] = bad
        with pytest.raises(ValueError, match=r"expert 2, output 1"):
            w4.quantize_mxfp4(w, True, BF16)
        with pytest.raises(ValueError, match=r"expert 2, output 1"):
            w4.quantize_mxfp4(w.transpose(1, 2).contiguous(), False, BF16)
    with pytest.raises(AssertionError):
        w4.quantize_mxfp4(torch.ones([1, 2, 48]), True, BF16)
    with pytest.raises(AssertionError):
        w4.quantize_mxfp4(torch.ones([1, 2, 64]), True)   # fp32 weights: the activations' dtype has to be named


# ---- 4. the error bound, 5. idempotence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF16, F16])
@pytest.mark.parametrize("w_kmajor", [True, False])
def test_error_bound_and_idempotence_in_value(dtype, w_kmajor):
    """|w - dq| <= 0.5 amax per block, derived: with e = floor(log2(amax)) - 2, amax / 2^e is in [4, 8); inside the grid the distance to
    the nearest point is at most half the widest gap, 1 = 0.25 * 4 <= 0.25 amax / 2^e; a value above 6 saturates with an error below
    8 - 6 = 2 <= 0.5 amax / 2^e.  Holds for blocks whose exponent was not clamped.  And quantising the dequantised weights again gives
    the same VALUES bit for bit (the codes may differ: a block whose largest code is below 4 gets a smaller exponent)."""
    w4 = _w4()
    act = BF16 if dtype == torch.float32 else dtype
    w = torch.randn([3, 96, 128], generator=torch.Generator().manual_seed(5)).to(dtype)
    w[1, 7, 32:64] = 0
    w[2, 9, 5] = 30.0
    if not w_kmajor:
        w = w.transpose(1, 2).contiguous()
    codes, scales = w4.quantize_mxfp4(w, w_kmajor, act)
    lo, hi = w4.SCALE_RANGE[act]
    assert bool(((scales > lo) & (scales < hi)).all()), "no block of this draw is clamped"
    dq = w4.dequantize(codes, scales)
    wf = (w if w_kmajor else w.transpose(1, 2)).float().reshape(3, 96, 4, 32)
    err = (wf - dq.view(3, 96, 4, 32)).abs()
    amax = wf.abs().amax(dim=3, keepdim=True)
    assert bool((err <= 0.5 * amax).all()), float((err / amax.clamp_min(1e-30)).max())
    assert float((err / amax.clamp_min(1e-30)).max()) > 0.1, "the bound is not vacuous on this draw"
    codes2, scales2 = w4.quantize_mxfp4(dq, True, act)
    assert torch.equal(w4.dequantize(codes2, scales2).view(torch.int32), dq.view(torch.int32))
    assert torch.equal(w4.dequantize(codes, scales, act).float(), dq), "exact in the activations' dtype"


def test_idempotence_for_every_largest_code():
    """a block whose largest code is c: the second pass picks e' = e + floor(log2(val(c))) - 2 and every value stays on its grid"""
    w4 = _w4()
    for top in range(1, 8):
        for byte in (114, 116, 124, 140):   # the bottom of fp16's range too: the second exponent is clamped there
            one = (torch.arange(32) % (top + 1)).to(torch.uint8)
            one[1::2] |= 8
            dq = w4.dequantize((one[0::2] | (one[1::2] << 4)).view(1, 1, 16), torch.tensor([[[byte]]], dtype=torch.uint8))
            assert float(dq.abs().max()) == GRID[top] * 2.0 ** (byte - 127)
            c2, s2 = w4.quantize_mxfp4(dq, True, F16)
            assert torch.equal(w4.dequantize(c2, s2), dq), (top, byte)


# ---- 6. pack / unpack -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(32, 64), (96, 192), (160, 320)])
def test_pack_unpack_round_trip_and_hand_computed_bytes(N, K):
    w4 = _w4()
    g = torch.Generator().manual_seed(N + K)
    E = 2
    codes = torch.randint(0, 256, [E, N, K // 2], generator=g, dtype=torch.uint8)
    scales = torch.randint(2, 253, [E, N, K // 32], generator=g, dtype=torch.uint8)
    ci, si = w4.pack(codes, scales)
    T = (K + 127) // 128
    assert ci.shape == (E, N // 32, K // 64, 64, 16) and si.shape == (E, N // 32, T, 32, 4) and ci.is_contiguous() and si.is_contiguous()
    c2, s2 = w4.unpack(ci, si, N, K)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    # the layout rule, element by element: nibble j of dword q of lane l of block (g, t) is the code of channel 32 g + (l & 31) at
    # k = 64 t + 16 q + 8 (l >> 5) + j
    one = w4.unpack_nibbles(codes)
    flat = ci.view(E, N // 32, K // 64, 64, 4, 4)
    for (e, gi, t, l, q, j) in ((0, 0, 0, 0, 0, 0), (1, N // 32 - 1, K // 64 - 1, 63, 3, 7), (0, N // 64, 0, 37, 2, 5), (1, 0, K // 64 - 1, 31, 1, 2)):
        byte = int(flat[e, gi, t, l, q, j // 2])
        nib = (byte >> 4) if j & 1 else (byte & 15)
        assert nib == int(one[e, 32 * gi + (l & 31), 64 * t + 16 * q + 8 * (l >> 5) + j]), (e, gi, t, l, q, j)
    # scales: byte i of channel c of block (g, t128) is k-block 4 t128 + i; the pad is 127
    for (e, gi, t, c, i) in ((0, 0, 0, 0, 0), (1, N // 32 - 1, T - 1, 31, 0), (0, 0, T - 1, 17, 3), (1, N // 64, 0, 5, 2)):
        b = 4 * t + i
        assert int(si[e, gi, t, c, i]) == (int(scales[e, 32 * gi + c, b]) if b < K // 32 else 127), (e, gi, t, c, i)
    pad = torch.arange(4 * T).view(1, 1, T, 1, 4).expand_as(si) >= K // 32
    assert bool((si[pad] == 127).all()) and int(pad.sum()) == E * N * (4 * T - K // 32)


def test_pack_refuses_shapes_the_kernel_does_not_cover():
    w4 = _w4()
    with pytest.raises(AssertionError):
        w4.pack(torch.zeros([1, 48, 32], dtype=torch.uint8), torch.zeros([1, 48, 2], dtype=torch.uint8))
    with pytest.raises(AssertionError):
        w4.pack(torch.zeros([1, 32, 48], dtype=torch.uint8), torch.zeros([1, 32, 3], dtype=torch.uint8))


def test_prepare_gate_up_is_pack_of_the_interleaved_order():
    from tutel_amd.experts import w8
    w4 = _w4()
    g = torch.Generator().manual_seed(3)
    wg, wu = torch.randn([2, 64, 48], generator=g).to(BF16), torch.randn([2, 64, 48], generator=g).to(BF16)   # [E, K, H]: n-major storage
    ci, si = w4.prepare_gate_up(wg, wu, False)
    cg, sg = w4.quantize_mxfp4(wg, False)
    cu, su = w4.quantize_mxfp4(wu, False)
    want_c, want_s = w4.pack(w8.interleave_gate_up(cg, cu), w8.interleave_gate_up(sg, su))
    assert torch.equal(ci, want_c) and torch.equal(si, want_s)
    codes, scales = w4.unpack(ci, si, 96, 64)
    assert torch.equal(codes[:, 0:16], cg[:, 0:16]) and torch.equal(codes[:, 16:32], cu[:, 0:16]) and torch.equal(scales[:, 80:96], su[:, 32:48])
    w = torch.randn([2, 64, 32], generator=g).to(F16)
    c1, s1 = w4.prepare(w, False)
    want = w4.pack(*w4.quantize_mxfp4(w.transpose(1, 2).contiguous(), True))
    assert torch.equal(c1, want[0]) and torch.equal(s1, want[1])


# ---- 7. check_scales --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,lo,hi", [(BF16, 2, 252), (F16, 114, 140)])
def test_check_scales_accepts_the_range_and_refuses_one_step_outside(dtype, lo, hi):
    w4 = _w4()
    s = torch.full([2, 3, 4], 127, dtype=torch.uint8)
    s[0, 0, 0], s[1, 2, 3] = lo, hi
    w4.check_scales(s, dtype)
    for bad in (lo - 1, hi + 1, 0xFF, 0):
        t = s.clone()
        t[1, 2, 1] = bad
        with pytest.raises(ValueError, match=r"scale byte %d of \(expert 1, channel 2, block 1\)" % bad):
            w4.check_scales(t, dtype)


# ---- 8. the C ABI refuses before any HIP call -------------------------------------------------------------------------------------
def _call(L, glu=False, E_loc=1, R=1, N=32, K=64, dtype=None, act=0, lda=None, ldd=None, a_rpw=None, a_sw=0, d_rpw=None, d_sw=0, w_stride=None,
          s_stride=None, row_counts=None, bias_stride=0, ptrs=(None, None, None, None)):
    """an entry point with null pointers everywhere (N: H for the GLU form): only the argument checks can answer"""
    from tutel_amd import _lib
    dtype = _lib.BF16 if dtype is None else dtype
    lda = K if lda is None else lda
    ldd = N if ldd is None else ldd
    NI = 2 * N if glu else N
    w_stride = NI * K // 2 if w_stride is None else w_stride
    s_stride = NI * ((K + 127) // 128) * 4 if s_stride is None else s_stride
    A, Wq, Ws, D = ptrs
    head = (A, R * lda, a_sw, max(R, 1) if a_rpw is None else a_rpw, lda, Wq, w_stride, Ws, s_stride)
    tail = (D, R * ldd, d_sw, max(R, 1) if d_rpw is None else d_rpw, ldd, E_loc, R, N, K, dtype, act, row_counts, None, 0, None, None)
    if glu:
        return L.tutel_amd_expert_gemm_w4_glu(*head, *tail)
    return L.tutel_amd_expert_gemm_w4(*head, None, bias_stride, *tail)


def test_signatures_and_supported_queries(L):
    from tutel_amd import _lib, ops
    assert len(_lib.SIGNATURES["tutel_amd_expert_gemm_w4"][1]) == 27 and len(_lib.SIGNATURES["tutel_amd_expert_gemm_w4_glu"][1]) == 25
    q, qg = L.tutel_amd_expert_gemm_w4_supported, L.tutel_amd_expert_gemm_w4_glu_supported
    for (N, K), want in {(32, 64): 1, (96, 192): 1, (2048, 2048): 1, (48, 64): 0, (16, 64): 0, (0, 64): 0, (32, 96): 0, (32, 32): 0, (32, 0): 0}.items():
        for code, dt in ((_lib.BF16, BF16), (_lib.F16, F16)):
            assert q(code, N, K) == want and ops.gemm_w4_supported(dt, N, K) is bool(want), (N, K)
        assert q(_lib.F32, N, K) == 0 and ops.gemm_w4_supported(torch.float32, N, K) is False
    for (H, K), want in {(16, 64): 1, (48, 192): 1, (1024, 2048): 1, (8, 64): 0, (24, 64): 0, (16, 96): 0, (0, 64): 0}.items():
        for code, dt in ((_lib.BF16, BF16), (_lib.F16, F16)):
            assert qg(code, H, K) == want and ops.gemm_w4_glu_supported(dt, H, K) is bool(want), (H, K)
        assert qg(_lib.F32, H, K) == 0 and ops.gemm_w4_glu_supported(torch.float32, H, K) is False


@pytest.mark.parametrize("glu", [False, True], ids=["plain", "glu"])
def test_refusals_name_their_reason_and_enqueue_nothing(L, glu):
    from tutel_amd import _lib
    counts = ctypes.c_void_p(64)   # any non-null address: it is never followed
    bad_n = (dict(N=24), b"H must be a multiple of 16") if glu else (dict(N=48), b"N must be a multiple of 32")
    cases = [(dict(K=96), b"K must be a multiple of 64"), bad_n, (dict(dtype=_lib.F32), b"bf16 or fp16"), (dict(act=4), b"activation"),
             (dict(row_counts=counts), b"row_counts"), (dict(R=8, a_rpw=4, a_sw=1024), b"exchange layouts"), (dict(R=8, d_rpw=4), b"exchange layouts"),
             (dict(d_sw=64), b"exchange layouts"), (dict(lda=68), b"aligned"), (dict(ldd=34), b"aligned"), (dict(w_stride=4096 + 8), b"aligned"),
             (dict(s_stride=1024 + 2), b"aligned"), (dict(w_stride=512), b"image"), (dict(s_stride=64), b"image")]
    if not glu:
        cases.append((dict(bias_stride=34), b"aligned"))
    for kw, word in cases:
        rc = _call(L, glu, **kw)
        err = L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and b"not covered" in err and word in err, (kw, rc, err)
    # a covered shape: null operands and a misaligned pointer are argument errors (not ENOTSUP), still before any HIP call
    assert _call(L, glu) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    for ptrs in ((4096 + 8, 4096, 4096, 4096), (4096, 4096 + 8, 4096, 4096), (4096, 4096, 4096 + 2, 4096), (4096, 4096, 4096, 4096 + 4)):
        rc = _call(L, glu, ptrs=tuple(ctypes.c_void_p(p) for p in ptrs))
        assert rc not in (0, _lib.ENOTSUP) and b"aligned" in L.tutel_amd_last_error(), ptrs
    assert _call(L, glu, N=0) not in (0, _lib.ENOTSUP) and b"bad sizes" in L.tutel_amd_last_error()
    assert _call(L, glu, E_loc=1 << 20, R=1 << 12) == _lib.ENOTSUP and b"2^31" in L.tutel_amd_last_error()
    assert _call(L, glu, E_loc=0, R=16) == 0 and _call(L, glu, E_loc=4, R=0) == 0


def test_switch_is_off_unless_the_environment_asks():
    code = ("from tutel_amd.experts import ffn, llama_ffn; n = ffn.FusedExpertsNetwork(64, 32, 1, 1); m = llama_ffn.LlamaFFNNetwork(64, 64, 1, 1); "
            "print(int(ffn._FP4_WEIGHTS), int(n.fp4_weights), int(m.fp4_weights), int(n.fp8_weights))")
    for value, want in ((None, "0 0 0 0"), ("0", "0 0 0 0"), ("1", "1 1 1 0")):
        env = {k: v for k, v in os.environ.items() if k not in ("TUTEL_AMD_FP4_WEIGHTS", "TUTEL_AMD_FP8_WEIGHTS")}
        if value is not None:
            env["TUTEL_AMD_FP4_WEIGHTS"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


# ---- 9. the order of the W4 ladder ------------------------------------------------------------------------------------------------
class _CudaLike:
    """stands in for a device tensor where only dtype / device flags are looked at"""
    is_cuda, dtype, requires_grad = True, torch.bfloat16, False


def _walk(refusal, steps):
    for want, repair in steps:
        assert refusal() == want
        repair()
    assert refusal() is None


def test_fp4_weights_ladder_order(L, monkeypatch):
    """a state that fails EVERY check at once is repaired one check at a time: the reason moves down the ladder in this order"""
    from tutel_amd.experts import ffn
    net = ffn.FusedExpertsNetwork(64, 48, 2, 1).to(BF16)   # hidden size 48: no multiple of 64 (fc2's K)
    net.skip_expert = True
    x = _CudaLike()
    x.is_cuda, x.dtype = False, torch.float32
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    for p in net.parameters():
        p.requires_grad_(p is net.batched_fc1_w)
    ctx = types.SimpleNamespace(sharded_count=2, adaptive_degree=1, megablocks_size=4)
    net.activation_fn, net._act_cache = (lambda t: t.clamp(0, 6)), {}
    net.train()
    net.fp4_weights, net.fp8_weights, net.fp8_frozen = False, True, True
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)

    def resize():
        for name, shape in (("batched_fc1_w", [2, 64, 64]), ("batched_fc2_w", [2, 64, 64]), ("batched_fc1_bias", [2, 64]), ("batched_fc2_bias", [2, 64])):
            setattr(net, name, torch.nn.Parameter(torch.zeros(shape, dtype=BF16), requires_grad=False))

    def relu():
        net.activation_fn, net._act_cache = torch.nn.functional.relu, {}

    assert ffn.ENGINES.index(ffn.W4) == ffn.ENGINES.index(ffn.W8) + 1 and not ffn.W4.on(net)
    with torch.enable_grad():
        _walk(lambda: net.w4_refusal(x, ctx), [
            ("fp4_weights is off (TUTEL_AMD_FP4_WEIGHTS)", lambda: setattr(net, "fp4_weights", True)),
            ("fp8_weights is on as well (one weight format per module)", lambda: setattr(net, "fp8_weights", False)),
            ("the module is FP8-resident", lambda: setattr(net, "fp8_frozen", False)),
            ("SKIP_EXPERT is set", lambda: setattr(net, "skip_expert", False)),
            ("the input is not on the HIP device", lambda: setattr(x, "is_cuda", True)),
            ("autograd is live (FP8 weights are inference only)", lambda: net.batched_fc1_w.requires_grad_(False)),
            ("the module is in training mode (FP8 weights are inference only)", lambda: net.eval()),
            ("autocast is on", lambda: monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: False)),
            ("the input is not bf16 / fp16 in the experts' own dtype", lambda: setattr(x, "dtype", BF16)),
            ("gathered-weight modes (sharded experts, adaptive_r = 0) are not covered", lambda: setattr(ctx, "sharded_count", 1)),
            ("megablocks row counts are not covered", lambda: setattr(ctx, "megablocks_size", 0)),
            ("the activation is not one of the fused epilogues", relu),
            ("the shape is not covered (M and H multiples of 64, H and M_out multiples of 32)", resize),
            ("the quantised weights are not cached yet: run one eager forward before capturing a graph", lambda: net.w4_params()),
        ])
    assert net.admitted_engine(x, ctx) is ffn.W4
    # a parameter update rebuilds the images (KMajorCache's rule); the FP8 switch on top hands the forward to the W8 engine
    (c1, _), _ = net.w4_params()
    with torch.no_grad():
        net.batched_fc1_w.add_(1.0)
    assert net.w4_refusal(x, ctx) == "the quantised weights are not cached yet: run one eager forward before capturing a graph"
    assert net.w4_params()[0][0] is not c1 and net.w4_refusal(x, ctx) is None
    net.fp8_weights = True
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert net.admitted_engine(x, ctx) is ffn.W8 and net.w4_refusal(x, ctx) == "fp8_weights is on as well (one weight format per module)"


def test_swiglu_ladder_order(L, monkeypatch):
    from tutel_amd.experts import llama_ffn
    net = llama_ffn.LlamaFFNNetwork(64, 48, 2, 1).to(BF16)   # H = 48: fc3's K is no multiple of 64
    x = _CudaLike()
    x.is_cuda, x.dtype = False, torch.float32
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    ctx = types.SimpleNamespace(sharded_count=1, adaptive_degree=0)
    net.activation_fn, net._act_cache = (lambda t: t.clamp(0, 6)), {}
    net.train()
    net.fp4_weights, net.fp8_weights, net.fp8_frozen = False, True, True
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)

    def resize():
        E, M, H = 2, 64, 64
        net.W_fc1_full_shape, net.W_fc2_full_shape, net.W_fc3_full_shape = torch.Size([E, M, H]), torch.Size([E, M, H]), torch.Size([E, H, M])
        for name in ("W_fc1", "W_fc2", "W_fc3"):
            setattr(net, name, torch.nn.Parameter(torch.zeros([E * M * H], dtype=BF16), requires_grad=False))

    def silu():
        net.activation_fn, net._act_cache = torch.nn.functional.silu, {}

    with torch.enable_grad():
        _walk(lambda: net.w4_refusal(x, ctx), [
            ("fp4_weights is off (TUTEL_AMD_FP4_WEIGHTS)", lambda: setattr(net, "fp4_weights", True)),
            ("fp8_weights is on as well (one weight format per module)", lambda: setattr(net, "fp8_weights", False)),
            ("the module is FP8-resident", lambda: setattr(net, "fp8_frozen", False)),
            ("the input is not on the HIP device", lambda: setattr(x, "is_cuda", True)),
            ("autograd is live (FP8 weights are inference only)", lambda: [p.requires_grad_(False) for p in net.parameters()]),
            ("the module is in training mode (FP8 weights are inference only)", lambda: net.eval()),
            ("autocast is on", lambda: monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: False)),
            ("the input is not bf16 / fp16 in the experts' own dtype", lambda: setattr(x, "dtype", BF16)),
            ("gathered-weight modes (sharded experts, adaptive_r = 0) are not covered", lambda: setattr(ctx, "adaptive_degree", 1)),
            ("the activation is not one of the fused epilogues", silu),
            ("the shape is not covered (M a multiple of 64, H a multiple of 64)", resize),
            ("the quantised weights are not cached yet: run one eager forward before capturing a graph", lambda: net.w4_params()),
        ])
