"""W8A16 (csrc/expert_gemm_w8.hip, tutel_amd_expert_gemm_w8; tutel_amd/experts/w8.py) without a GPU: the C ABI declares, exports and
binds both entry points, the coverage query on both sides of every limit, refusals that name their reason before anything is
enqueued, the quantiser against its formula written out here, bit for bit, the weight image's round trip, and every reason for which
a layer keeps its 16-bit weights."""
import ctypes
import os
import re
import subprocess
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("tutel_amd_expert_gemm_w8_supported", "tutel_amd_expert_gemm_w8")
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _call(L, E_loc=1, R=1, N=32, K=64, dtype=None, act=0, lda=None, ldd=None, a_rpw=None, a_sw=0, d_rpw=None, d_sw=0, w_stride=None,
          row_counts=None, bias_stride=0):
    """the entry point with null pointers everywhere: only the argument checks can answer"""
    from tutel_amd import _lib
    dtype = _lib.BF16 if dtype is None else dtype
    lda = K if lda is None else lda
    ldd = N if ldd is None else ldd
    return L.tutel_amd_expert_gemm_w8(None, R * lda, a_sw, max(R, 1) if a_rpw is None else a_rpw, lda, None, N * K if w_stride is None else w_stride,
                                      None, None, bias_stride, None, R * ldd, d_sw, max(R, 1) if d_rpw is None else d_rpw, ldd,
                                      E_loc, R, N, K, dtype, act, row_counts, None, 0, None, None)


def test_header_declares_and_signatures_bind_both_entry_points(L):
    from tutel_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " is not declared"
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == 26 and len(_lib.SIGNATURES[NAMES[0]][1]) == 3


def test_supported_query_on_both_sides_of_every_limit(L):
    from tutel_amd import _lib, ops
    q = L.tutel_amd_expert_gemm_w8_supported
    cases = {(32, 64): 1, (64, 64): 1, (96, 192): 1, (2048, 2048): 1, (288, 1024): 1,
             (0, 64): 0, (8, 64): 0, (16, 64): 0, (31, 64): 0, (33, 64): 0, (48, 64): 0, (-32, 64): 0,   # N: a positive multiple of 32
             (32, 0): 0, (32, 32): 0, (32, 63): 0, (32, 65): 0, (32, 96): 0, (32, -64): 0,              # K: a positive multiple of 64
             (64, 32): 0}
    for (N, K), want in cases.items():
        for code, dt in ((_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)):
            assert q(code, N, K) == want, (N, K)
            assert ops.gemm_w8_supported(dt, N, K) is bool(want), (N, K)
        assert q(_lib.F32, N, K) == 0 and q(-1, N, K) == 0 and q(3, N, K) == 0      # the dtype: bf16 or fp16 only
        assert ops.gemm_w8_supported(torch.float32, N, K) is False and ops.gemm_w8_supported(torch.float64, N, K) is False


def test_refusals_name_their_reason_and_enqueue_nothing(L):
    from tutel_amd import _lib
    counts = ctypes.c_void_p(64)   # any non-null address: it is never followed
    for kw, word in ((dict(K=96), b"K must be a multiple of 64"), (dict(K=100), b"K must be"), (dict(N=40), b"N must be a multiple of 32"),
                     (dict(N=8), b"N must be"), (dict(dtype=_lib.F32), b"bf16 or fp16"), (dict(dtype=7), b"bf16 or fp16"),
                     (dict(act=4), b"activation"), (dict(act=-1), b"activation"), (dict(row_counts=counts), b"row_counts"),
                     (dict(R=8, a_rpw=4, a_sw=1024), b"exchange layouts"), (dict(R=8, d_rpw=4), b"exchange layouts"),
                     (dict(d_sw=64), b"exchange layouts"), (dict(lda=68), b"aligned"), (dict(ldd=34), b"aligned"),
                     (dict(bias_stride=34), b"aligned"), (dict(w_stride=32 * 64 + 8), b"aligned"), (dict(w_stride=1024), b"image")):
        rc = _call(L, **kw)
        err = L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and b"not covered" in err and word in err, (kw, rc, err)
    # covered shape, null operands: an error (not ENOTSUP), still before any HIP call -- this machine may have no GPU at all
    rc = _call(L)
    assert rc not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _call(L, N=0) not in (0, _lib.ENOTSUP) and b"bad sizes" in L.tutel_amd_last_error()
    assert _call(L, R=-1) not in (0, _lib.ENOTSUP)
    # more rows than the addressing takes: refused, not wrapped
    assert _call(L, E_loc=1 << 20, R=1 << 12) == _lib.ENOTSUP and b"2^31" in L.tutel_amd_last_error()


def test_empty_problem_is_a_no_op(L):
    assert _call(L, E_loc=0, R=16) == 0 and _call(L, E_loc=4, R=0) == 0 and _call(L, E_loc=0, R=0) == 0


def test_switch_is_off_unless_the_environment_asks():
    code = ("from tutel_amd.experts import ffn; n = ffn.FusedExpertsNetwork(64, 32, 1, 1); "
            "print(int(ffn._FP8_WEIGHTS), int(n.fp8_weights))")
    for value, want in ((None, "0 0"), ("0", "0 0"), ("1", "1 1")):
        env = {k: v for k, v in os.environ.items() if k != "TUTEL_AMD_FP8_WEIGHTS"}
        if value is not None:
            env["TUTEL_AMD_FP8_WEIGHTS"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------
def _formula(w, w_kmajor):
    """the issue's formula, written out: scale = fp32(amax_k |w|) / 448.0f (all-zero channel: 1); q = e4m3_rne(clamp(fp32(w) / scale))"""
    wf = (w if w_kmajor else w.transpose(1, 2)).to(torch.float32)
    E, N, K = wf.shape
    scale = torch.empty([E, N], dtype=torch.float32)
    q = torch.empty([E, N, K], dtype=F8)
    for e in range(E):
        for n in range(N):
            amax = wf[e, n].abs().max()
            s = amax / torch.tensor(448.0, dtype=torch.float32) if float(amax) != 0.0 else torch.tensor(1.0)
            scale[e, n] = s
            q[e, n] = torch.clamp(wf[e, n] / s, -448.0, 448.0).to(F8)
    return q, scale


def _overflowing_channel(K):
    """a channel whose largest quotient rounds ABOVE 448 in fp32 before the clamp: amax = a, another element exactly a as well is 448 at
    best -- but scale = fl(a / 448) may round DOWN, and then a / scale > 448.  Search the fp32 values near 1 for such an a."""
    for i in range(1, 4096):
        a = torch.tensor(1.0 + i * 2.0 ** -23, dtype=torch.float32)
        s = a / torch.tensor(448.0, dtype=torch.float32)
        if float(a / s) > 448.0:
            ch = torch.linspace(-0.9, 0.9, K, dtype=torch.float32)
            ch[3], ch[K - 2] = a, -a
            return ch
    raise AssertionError("no fp32 value near 1 whose quotient by its own scale exceeds 448")


def _sources(K=64):
    g = torch.Generator().manual_seed(88)
    w = torch.randn([2, 6, K], generator=g)
    w[0, 1] = 0                                           # an all-zero channel
    w[0, 2] = torch.randn([K], generator=g) * 1e-3
    w[0, 2, 5] = 3.0e4                                    # one huge element: everything else falls into the subnormal codes or to zero
    w[1, 0] = _overflowing_channel(K)
    w[1, 3] = torch.randn([K], generator=g) * 1e-6
    return w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("w_kmajor", [True, False])
def test_quantize_equals_the_formula_bit_for_bit(dtype, w_kmajor):
    from tutel_amd.experts import w8
    w = _sources().to(dtype)
    src = w if w_kmajor else w.transpose(1, 2).contiguous()
    q, scale = w8.quantize_e4m3(src, w_kmajor)
    rq, rs = _formula(src, w_kmajor)
    assert q.dtype == F8 and q.shape == w.shape and scale.dtype == torch.float32 and scale.shape == w.shape[:2]
    assert torch.equal(scale.view(torch.int32), rs.view(torch.int32))
    assert torch.equal(q.view(torch.uint8), rq.view(torch.uint8))
    assert float(scale[0, 1]) == 1.0 and not q[0, 1].view(torch.uint8).any()
    # deterministic, and no NaN code for finite input
    q2, s2 = w8.quantize_e4m3(src, w_kmajor)
    assert torch.equal(q.view(torch.uint8), q2.view(torch.uint8)) and torch.equal(scale, s2)
    assert not ((q.view(torch.uint8) & 0x7F) == 0x7F).any()


def test_the_clamp_is_needed_and_applied():
    from tutel_amd.experts import w8
    ch = _overflowing_channel(64)
    amax = ch.abs().max()
    s = amax / torch.tensor(448.0, dtype=torch.float32)
    assert float((ch / s).abs().max()) > 448.0, "the constructed channel's pre-clamp quotient exceeds 448"
    q, scale = w8.quantize_e4m3(ch.view(1, 1, 64), True)
    assert float(scale) == float(s)
    codes = q.view(torch.uint8).view(-1)
    assert int(codes[3]) == 0x7E and int(codes[62]) == 0xFE and not ((codes & 0x7F) == 0x7F).any()
    # what the clamp keeps out: far enough above 448 torch's cast gives the NaN code
    assert int(torch.tensor([480.0]).to(F8).view(torch.uint8)) == 0x7F


def test_round_trip_error_bound():
    """per element: |q * scale - w| <= 2^-4 |w| where |w / scale| >= 2^-6 (3 mantissa bits: half an ulp is 2^-4 relative), and
    <= 2^-10 scale below (subnormal spacing 2^-9).  The product q * scale and the quotient are taken in float64 here and the bounds
    are held as stated, with no slack (the quantiser's fp32 quotient could exceed them by a relative 2^-24 only on an exact tie)."""
    from tutel_amd.experts import w8
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        w = _sources(256).to(dtype)
        q, scale = w8.quantize_e4m3(w, True)
        wd, sd = w.double(), scale.double().unsqueeze(2)
        err = (q.double() * sd - wd).abs()
        big = (wd / sd).abs() >= 2.0 ** -6
        slack = 1.0
        assert bool((err[big] <= 2.0 ** -4 * wd.abs()[big] * slack).all())
        assert bool((err[~big] <= (2.0 ** -10 * sd).expand_as(err)[~big] * slack).all())
        assert int(big.sum()) > 0 and int((~big).sum()) > 0


def test_non_finite_weights_raise():
    from tutel_amd.experts import w8
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = torch.randn([2, 4, 64])
        w[1, 2, 7] = bad
        with pytest.raises(ValueError, match="non-finite"):
            w8.quantize_e4m3(w, True)
        with pytest.raises(ValueError, match="non-finite"):
            w8.quantize_e4m3(w.transpose(1, 2).contiguous(), False)


@pytest.mark.parametrize("K", [64, 192, 1024])
@pytest.mark.parametrize("N", [32, 96, 160, 288, 2048])
def test_pack_unpack_round_trip(N, K):
    from tutel_amd.experts import w8
    E = 2
    g = torch.Generator().manual_seed(N * 7 + K)
    codes = torch.randint(0, 256, [E, N, K], generator=g, dtype=torch.uint8)
    q = codes.view(F8)
    image = w8.pack(q)
    assert image.dtype == torch.uint8 and image.is_contiguous() and image.numel() == E * N * K
    assert torch.equal(w8.unpack(image, N, K).view(torch.uint8), codes)
    # the layout of include/tutel_amd.h, spelled out at a few places
    flat = image.view(E, -1)
    for (e, n, k) in ((0, 0, 0), (1, 33 % N, 17), (0, N - 1, K - 1), (1, N // 2 + 5, K // 2 + 9)):
        g_, l31, t, r = n // 32, n % 32, k // 32, k % 32
        s, kg, j = r // 16, (r % 16) // 8, r % 8
        off = ((g_ * (K // 32) + t) * 64 + (32 * kg + l31)) * 16 + 8 * s + j
        assert int(flat[e, off]) == int(codes[e, n, k]), (e, n, k)


def test_pack_pads_with_code_zero():
    from tutel_amd.experts import w8
    codes = torch.randint(1, 256, [1, 40, 72], dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    image = w8.pack(codes.view(F8))
    assert image.shape == (1, 2, 3, 64, 16)
    assert torch.equal(w8.unpack(image, 40, 72).view(torch.uint8), codes)
    assert int((image == 0).sum()) == 64 * 96 - 40 * 72 and int((image != 0).sum()) == 40 * 72


# ---- the layer's predicate --------------------------------------------------------------------------------------------------------
class _CudaLike:
    """stands in for a device tensor where only dtype / device flags are looked at (this machine has no GPU)"""
    is_cuda, dtype, requires_grad = True, torch.bfloat16, False


def _net(M=64, H=64, dtype=torch.bfloat16):
    from tutel_amd.experts import ffn
    net = ffn.FusedExpertsNetwork(M, H, 2, 1).to(dtype).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def test_w8_refusal_returns_each_reason(L, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    net = _net()
    ctx = types.SimpleNamespace(sharded_count=1, adaptive_degree=1, megablocks_size=0)
    dev = _CudaLike()
    assert net.fp8_weights is False and "off" in net.w8_refusal(dev, ctx)
    net.fp8_weights = True
    assert net.w8_refusal(dev, ctx) is None, "the admitted case, so that each exclusion below shows"
    assert "device" in net.w8_refusal(torch.zeros([2, 4, 64], dtype=torch.bfloat16), ctx)
    for field, value, word in (("sharded_count", 2, "gathered"), ("adaptive_degree", 0, "gathered"), ("megablocks_size", 4, "megablocks")):
        bad = types.SimpleNamespace(**{**vars(ctx), field: value})
        assert word in net.w8_refusal(dev, bad), field
    assert "megablocks" in net.w8_refusal(dev, ctx, megablocks_size=2)
    for dt in (torch.float32, torch.float16, torch.float64):   # not 16-bit, or not the weights' own dtype
        other = _CudaLike()
        other.dtype = dt
        assert "dtype" in net.w8_refusal(other, ctx), dt
    half = _CudaLike()
    half.dtype = torch.float16
    assert _net(dtype=torch.float16).w8_refusal(half, ctx) == "fp8_weights is off (TUTEL_AMD_FP8_WEIGHTS)"
    h = _net(dtype=torch.float16)
    h.fp8_weights = True
    assert h.w8_refusal(half, ctx) is None
    net.train()
    assert "training mode" in net.w8_refusal(dev, ctx)
    net.eval()
    with monkeypatch.context() as m:   # (the device's autocast state: nothing can switch it on without the device)
        m.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert "autocast" in net.w8_refusal(dev, ctx)
    net.batched_fc1_w.requires_grad_(True)
    assert "autograd" in net.w8_refusal(dev, ctx)
    with torch.no_grad():
        assert net.w8_refusal(dev, ctx) is None
    net.batched_fc1_w.requires_grad_(False)
    net.skip_expert = True
    assert "SKIP_EXPERT" in net.w8_refusal(dev, ctx)
    net.skip_expert = False
    net.activation_fn, net._act_cache = (lambda t: t.clamp(0, 6)), {}
    assert "activation" in net.w8_refusal(dev, ctx)
    for M, H in ((64, 96), (96, 64), (64, 48)):   # fc2's K = 96; fc1's K = 96 and fc2's N = 96 % 32 == 0 but K; H = 48: no multiple of 32
        narrow = _net(M, H)
        narrow.fp8_weights = True
        assert "shape" in narrow.w8_refusal(dev, ctx), (M, H)
    # a first use inside a graph capture: the images are not cached, quantising would allocate in the graph's pool
    ok = _net()
    ok.fp8_weights = True
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert "eager forward" in ok.w8_refusal(dev, ctx)
    ok.w8_params()
    assert ok.w8_refusal(dev, ctx) is None
    with torch.no_grad():
        ok.batched_fc2_w.mul_(2)   # the version counter moved: the cached image is stale
    assert "eager forward" in ok.w8_refusal(dev, ctx)


def test_cache_requantises_when_the_parameter_changes():
    from tutel_amd.experts import w8
    net = _net()
    (i1, s1), (i2, s2) = net.w8_params()
    again = net.w8_params()
    assert again[0][0] is i1 and again[1][0] is i2, "a hit returns the cached image"
    q2, rs2 = w8.quantize_e4m3(net.batched_fc2_w, False)
    assert torch.equal(w8.unpack(i2, 64, 64).view(torch.uint8), q2.view(torch.uint8)) and torch.equal(s2, rs2)
    with torch.no_grad():
        net.batched_fc1_w.mul_(2)
    (j1, t1), (j2, _) = net.w8_params()
    assert j1 is not i1 and j2 is i2 and torch.equal(t1, s1 * 2) and torch.equal(j1, i1)   # a power of two moves the scale only
    for poke in (lambda: net.train(), lambda: net.eval(), lambda: net.load_state_dict(net.state_dict()), lambda: net.to(torch.bfloat16).float().bfloat16()):
        before = net.w8_params()[0][0]
        poke()
        assert net.w8_params()[0][0] is not before
    # the k-major copies share the store and the key rule
    k2 = net._kmajor.get("fc2", net.batched_fc2_w)
    assert net._kmajor.get("fc2", net.batched_fc2_w) is k2 and torch.equal(k2, net.batched_fc2_w.transpose(1, 2))
