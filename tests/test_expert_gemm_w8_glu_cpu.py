"""The W8A16 gate / up GEMM of SwiGLU experts (csrc/expert_gemm_w8.hip, tutel_amd_expert_gemm_w8_glu; tutel_amd/experts/w8.py) without
a GPU: the C ABI declares, exports and binds both entry points, the coverage query on both sides of every limit, refusals that name
their reason before anything is enqueued, the gate / up interleave and its image against a closed form written here independently
of pack, and every reason for which a SwiGLU layer keeps its 16-bit weights, in ladder order, with the cache's keys."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from test_expert_gemm_w8_cpu import L, _CudaLike   # noqa: E402,F401  (the built library; the device tensor's stand-in)

NAMES = ("tutel_amd_expert_gemm_w8_glu_supported", "tutel_amd_expert_gemm_w8_glu")
F8 = torch.float8_e4m3fn


def _call(L, E_loc=1, R=1, H=16, K=64, dtype=None, act=3, lda=None, ldd=None, a_rpw=None, a_sw=0, d_rpw=None, d_sw=0, w_stride=None,
          row_counts=None, a_se=None, d_se=None):
    """the entry point with null pointers everywhere: only the argument checks can answer"""
    from tutel_amd import _lib
    dtype = _lib.BF16 if dtype is None else dtype
    lda = K if lda is None else lda
    ldd = H if ldd is None else ldd
    return L.tutel_amd_expert_gemm_w8_glu(None, R * lda if a_se is None else a_se, a_sw, max(R, 1) if a_rpw is None else a_rpw, lda, None,
                                          2 * H * K if w_stride is None else w_stride, None, None, R * ldd if d_se is None else d_se, d_sw,
                                          max(R, 1) if d_rpw is None else d_rpw, ldd, E_loc, R, H, K, dtype, act, row_counts, None, 0, None, None)


def test_header_declares_and_signatures_bind_both_entry_points(L):
    from tutel_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " is not declared"
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == 24 and len(_lib.SIGNATURES[NAMES[0]][1]) == 3
    assert callable(ops.gemm_w8_glu_supported) and callable(ops.expert_gemm_w8_glu)
    assert L.tutel_amd_abi_version() == 1, "the change is additive"


def test_supported_truth_table(L):
    from tutel_amd import _lib, ops
    q = L.tutel_amd_expert_gemm_w8_glu_supported
    for H in (8, 16, 24, 48, 64):
        for K in (32, 64, 96, 192):
            want = H % 16 == 0 and H >= 16 and K % 64 == 0
            for code, dt in ((_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)):
                assert q(code, H, K) == int(want), (H, K)
                assert ops.gemm_w8_glu_supported(dt, H, K) is want, (H, K)
            assert q(_lib.F32, H, K) == 0 and q(-1, H, K) == 0 and q(3, H, K) == 0
            assert ops.gemm_w8_glu_supported(torch.float32, H, K) is False and ops.gemm_w8_glu_supported(torch.float64, H, K) is False
    for H, K in ((0, 64), (-16, 64), (16, 0), (16, -64)):
        assert q(_lib.BF16, H, K) == 0, (H, K)


def test_refusals_name_their_reason_and_enqueue_nothing(L):
    from tutel_amd import _lib
    counts = ctypes.c_void_p(64)   # any non-null address: it is never followed
    for kw, word in ((dict(row_counts=counts), b"row_counts"),
                     (dict(R=8, a_rpw=4, a_sw=1024), b"exchange layouts"), (dict(R=8, d_rpw=4), b"exchange layouts"), (dict(d_sw=64), b"exchange layouts"),
                     (dict(lda=68), b"aligned"), (dict(ldd=18), b"aligned"), (dict(a_se=68), b"aligned"), (dict(d_se=18), b"aligned"),
                     (dict(w_stride=2 * 16 * 64 + 8), b"aligned"),
                     (dict(w_stride=16 * 64), b"image"), (dict(H=32, w_stride=2 * 32 * 64 - 16), b"image"),
                     (dict(K=96), b"K must be a multiple of 64"), (dict(H=24), b"H must be a multiple of 16"), (dict(H=8), b"H must be"),
                     (dict(dtype=_lib.F32), b"bf16 or fp16"), (dict(act=4), b"activation"), (dict(act=-1), b"activation")):
        rc = _call(L, **kw)
        err = L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and b"tutel_amd_expert_gemm_w8_glu: not covered" in err and word in err, (kw, rc, err)
    # covered shape, null operands: an error (not ENOTSUP), still before any HIP call -- this machine may have no GPU at all
    for act in (0, 1, 2, 3):
        rc = _call(L, act=act)
        assert rc not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _call(L, H=0) not in (0, _lib.ENOTSUP) and b"bad sizes" in L.tutel_amd_last_error()
    assert _call(L, E_loc=1 << 20, R=1 << 12) == _lib.ENOTSUP and b"2^31" in L.tutel_amd_last_error()


def test_empty_problem_is_a_no_op(L):
    assert _call(L, E_loc=0, R=16) == 0 and _call(L, E_loc=4, R=0) == 0 and _call(L, E_loc=0, R=0) == 0


# ---- the image --------------------------------------------------------------------------------------------------------------------
def _codes(E, H, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(1, 256, [E, H, K], generator=g, dtype=torch.uint8), torch.randint(1, 256, [E, H, K], generator=g, dtype=torch.uint8))


@pytest.mark.parametrize("H,K", [(16, 64), (48, 64), (128, 192)])
def test_interleave_round_trip(H, K):
    from tutel_amd.experts import w8
    gate, up = _codes(2, H, K, H + K)
    both = w8.interleave_gate_up(gate.view(F8), up.view(F8))
    assert both.dtype == F8 and both.shape == (2, 2 * H, K)
    g2, u2 = w8.deinterleave_gate_up(both)
    assert torch.equal(g2.view(torch.uint8), gate) and torch.equal(u2.view(torch.uint8), up)
    b = both.view(torch.uint8)
    for g in range(H // 16):   # the rule, spelled out: group g = gate channels 16 g .. + 15, then the up channels of the same indices
        assert torch.equal(b[:, 32 * g:32 * g + 16], gate[:, 16 * g:16 * g + 16]) and torch.equal(b[:, 32 * g + 16:32 * g + 32], up[:, 16 * g:16 * g + 16])
    # scales take the same order
    sg, su = torch.rand([2, H]), torch.rand([2, H])
    s = w8.interleave_gate_up(sg, su)
    assert s.shape == (2, 2 * H) and all(torch.equal(t, r) for t, r in zip(w8.deinterleave_gate_up(s), (sg, su)))
    with pytest.raises(AssertionError):
        w8.interleave_gate_up(gate[:, :H - 8].view(F8), up[:, :H - 8].view(F8))   # H % 16 != 0


# (H = 16: one channel group.  The image of a covered H never pads its channels -- 2 H is a multiple of 32 whenever H is one of 16, and
# interleave_gate_up takes nothing else, H = 40 included -- so the pad bytes are shown where they can arise: K = 40, padded to 64)
@pytest.mark.parametrize("H,K", [(16, 64), (48, 40), (32, 96)])
def test_image_closed_form(H, K):
    """byte b of lane l of block (g, t): with p = l & 31, the gate code when p < 16 and the up code otherwise, of channel 16 g + (p & 15),
    at k = 32 t + 16 (b >> 3) + 8 (l >> 5) + (b & 7); 0x00 where k is past K"""
    from tutel_amd.experts import w8
    E = 2
    gate, up = _codes(E, H, K, 3 * H + K)   # no code is 0x00: a pad byte cannot be mistaken for one
    image = w8.pack(w8.interleave_gate_up(gate.view(F8), up.view(F8)))
    Kp = (K + 31) // 32 * 32
    assert image.shape == (E, 2 * H // 32, Kp // 32, 64, 16) and image.dtype == torch.uint8
    for e in range(E):
        for g in range(2 * H // 32):
            for t in range(Kp // 32):
                for l in range(64):
                    p = l & 31
                    src = gate if p < 16 else up
                    n = 16 * g + (p & 15)
                    for b in range(16):
                        k = 32 * t + 16 * (b >> 3) + 8 * (l >> 5) + (b & 7)
                        want = int(src[e, n, k]) if k < K else 0
                        assert int(image[e, g, t, l, b]) == want, (e, g, t, l, b)
    assert int((image == 0).sum()) == E * 2 * H * (Kp - K)
    g2, u2 = w8.deinterleave_gate_up(w8.unpack(image, 2 * H, K))
    assert torch.equal(g2.view(torch.uint8), gate) and torch.equal(u2.view(torch.uint8), up), "unpack drops the pad bytes"


@pytest.mark.parametrize("w_kmajor", [True, False], ids=["kmajor", "nmajor"])
def test_prepare_gate_up_is_prepare_of_each_interleaved(w_kmajor):
    from tutel_amd.experts import w8
    E, H, K = 2, 32, 64
    g = torch.Generator().manual_seed(5)
    shape = [E, H, K] if w_kmajor else [E, K, H]
    wg, wu = torch.randn(shape, generator=g).bfloat16(), (torch.randn(shape, generator=g) * 3).bfloat16()
    image, scale = w8.prepare_gate_up(wg, wu, w_kmajor)
    (ig, sg), (iu, su) = w8.prepare(wg, w_kmajor), w8.prepare(wu, w_kmajor)
    assert image.dtype == torch.uint8 and image.is_contiguous() and image.numel() == E * 2 * H * K
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.shape == (E, 2 * H)
    q = w8.unpack(image, 2 * H, K)
    qg, qu = w8.deinterleave_gate_up(q)
    assert torch.equal(qg.view(torch.uint8), w8.unpack(ig, H, K).view(torch.uint8)) and torch.equal(qu.view(torch.uint8), w8.unpack(iu, H, K).view(torch.uint8))
    assert torch.equal(image, w8.pack(w8.interleave_gate_up(w8.unpack(ig, H, K), w8.unpack(iu, H, K))))
    s1, s2 = w8.deinterleave_gate_up(scale)
    assert torch.equal(s1, sg) and torch.equal(s2, su), "each matrix keeps its own per-channel scales"
    assert not torch.equal(sg, su)


# ---- the layer's predicate --------------------------------------------------------------------------------------------------------
def _net(M=64, H=64, dtype=torch.bfloat16, shards=1):
    from tutel_amd.experts.llama_ffn import LlamaFFNNetwork
    net = LlamaFFNNetwork(M, H, 2, shards).to(dtype).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def test_switch_default_is_the_ffn_experts(monkeypatch):
    from tutel_amd.experts import ffn
    from tutel_amd.experts.llama_ffn import LlamaFFNNetwork
    assert LlamaFFNNetwork(64, 64, 1, 1).fp8_weights is ffn._FP8_WEIGHTS is ffn.FusedExpertsNetwork(64, 32, 1, 1).fp8_weights
    monkeypatch.setattr(ffn, "_FP8_WEIGHTS", True)
    assert LlamaFFNNetwork(64, 64, 1, 1).fp8_weights is True


def test_w8_refusal_admits_then_walks_the_ladder_in_order(L, monkeypatch):
    """the admitted case first; then a state that fails EVERY check is repaired one check at a time and the reason moves down the
    ladder: switch, device, autograd, training mode, autocast, dtype, sharded / adaptive_r = 0, activation, shape, capture"""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    ok = _net()
    ctx = types.SimpleNamespace(sharded_count=1, adaptive_degree=1)
    dev = _CudaLike()
    assert ok.fp8_weights is False and ok.w8_refusal(dev, ctx) == "fp8_weights is off (TUTEL_AMD_FP8_WEIGHTS)"
    ok.fp8_weights = True
    assert ok.w8_refusal(dev, ctx) is None, "the admitted case, so that each exclusion below shows"
    half = _CudaLike()
    half.dtype = torch.float16
    h = _net(dtype=torch.float16)
    h.fp8_weights = True
    assert h.w8_refusal(half, ctx) is None and "dtype" in h.w8_refusal(dev, ctx)
    assert "gathered" in ok.w8_refusal(dev, types.SimpleNamespace(sharded_count=1, adaptive_degree=0))
    sharded = _net(shards=2)
    sharded.fp8_weights = True
    assert "gathered" in sharded.w8_refusal(dev, ctx), "the experts' own shard count"
    for M, H in ((64, 96), (96, 64), (64, 48), (64, 16), (32, 64)):
        narrow = _net(M, H)
        narrow.fp8_weights = True
        assert narrow.w8_refusal(dev, ctx) == "the shape is not covered (M a multiple of 64, H a multiple of 64)", (M, H)

    net = _net(64, 48)   # hidden size 48: fc3's K is no multiple of 64
    x = _CudaLike()
    x.is_cuda, x.dtype = False, torch.float32
    bad = types.SimpleNamespace(sharded_count=2, adaptive_degree=1)
    net.W_fc1.requires_grad_(True)
    net.train()
    net.activation_fn, net._act_cache = (lambda t: t.clamp(0, 6)), {}
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)

    def relu():
        net.activation_fn, net._act_cache = torch.nn.functional.silu, {}

    def resize():
        for name, shape in (("W_fc1", [2, 64, 64]), ("W_fc2", [2, 64, 64]), ("W_fc3", [2, 64, 64])):
            setattr(net, name, torch.nn.Parameter(torch.randn(shape).bfloat16().view(-1), requires_grad=False))
            setattr(net, name + "_full_shape", torch.Size(shape))

    steps = [
        ("fp8_weights is off (TUTEL_AMD_FP8_WEIGHTS)", lambda: setattr(net, "fp8_weights", True)),
        ("the input is not on the HIP device", lambda: setattr(x, "is_cuda", True)),
        ("autograd is live (FP8 weights are inference only)", lambda: net.W_fc1.requires_grad_(False)),
        ("the module is in training mode (FP8 weights are inference only)", lambda: net.eval()),
        ("autocast is on", lambda: monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: False)),
        ("the input is not bf16 / fp16 in the experts' own dtype", lambda: setattr(x, "dtype", torch.bfloat16)),
        ("gathered-weight modes (sharded experts, adaptive_r = 0) are not covered", lambda: setattr(bad, "sharded_count", 1)),
        ("the activation is not one of the fused epilogues", relu),
        ("the shape is not covered (M a multiple of 64, H a multiple of 64)", resize),
        ("the quantised weights are not cached yet: run one eager forward before capturing a graph", lambda: net.w8_params()),
    ]
    with torch.enable_grad():
        for want, repair in steps:
            assert net.w8_refusal(x, bad) == want
            repair()
        assert net.w8_refusal(x, bad) is None
        with torch.no_grad():
            net.W_fc2.mul_(2)   # the version counter moved: the cached gate / up image is stale
        assert "eager forward" in net.w8_refusal(x, bad)


def test_cache_rebuilds_exactly_the_entries_that_depend_on_a_parameter():
    from tutel_amd.experts import w8
    net = _net()
    (igu, sgu), (i3, s3) = net.w8_params()
    again = net.w8_params()
    assert again[0][0] is igu and again[1][0] is i3 and net.w8_cached(), "a hit returns the cached images"
    w1, w2, w3 = (p.view(s) for p, s in ((net.W_fc1, net.W_fc1_full_shape), (net.W_fc2, net.W_fc2_full_shape), (net.W_fc3, net.W_fc3_full_shape)))
    ri, rs = w8.prepare_gate_up(w1, w2, False)
    assert torch.equal(igu, ri) and torch.equal(sgu, rs), "W_fc1 / W_fc2 are read from their [K, N] storage"
    r3, rs3 = w8.prepare(w3, False)
    assert torch.equal(i3, r3) and torch.equal(s3, rs3)
    for name, gate_up_rebuilt in (("W_fc1", True), ("W_fc2", True), ("W_fc3", False)):
        (a, sa), (b, sb) = net.w8_params()
        with torch.no_grad():
            getattr(net, name).mul_(2)   # a power of two moves the scales only
        assert not net.w8_cached()
        (c, sc), (d, sd) = net.w8_params()
        assert (c is not a) is gate_up_rebuilt and (d is not b) is (not gate_up_rebuilt), name
        assert torch.equal(c, a) and torch.equal(d, b)
        half = {"W_fc1": 0, "W_fc2": 1}.get(name)
        if half is None:
            assert torch.equal(sd, sb * 2) and sc is sa
        else:
            old, new = w8.deinterleave_gate_up(sa), w8.deinterleave_gate_up(sc)
            assert torch.equal(new[half], old[half] * 2) and torch.equal(new[1 - half], old[1 - half]), name
    for poke in (lambda: net.train(), lambda: net.eval(), lambda: net.load_state_dict(net.state_dict()), lambda: net.invalidate_prepacked()):
        before = net.w8_params()[0][0]
        poke()
        assert net.w8_params()[0][0] is not before
