"""The fp32 grouped GEMM (csrc/expert_gemm_f32.hip, tutel_amd_expert_gemm_f32) without a GPU: the C ABI declares, exports and binds it,
its coverage query on both sides of every limit, refusals that name their reason before anything is enqueued, the Python switch and
the predicates that keep a forward on ATen, and the CPU replay of the contract (tests/expert_gemm_f32_ref.c) against float64."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("tutel_amd_expert_gemm_f32_supported", "tutel_amd_expert_gemm_f32")


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _call(L, E_loc=1, R=1, N=8, K=32, act=0, lda=None, ldw=None, ldd=None, w_kmajor=1):
    """the entry point with null pointers everywhere: only the argument checks can answer"""
    lda = K if lda is None else lda
    ldw = (K if w_kmajor else N) if ldw is None else ldw
    ldd = N if ldd is None else ldd
    return L.tutel_amd_expert_gemm_f32(None, R * lda, 0, max(R, 1), lda, None, w_kmajor, N * K, ldw, None, 0, None, R * ldd, 0, max(R, 1), ldd,
                                       E_loc, R, N, K, act, None, 0, None, None)


def test_header_declares_and_signatures_bind_both_entry_points(L):
    from tutel_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " is not declared"
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == 25 and len(_lib.SIGNATURES[NAMES[0]][1]) == 2
    assert "fp32/fp64 experts stay on the ATen/rocBLAS bmm" not in open(os.path.join(ROOT, "include", "tutel_amd.h")).read()


def test_supported_query_on_both_sides_of_every_limit(L):
    from tutel_amd import ops
    q = L.tutel_amd_expert_gemm_f32_supported
    cases = {(4, 32): 1, (8, 32): 1, (36, 96): 1, (2048, 2048): 1, (132, 64): 1,
             (0, 32): 0, (2, 32): 0, (6, 32): 0, (7, 32): 0, (-4, 32): 0,              # N: a positive multiple of 4
             (4, 0): 0, (4, 16): 0, (4, 31): 0, (4, 33): 0, (4, 48): 0, (4, -32): 0,   # K: a positive multiple of 32
             (24, 64): 1, (64, 24): 0}                                                 # hidden size 24: fc1's N passes, fc2's K does not
    for (N, K), want in cases.items():
        assert q(N, K) == want, (N, K)
        assert ops.gemm_f32_supported(N, K) is bool(want), (N, K)
    # every fp32 fixture's products
    for N in (32, 64, 128, 2048):
        for K in (32, 64, 128, 2048):
            assert q(N, K) == 1
    # the 16-bit query keeps naming the 16-bit kernels
    assert ops.gemm_supported(torch.float32, 64, 64) is False


def test_refusals_name_their_reason_and_enqueue_nothing(L):
    from tutel_amd import _lib
    for kw, word in ((dict(K=48), b"K must be a multiple of 32"), (dict(K=100), b"K must be"), (dict(N=6), b"N must be a multiple of 4"),
                     (dict(act=4), b"activation"), (dict(act=-1), b"activation"), (dict(lda=33), b"16-byte"), (dict(ldw=34), b"16-byte"),
                     (dict(ldd=9), b"16-byte")):
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
    assert _call(L, E_loc=0, R=16) == 0 and _call(L, E_loc=4, R=0) == 0 and _call(L, E_loc=0, R=0, w_kmajor=0) == 0


def test_the_16_bit_entry_point_still_refuses_fp32(L):
    from tutel_amd import _lib
    rc = L.tutel_amd_expert_gemm(None, 0, 0, 1, 0, None, 1, 0, 0, None, 0, None, 0, 0, 1, 0, 1, 1, 8, 64, _lib.F32, 0, None, 1, None)
    assert rc != 0 and b"bf16 or fp16" in L.tutel_amd_last_error()


def test_switch_is_off_unless_the_environment_asks():
    code = "from tutel_amd.experts import ffn; print(int(ffn._NATIVE_FP32))"
    for value, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "TUTEL_AMD_NATIVE_FP32"}
        if value is not None:
            env["TUTEL_AMD_NATIVE_FP32"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


class _CudaLike:
    """stands in for a device tensor where only dtype / device flags are looked at (this machine has no GPU)"""
    is_cuda, dtype, requires_grad = True, torch.float32, False


def test_can_fuse_f32_is_false_for_cpu_tensors_and_every_excluded_case(L, monkeypatch):
    from tutel_amd.experts import ffn
    net = ffn.FusedExpertsNetwork(64, 32, 2, 1)
    for p in net.parameters():
        p.requires_grad_(False)
    ctx = types.SimpleNamespace(sharded_count=1, adaptive_degree=1, megablocks_size=0)
    x = torch.zeros([2, 4, 64])
    assert not ffn._NATIVE_FP32 and net.can_fuse_f32(x, ctx) is False and "off" in net.f32_refusal(x, ctx)
    monkeypatch.setattr(ffn, "_NATIVE_FP32", True)
    assert net.can_fuse_f32(x, ctx) is False and "device" in net.f32_refusal(x, ctx), "a CPU tensor"
    dev = _CudaLike()
    assert net.f32_refusal(dev, ctx) is None and net.can_fuse_f32(dev, ctx) is True, "the admitted case, so that each exclusion below shows"
    # each excluded case
    for field, value, word in (("sharded_count", 2, "gathered"), ("adaptive_degree", 0, "gathered"), ("megablocks_size", 4, "megablocks")):
        bad = types.SimpleNamespace(**{**vars(ctx), field: value})
        assert net.can_fuse_f32(dev, bad) is False and word in net.f32_refusal(dev, bad), field
    half = _CudaLike()
    half.dtype = torch.bfloat16
    assert net.can_fuse_f32(half, ctx) is False and "fp32" in net.f32_refusal(half, ctx)
    net.skip_expert = True
    assert net.can_fuse_f32(dev, ctx) is False
    net.skip_expert = False
    with monkeypatch.context() as m:   # (the device's autocast state: nothing can switch it on without the device)
        m.setattr(torch, "is_autocast_enabled", lambda *a: True)
        assert net.can_fuse_f32(dev, ctx) is False and "autocast" in net.f32_refusal(dev, ctx)
    net.batched_fc1_w.requires_grad_(True)
    assert net.can_fuse_f32(dev, ctx) is False and "autograd" in net.f32_refusal(dev, ctx)
    with torch.no_grad():
        assert net.can_fuse_f32(dev, ctx) is True
    net.batched_fc1_w.requires_grad_(False)
    net.activation_fn, net._act_cache = (lambda t: t.clamp(0, 6)), {}
    assert net.can_fuse_f32(dev, ctx) is False and "activation" in net.f32_refusal(dev, ctx)
    narrow = ffn.FusedExpertsNetwork(64, 24, 2, 1)   # hidden size 24: fc2's K is no multiple of 32
    for p in narrow.parameters():
        p.requires_grad_(False)
    assert narrow.can_fuse_f32(dev, ctx) is False and "shape" in narrow.f32_refusal(dev, ctx)
    dbl = ffn.FusedExpertsNetwork(64, 32, 2, 1).double()
    for p in dbl.parameters():
        p.requires_grad_(False)
    assert dbl.can_fuse_f32(dev, ctx) is False and "fp32" in dbl.f32_refusal(dev, ctx)


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    so = tmp_path_factory.mktemp("expert_gemm_f32_ref") / "expert_gemm_f32_ref.so"
    r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "expert_gemm_f32_ref.c"), "-o", str(so), "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fn = ctypes.CDLL(str(so)).expert_gemm_f32_chain
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p]

    def run(a, w, bias, w_kmajor, act):
        a, w = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(w, dtype=np.float32)
        E, R, K = a.shape
        N = w.shape[1] if w_kmajor else w.shape[2]
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        out = np.empty([E, R, N], dtype=np.float32)
        fn(a.ctypes.data, w.ctypes.data, None if b is None else b.ctypes.data, E, R, N, K, int(w_kmajor), int(act), out.ctypes.data)
        return out
    return run


@pytest.mark.parametrize("K", [32, 96, 2048])
@pytest.mark.parametrize("w_kmajor", [1, 0])
def test_reference_chain_against_float64(chain, K, w_kmajor):
    """|chain - exact| <= K * 2^-24 * sum |a w|: the standard forward bound of a length-K fp32 recurrence (one rounding of relative size
    2^-24 per step, K steps); x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), seeded"""
    g = np.random.default_rng(1000 + K + w_kmajor)
    E, R, N = 2, 5, 12
    a = g.standard_normal([E, R, K]).astype(np.float32)
    w = (g.standard_normal([E, N, K] if w_kmajor else [E, K, N]) / np.sqrt(K)).astype(np.float32)
    bias = g.standard_normal([E, N]).astype(np.float32)
    wt = w.astype(np.float64) if not w_kmajor else w.astype(np.float64).transpose(0, 2, 1)   # [E, K, N]
    exact = np.einsum("erk,ekn->ern", a.astype(np.float64), wt)
    mass = np.einsum("erk,ekn->ern", np.abs(a.astype(np.float64)), np.abs(wt))
    got = chain(a, w, None, w_kmajor, 0)
    assert np.all(np.abs(got.astype(np.float64) - exact) <= K * 2.0 ** -24 * mass)
    assert float(np.abs(got).max()) > 0.5
    # bias: ONE fp32 add on the chain; relu on that
    with_bias = chain(a, w, bias, w_kmajor, 0)
    assert np.array_equal(with_bias, got + bias[:, None, :])
    assert np.array_equal(chain(a, w, bias, w_kmajor, 1), np.maximum(with_bias, np.float32(0)))
    # and the chain is an ORDER: the same sum taken descending differs somewhere at this length
    if K >= 96:
        flipped = chain(a[:, :, ::-1], w[:, :, ::-1] if w_kmajor else w[:, ::-1, :], None, w_kmajor, 0)
        assert not np.array_equal(flipped, got)
