"""The fp32 grouped GEMM (csrc/expert_gemm_f32.hip, tutel_amd_expert_gemm_f32) on the MI355X: its output contract (include/tutel_amd.h)
checked bit for bit against the sequential fmaf chain of tests/expert_gemm_f32_ref.c in both weight layouts, the gathered and the strided
row addressing against the contiguous call, guard bands around every operand, the two activations a math library decides against
torch's own on the same pre-activations, and the refusals."""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (E_loc, R, N, K): one element; an odd number of K-tiles, ragged both ways; more than one row and column tile, each with a sliver;
# five column tiles; a long chain; the fixtures' fc1 and fc2 -- all of them on the 64 x 64 tile (fewer 128 x 128 tiles than compute
# units) -- and BIG: 32 x 2 x 5 = 320 tiles of 128 x 128, the other tile size, with a sliver in both directions
BIG = (32, 130, 516, 32)
SHAPES = [(1, 1, 4, 32), (3, 33, 36, 96), (2, 130, 132, 64), (3, 40, 260, 160), (2, 40, 36, 2048), (16, 64, 32, 64), (16, 64, 64, 32), BIG]
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))


def _ops():
    from tutel_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _chain_fn():
    """expert_gemm_f32_chain of tests/expert_gemm_f32_ref.c, built once per process with gcc"""
    so = os.path.join(tempfile.mkdtemp(prefix="expert_gemm_f32_ref"), "expert_gemm_f32_ref.so")
    r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "expert_gemm_f32_ref.c"), "-o", so, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fn = ctypes.CDLL(so).expert_gemm_f32_chain
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    return fn


def _chain_on(a, w, bias, w_kmajor, act):
    """the contract on explicit CPU tensors: a [E, R, K], w, bias | None, act 0 (none) | 1 (relu) -> [E, R, N]"""
    a, w = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (a, w))
    b = None if bias is None else np.ascontiguousarray(bias.numpy(), dtype=np.float32)
    E, R, K = a.shape
    N = w.shape[1] if w_kmajor else w.shape[2]
    out = np.empty([E, R, N], dtype=np.float32)
    _chain_fn()(a.ctypes.data, w.ctypes.data, None if b is None else b.ctypes.data, E, R, N, K, int(w_kmajor), int(act), out.ctypes.data)
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=None)
def _chain(shape, w_kmajor, has_bias, act):
    """the contract on _inputs(shape, w_kmajor): computed once, shared, never modified"""
    a, w, bias = _inputs(shape, w_kmajor)
    return _chain_on(a, w, bias if has_bias else None, w_kmajor, act)


@functools.lru_cache(maxsize=None)
def _inputs(shape, w_kmajor):
    """a ~ N(0, 1), w ~ N(0, 1) / sqrt(K), bias ~ N(0, 1), seeded (CPU tensors; never modified)"""
    E, R, N, K = shape
    g = torch.Generator().manual_seed(7919 * E + 31 * R + N + 3 * K + int(w_kmajor))
    a = torch.randn([E, R, K], generator=g)
    w = torch.randn([E, N, K] if w_kmajor else [E, K, N], generator=g) / K ** 0.5
    return a, w, torch.randn([E, N], generator=g)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    ne = (_bits(got) != _bits(want)).nonzero()
    assert ne.numel() == 0, (f"{what}: {ne.shape[0]} of {got.numel()} elements differ; the first at {tuple(int(v) for v in ne[0])}: "
                             f"{float(got[tuple(ne[0])])!r} against {float(want[tuple(ne[0])])!r}")


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("w_kmajor", [1, 0], ids=["kmajor", "nmajor"])
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_output_is_the_ascending_fmaf_chain_bit_for_bit(shape, w_kmajor, has_bias, act):
    ops = _ops()
    a, w, bias = _inputs(shape, w_kmajor)
    ad, wd, bd = a.cuda(), w.cuda(), (bias.cuda() if has_bias else None)
    assert ops.gemm_f32_supported(shape[2], shape[3])
    out = ops.expert_gemm_f32(ad, wd, bd, w_kmajor, act=act)
    assert out is not None and tuple(out.shape) == shape[:3] and out.dtype == torch.float32
    _same_bits(out, _chain(shape, w_kmajor, has_bias, int(act == "relu")), "kernel against the chain")
    _same_bits(ops.expert_gemm_f32(ad, wd, bd, w_kmajor, act=act), out, "a second run")


def _slot_map(E, R, T, seed):
    """random slots: -1 (no token) on about a quarter of the rows, else any value below 4 T (the kernel takes it modulo T); the first and
    the last row of the map are pad rows, 4 T - 1 occurs"""
    g = torch.Generator().manual_seed(seed)
    smap = torch.randint(0, 4 * T, [E * R], generator=g, dtype=torch.int32)
    smap[torch.rand([E * R], generator=g) < 0.25] = -1
    smap[0] = smap[-1] = -1
    smap[1] = 4 * T - 1
    return smap


def _encode(x, smap, E, R):
    """the materialised fast_encode with unit gates: row (e, r) = x[smap % T], zeros where smap < 0"""
    rows = x[(smap.long() % x.shape[0])]
    rows[smap < 0] = 0
    return rows.view(E, R, x.shape[1]).contiguous()


GATHER = (3, 33, 36, 96)   # (E_loc, R, N, K), T = 50


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("shape", [GATHER, BIG], **_ids)
def test_gather_is_the_bucket_form_on_a_materialised_encode(shape, act):
    ops = _ops()
    E, R, N, K = shape
    T = 50
    _, w, bias = _inputs(shape, 1)
    x = torch.randn([T, K], generator=torch.Generator().manual_seed(5))
    smap = _slot_map(E, R, T, 6)
    assert int((smap < 0).sum()) >= 3 and int(smap.max()) == 4 * T - 1
    xd, wd, bd, sd = x.cuda(), w.cuda(), bias.cuda(), smap.cuda()
    got = ops.expert_gemm_f32(xd, wd, bd, True, act=act, slot_map=sd, R=R)
    want = ops.expert_gemm_f32(_encode(x, smap, E, R).cuda(), wd, bd, True, act=act)
    _same_bits(got, want, "gathered against bucket form")
    pad = (smap < 0).view(E, R)
    act_bias = torch.relu(bias) if act == "relu" else bias
    _same_bits(got.cpu()[pad], act_bias[:, None, :].expand(E, R, N)[pad].contiguous(), "pad rows are act(bias)")


def test_strided_exchange_buffers_against_the_contiguous_call():
    """A and D as raw [W = 2, E_loc = 3, C = 20, *] all-to-all buffers (rows_per_w = C): the bits of the contiguous call on the permuted copy"""
    ops = _ops()
    Wr, E, Cc, N, K = 2, 3, 20, 36, 96
    g = torch.Generator().manual_seed(9)
    recv = torch.randn([Wr, E, Cc, K], generator=g).cuda()
    w1 = (torch.randn([E, N, K], generator=g) / K ** 0.5).cuda()
    bias = torch.randn([E, N], generator=g).cuda()
    for w_kmajor, w in ((1, w1), (0, w1.transpose(1, 2).contiguous())):
        send = torch.full([Wr, E, Cc, N], float("nan"), device="cuda")
        out = ops.expert_gemm_f32(recv, w, bias, w_kmajor, act="relu", R=Wr * Cc, a_layout=(Cc * K, E * Cc * K, Cc, K), out=send,
                                  d_layout=(Cc * N, E * Cc * N, Cc, N))
        assert out.data_ptr() == send.data_ptr()
        want = ops.expert_gemm_f32(recv.permute(1, 0, 2, 3).reshape(E, Wr * Cc, K).contiguous(), w, bias, w_kmajor, act="relu")
        _same_bits(send.permute(1, 0, 2, 3).reshape(E, Wr * Cc, N), want, f"raw exchange layout, w_kmajor={w_kmajor}")


@pytest.mark.parametrize("w_kmajor", [1, 0], ids=["kmajor", "nmajor"])
@pytest.mark.parametrize("gather", [False, True], ids=["buckets", "gather"])
@pytest.mark.parametrize("shape", [GATHER, BIG], **_ids)
def test_guard_bands_stay_untouched(shape, gather, w_kmajor):
    """every operand and a caller-allocated NaN-filled output inside NaN bands: ragged tiles clamp their loads and mask their stores"""
    from _packed_fuzz import moat_intact, moated
    ops = _ops()
    E, R, N, K = shape
    a, w, bias = _inputs(shape, w_kmajor)
    wm, bm = moated(w.cuda()), moated(bias.cuda())
    om = moated(torch.full([E, R, N], float("nan"), device="cuda"))
    checks = [(wm, "w", w), (bm, "bias", bias)]
    if gather:
        T = 50
        x = torch.randn([T, K], generator=torch.Generator().manual_seed(5))
        smap = _slot_map(E, R, T, 6)
        xm, sm = moated(x.cuda()), moated(smap.cuda(), fill=T - 1)
        checks += [(xm, "x", x), (sm, "slot map", smap)]
        out = ops.expert_gemm_f32(xm, wm, bm, w_kmajor, act="relu", slot_map=sm, R=R, out=om, d_layout=(R * N, 0, R, N))
        want = _chain_on(_encode(x, smap, E, R), w, bias, w_kmajor, 1)
    else:
        am = moated(a.cuda())
        checks.append((am, "a", a))
        out = ops.expert_gemm_f32(am, wm, bm, w_kmajor, act="relu", out=om, d_layout=(R * N, 0, R, N))
        want = _chain(shape, w_kmajor, True, 1)
    torch.cuda.synchronize()
    assert out.data_ptr() == om.data_ptr()
    for view, what, orig in checks:
        moat_intact(view, what)
        assert torch.equal(view.cpu(), orig), f"the operand {what} itself"
    moat_intact(om, "out")
    got = om.cpu()
    assert bool(torch.isfinite(got).all()), "a value from a band reached a result, or an output element was left unwritten"
    _same_bits(got, want, "inside guard bands")


@pytest.mark.parametrize("act", ["gelu", "silu"])
def test_gelu_and_silu_against_torch_on_the_kernels_own_pre_activations(act):
    """pre = the kernel's act-none output (pinned to the chain above).  The kernel's activation and torch's fp32 F.gelu / F.silu of the
    same pre on the device, both against the float64 activation of pre, relative to |pre|:
        max_i err_kernel_i / |pre_i|  <=  2 x max_i err_torch_i / |pre_i| + 2^-24
    -- the factor 2 allows for two few-ulp erff / expf implementations of the same formula"""
    ops = _ops()
    shape = (3, 40, 260, 160)
    a, w, bias = _inputs(shape, 1)
    ad, wd, bd = a.cuda(), w.cuda(), bias.cuda()
    pre = ops.expert_gemm_f32(ad, wd, bd, True, act="none")
    got = ops.expert_gemm_f32(ad, wd, bd, True, act=act)
    fn = torch.nn.functional.gelu if act == "gelu" else torch.nn.functional.silu
    yard = fn(pre)
    exact = fn(pre.double())
    mag = pre.double().abs()
    assert float(mag.min()) > 0
    err_kernel = float(((got.double() - exact).abs() / mag).max())
    err_torch = float(((yard.double() - exact).abs() / mag).max())
    print(f"\n{act}: max err / |pre|: kernel {err_kernel:.4e}, torch {err_torch:.4e}")
    assert err_kernel <= 2 * err_torch + 2.0 ** -24, (err_kernel, err_torch)


def test_refusals_leave_the_output_untouched():
    from tutel_amd import _lib
    ops = _ops()
    L = _lib.lib()
    sentinel = 12345.0
    E, R = 2, 8
    for N, K, act, lda in ((8, 48, 0, None), (6, 32, 0, None), (8, 32, 7, None), (8, 32, 0, 33)):
        a = torch.zeros([E, R, 64], device="cuda")
        w = torch.zeros([E, 64, 64], device="cuda")
        out = torch.full([E, R, 64], sentinel, device="cuda")
        ld = K if lda is None else lda
        rc = L.tutel_amd_expert_gemm_f32(a.data_ptr(), R * 64, 0, R, ld, w.data_ptr(), 1, 64 * 64, 64, None, 0, out.data_ptr(), R * 64, 0, R, 64,
                                         E, R, N, K, act, None, 0, None, None)
        assert rc == _lib.ENOTSUP and b"not covered" in L.tutel_amd_last_error(), (N, K, act, lda)
        torch.cuda.synchronize()
        assert bool((out == sentinel).all()), "nothing was enqueued"
    assert not ops.gemm_f32_supported(8, 48) and not ops.gemm_f32_supported(6, 32)
    # through ops: None, output untouched
    a = torch.zeros([E, R, 48], device="cuda")
    w = torch.zeros([E, 8, 48], device="cuda")
    out = torch.full([E, R, 8], sentinel, device="cuda")
    assert ops.expert_gemm_f32(a, w, None, True, out=out, d_layout=(R * 8, 0, R, 8)) is None
    # a misaligned operand is an error, not a launch
    buf = torch.zeros([E * R * 32 + 1], device="cuda")
    rc = L.tutel_amd_expert_gemm_f32(buf.data_ptr() + 4, R * 32, 0, R, 32, w.data_ptr(), 1, 8 * 32, 32, None, 0, out.data_ptr(), R * 8, 0, R, 8,
                                     E, R, 8, 32, 0, None, 0, None, None)
    assert rc not in (0, _lib.ENOTSUP) and b"aligned" in L.tutel_amd_last_error()
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


def test_integration_stub_runs_verbatim():
    """INTEGRATION.md B.3's fp32 stub, extracted from the markdown and executed as written (on B.1's binding): the bits of
    ops.expert_gemm_f32 in both layouts and in the gathered form, None for an uncovered shape"""
    import test_integration_stubs_gpu as TI
    from tutel_amd import _lib
    ops = _ops()
    _lib.lib()
    env = {}
    exec(compile(TI._blocks("B.1")[0].replace("/path/to/libtutel_amd.so", _lib.LIB_PATH), "INTEGRATION.md:B.1", "exec"), env)
    stub = [b for b in TI._blocks("B.3") if "tutel_amd_expert_gemm_f32(" in b]
    assert len(stub) == 1
    exec(compile(stub[0], "INTEGRATION.md:B.3[f32]", "exec"), env)
    gemm = env["_gemm_f32"]
    E, R, N, K = GATHER
    for w_kmajor in (1, 0):
        a, w, bias = (t.cuda() for t in _inputs(GATHER, w_kmajor))
        _same_bits(gemm(a, w, bias, bool(w_kmajor), 1), ops.expert_gemm_f32(a, w, bias, w_kmajor, act="relu"), f"stub, w_kmajor={w_kmajor}")
    _, w, bias = (t.cuda() for t in _inputs(GATHER, 1))
    x = torch.randn([50, K], generator=torch.Generator().manual_seed(5)).cuda()
    smap = _slot_map(E, R, 50, 6).cuda()
    got = gemm(x, w, bias, True, 0, slot_map=smap, R=R, zero_row=torch.zeros([K], device="cuda"))
    _same_bits(got, ops.expert_gemm_f32(x, w, bias, True, slot_map=smap, R=R), "stub, gathered")
    assert gemm(torch.zeros([2, 8, 48], device="cuda"), torch.zeros([2, 8, 48], device="cuda"), None, True, 0) is None
    torch.cuda.synchronize()
