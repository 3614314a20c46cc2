"""The HIP quantiser of the FP8 expert weights (csrc/quantize_w8.hip, tutel_amd_quantize_w8) and fp8_freeze() without a GPU: the C ABI
declares, exports and binds both entry points, the coverage query on both sides of every limit, refusals that name their reason
before anything is enqueued, the channel map against w8.interleave_gate_up's order, and fp8_freeze() refusing a module that is not
on the device or in training mode, with the ladder's reason and the module untouched."""
import ctypes
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("tutel_amd_quantize_w8_supported", "tutel_amd_quantize_w8")


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _call(L, E=1, N=64, K=64, dtype=None, kmajor=1, ldw=None, w_stride=None, wq_stride=None, scale_stride=None, C=None, group=None,
          group_stride=None, group_offset=0, W=None, Wq=None, scale=None, status=None):
    """the entry point with null pointers unless given: only the argument checks can answer"""
    from tutel_amd import _lib
    dtype = _lib.BF16 if dtype is None else dtype
    C = N if C is None else C
    group = N if group is None else group
    group_stride = group if group_stride is None else group_stride
    ldw = (K if kmajor else N) if ldw is None else ldw
    w_stride = N * K if w_stride is None else w_stride
    return L.tutel_amd_quantize_w8(W, dtype, kmajor, w_stride, ldw, E, N, K, Wq, C * K if wq_stride is None else wq_stride, scale,
                                   C if scale_stride is None else scale_stride, C, group, group_stride, group_offset, status, None)


def test_header_declares_library_exports_and_signatures_bind_both_names(L):
    from tutel_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " is not declared"
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 7 and len(_lib.SIGNATURES[NAMES[1]][1]) == 18


def test_supported_query_on_both_sides_of_every_limit(L):
    from tutel_amd import _lib, ops
    q = L.tutel_amd_quantize_w8_supported
    BF = _lib.BF16
    plain = lambda N, K: q(BF, N, K, N, N, N, 0)   # noqa: E731
    for code in (_lib.BF16, _lib.F16, _lib.F32):                     # the dtype: one of the three
        assert q(code, 64, 96, 64, 64, 64, 0) == 1
    for code in (-1, 3, 7):
        assert q(code, 64, 96, 64, 64, 64, 0) == 0
    for K, want in ((32, 1), (64, 1), (96, 1), (2048, 1), (0, 0), (16, 0), (31, 0), (33, 0), (48, 0), (-32, 0)):   # K % 32 == 0
        assert plain(64, K) == want, K
    for C, want in ((64, 1), (96, 1), (128, 1), (80, 0), (65, 0)):   # image_channels % 32 == 0 (N = 64 channels mapped plainly into it)
        assert q(BF, 64, 64, C, 64, 64, 0) == want, C
    assert q(BF, 48, 64, 48, 48, 48, 0) == 0 and q(BF, 16, 64, 16, 16, 16, 0) == 0 and q(BF, 16, 64, 32, 16, 16, 0) == 1
    for g, want in ((16, 1), (32, 1), (64, 1), (8, 0), (24, 0), (0, 0), (-16, 0)):   # group % 16 == 0
        assert q(BF, 64, 64, 256, g, max(g, 16), 0) == want, g
    for N, want in ((32, 1), (64, 1), (96, 1), (48, 0), (16, 0), (0, 0)):    # N % group == 0 (group = 32)
        assert q(BF, N, 64, 128, 32, 32, 0) == want, N
    for go, gs, want in ((0, 32, 1), (16, 32, 1), (17, 32, 0), (32, 32, 0), (0, 16, 1), (1, 16, 0), (-16, 32, 0), (16, 48, 1)):   # offset + group <= stride
        assert q(BF, 64, 64, 256, 16, gs, go) == want, (go, gs)
    for C, want in ((128, 1), (160, 1), (96, 0), (64, 0)):           # (N / group) * group_stride <= image_channels: 4 * 32 = 128
        assert q(BF, 64, 64, C, 16, 32, 0) == want, C
    # the two maps the experts use, through the wrapper
    from tutel_amd.experts import w8
    for H in (16, 48, 64, 2048):
        assert ops.quantize_w8_supported(torch.bfloat16, H, 64, w8.glu_channel_map(H, False))
        assert ops.quantize_w8_supported(torch.float16, H, 64, w8.glu_channel_map(H, True))
    assert ops.quantize_w8_supported(torch.float32, 64, 96) and not ops.quantize_w8_supported(torch.float64, 64, 96)
    assert not ops.quantize_w8_supported(torch.bfloat16, 40, 64) and not ops.quantize_w8_supported(torch.bfloat16, 64, 40)


def test_refusals_name_their_reason_with_null_operands_and_enqueue_nothing(L):
    from tutel_amd import _lib
    for kw, word in ((dict(K=48), b"K must be a multiple of 32"), (dict(dtype=7), b"bf16, fp16 or fp32"), (dict(N=40), b"image_channels"),
                     (dict(N=64, C=128, group=24), b"group must be a multiple of 16"), (dict(N=48, C=64, group=32), b"N must be a multiple of group"),
                     (dict(C=256, group=16, group_stride=32, group_offset=17), b"fit its stride"),
                     (dict(C=96, group=16, group_stride=32), b"leaves the image"),
                     (dict(ldw=56), b"ldw is smaller"), (dict(kmajor=0, N=64, K=96, ldw=56), b"ldw is smaller"),      # ldw fits the layout
                     (dict(ldw=72, w_stride=64 * 64), b"w_stride_e is smaller"),
                     (dict(ldw=68, w_stride=64 * 68), b"16-byte aligned"), (dict(w_stride=64 * 64 + 4), b"16-byte aligned"),
                     (dict(dtype=_lib.F32, ldw=66, w_stride=64 * 66), b"16-byte aligned"),
                     (dict(wq_stride=64 * 64 + 8), b"wq_stride_e % 16"), (dict(wq_stride=64 * 64 - 16), b"wq_stride_e is smaller"),
                     (dict(scale_stride=32), b"scale_stride_e"),
                     (dict(E=1 << 20, N=1 << 11, C=1 << 11, K=32), b"2^31")):
        rc = _call(L, **kw)
        err = L.tutel_amd_last_error()
        assert rc == _lib.ENOTSUP and b"not covered" in err and word in err, (kw, rc, err)
    # just inside: fp32 rows of 68 elements are 16-byte aligned, bf16 rows of 72 are
    for kw in (dict(dtype=_lib.F32, ldw=68, w_stride=64 * 68), dict(ldw=72, w_stride=64 * 72), dict(wq_stride=64 * 64 + 16)):
        assert _call(L, **kw) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error(), kw
    # a covered call with null operands: an error (not ENOTSUP), still in front of any HIP call -- this machine may have no GPU
    assert _call(L) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()
    assert _call(L, N=0) not in (0, _lib.ENOTSUP) and b"bad sizes" in L.tutel_amd_last_error()
    # W and Wq aligned for 16-byte access: any non-null address, never followed
    ok, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    for kw in (dict(W=odd, Wq=ok, scale=ok, status=ok), dict(W=ok, Wq=odd, scale=ok, status=ok)):
        assert _call(L, **kw) == _lib.ENOTSUP and b"16-byte aligned" in L.tutel_amd_last_error(), kw
    # the image and the scales go together (neither: the finiteness check alone)
    assert _call(L, W=ok, Wq=ok, status=ok) not in (0, _lib.ENOTSUP) and b"null pointer" in L.tutel_amd_last_error()


def test_no_experts_is_a_no_op(L):
    assert _call(L, E=0) == 0


@pytest.mark.parametrize("H", [16, 48, 64])
def test_channel_map_is_interleave_gate_up(H):
    """c(n) = (n / group) * group_stride + group_offset + n % group with the gate's and the up's constants, written out here, is the
    order of w8.interleave_gate_up; the plain map is the identity"""
    from tutel_amd.experts import w8

    def c(n, image_channels, group, group_stride, group_offset):
        return (n // group) * group_stride + group_offset + n % group

    gate = torch.arange(H, dtype=torch.float32).view(1, H)
    up = 1000 + torch.arange(H, dtype=torch.float32).view(1, H)
    both = w8.interleave_gate_up(gate, up)[0]
    assert w8.glu_channel_map(H, False) == (2 * H, 16, 32, 0) and w8.glu_channel_map(H, True) == (2 * H, 16, 32, 16)
    seen = set()
    for n in range(H):
        cg, cu = c(n, *w8.glu_channel_map(H, False)), c(n, *w8.glu_channel_map(H, True))
        assert float(both[cg]) == n and float(both[cu]) == 1000 + n, n
        seen |= {cg, cu}
    assert seen == set(range(2 * H)), "every image channel belongs to exactly one source channel"
    assert all(c(n, H, H, H, 0) == n for n in range(H))


def test_native_prepare_on_a_cpu_tensor_is_the_torch_quantiser(L):
    from tutel_amd.experts import w8
    g = torch.Generator().manual_seed(4)
    w = torch.randn([2, 64, 96], generator=g).bfloat16()
    for kmajor in (True, False):
        a, b = w8.prepare_native(w, kmajor), w8.prepare(w, kmajor)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].dtype == torch.uint8
    gate, up = torch.randn([2, 64, 48], generator=g).half(), torch.randn([2, 64, 48], generator=g).half()
    a, b = w8.prepare_gate_up_native(gate, up, False), w8.prepare_gate_up(gate, up, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _modules():
    from tutel_amd.experts import ffn, llama_ffn
    return [("ffn", lambda: ffn.FusedExpertsNetwork(64, 64, 2, 1).bfloat16()), ("llama_ffn", lambda: llama_ffn.LlamaFFNNetwork(64, 64, 2, 1).bfloat16())]


@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
@pytest.mark.parametrize("case", ["cpu", "training"])
def test_fp8_freeze_refuses_with_the_ladders_reason_and_leaves_the_module_untouched(L, monkeypatch, kind, case):
    from tutel_amd.experts import fp8_resident
    mod = dict(_modules())[kind]()
    if case == "cpu":
        mod.eval()
        word = "not on the HIP device"
    else:
        # a training-mode module that IS on the device, as far as the ladder can tell (this machine may have no GPU): the stand-in
        # the static rungs look at says so, everything else is the module's own
        mod.train()
        real = fp8_resident.static_stand_ins

        def on_device(w, *a):
            x, ctx = real(w, *a)
            x.is_cuda = True
            return x, ctx
        monkeypatch.setattr(fp8_resident, "static_stand_ins", on_device)
        word = "training mode"
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    n_params = len(list(mod.parameters()))
    with pytest.raises(ValueError, match=word):
        mod.fp8_freeze()
    after = mod.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert mod.fp8_frozen is False and not any("_w8" in k for k in after) and len(list(mod.parameters())) == n_params
    assert word in mod._fp8_static_refusal()
    if case == "training":   # the same module in eval mode passes every static rung: the reason above was the training rung's alone
        mod.eval()
        assert mod._fp8_static_refusal() is None
