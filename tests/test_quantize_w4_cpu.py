"""tutel_amd_quantize_w4's coverage without a GPU: tutel_amd_quantize_w4_supported accepts and refuses as include/tutel_amd.h says, and
the entry point answers ENOTSUP with the reason for every condition of the call, in front of any HIP call (no device is needed)."""
import pytest
import torch

from tutel_amd import _lib, ops

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.mark.parametrize("dtype, act, N, K, cmap, ok", [
    (BF16, BF16, 64, 128, None, True),
    (F32, F16, 32, 64, None, True),
    (F16, BF16, 48, 192, (96, 16, 32, 16), True),        # a gate / up half of H = 48
    (torch.float64, BF16, 64, 128, None, False),         # dtype
    (BF16, F32, 64, 128, None, False),                   # act_dtype
    (BF16, BF16, 64, 96, None, False),                   # K % 64
    (BF16, BF16, 48, 128, None, False),                  # image_channels % 32 (the plain map: N)
    (BF16, BF16, 64, 128, (64, 8, 8, 0), False),         # group % 16
    (BF16, BF16, 40, 128, (64, 16, 16, 0), False),       # N % group
    (BF16, BF16, 32, 128, (64, 16, 32, 32), False),      # group_offset + group <= group_stride
    (BF16, BF16, 64, 128, (96, 16, 32, 0), False),       # (N / group) * group_stride <= image_channels
], ids=lambda v: str(v).replace("torch.", ""))
def test_supported_is_what_the_header_says(dtype, act, N, K, cmap, ok):
    assert ops.quantize_w4_supported(dtype, N, K, cmap, act) is ok


def _call(L, ldw=128, stride=64 * 128, wq_stride=64 * 64, s_stride=64 * 4, E=1, N=64, K=128, kmajor=1):
    return L.tutel_amd_quantize_w4(None, _lib.BF16, _lib.BF16, kmajor, stride, ldw, E, N, K, None, wq_stride, None, s_stride, N, N, N, 0, None, None)


@pytest.mark.parametrize("kw, reason", [
    (dict(ldw=120), "ldw is smaller"), (dict(kmajor=0, ldw=32), "ldw is smaller"), (dict(stride=64 * 128 - 8), "w_stride_e is smaller"),
    (dict(ldw=132, stride=64 * 132), "16-byte aligned"), (dict(wq_stride=64 * 64 + 8), "wq_stride_e % 16"),
    (dict(wq_stride=64 * 64 - 16), "code image"), (dict(s_stride=64 * 4 + 2), "s_stride_e % 4"), (dict(s_stride=64 * 4 - 4), "scale image"),
    (dict(K=96, ldw=96), "K must be a multiple of 64"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_entry_point_refuses_with_its_reason_before_any_hip_call(kw, reason):
    L = _lib.lib()
    assert _call(L, **kw) == _lib.ENOTSUP
    msg = L.tutel_amd_last_error().decode()
    assert msg.startswith("tutel_amd_quantize_w4: not covered: ") and reason in msg, msg
    assert _call(L, E=0) == 0, "E == 0 is a no-op"
    assert _call(L) not in (0, _lib.ENOTSUP) and "null pointer" in L.tutel_amd_last_error().decode()
