"""FP8 activations (W8A8) without a GPU: the order of the new ladders, the engine order, and the entry points' pure coverage queries."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_expert_gemm_w4_cpu import BF16, _CudaLike, _walk  # noqa: E402

SWITCH = ("fp8_activations is off (TUTEL_AMD_FP8_ACTIVATIONS)", "fp8_activations applies on top of fp8_weights or an FP8-resident module")
TAIL = ("the shape is not covered by the W8A8 kernels (M and H multiples of 64, at most 8192)",
        "the quantised weights are not cached yet: run one eager forward before capturing a graph")


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def test_coverage_queries(L):
    from tutel_amd import _lib
    assert L.tutel_amd_expert_gemm_w8a8_supported(_lib.BF16, 32, 64) == 1 and L.tutel_amd_expert_gemm_w8a8_glu_supported(_lib.F16, 16, 64) == 1
    for dtype, N, K in ((_lib.F32, 32, 64), (_lib.BF16, 48, 64), (_lib.BF16, 32, 96)):
        assert L.tutel_amd_expert_gemm_w8a8_supported(dtype, N, K) == 0
    assert L.tutel_amd_expert_gemm_w8a8_glu_supported(_lib.BF16, 24, 64) == 0
    assert [L.tutel_amd_quantize_rows_a8_supported(_lib.BF16, K) for K in (64, 96, 8192, 8256)] == [1, 0, 1, 0]
    assert L.tutel_amd_quantize_rows_a8_supported(_lib.F32, 64) == 0


@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_fp8_activations_ladder_order(L, monkeypatch, kind):
    """a state that fails EVERY check at once is repaired one check at a time: the switch's two rungs, the W8 ladder's own from its
    second rung on (asked through w8_refusal with its switch on: the same reasons in the same order), the W8A8 shape, the capture"""
    from tutel_amd.experts import ffn, llama_ffn
    assert ffn.ENGINES[:2] == (ffn.W8A8, ffn.W8) and ffn.W8A8.ladder[2:-2] == ffn.W8.ladder[1:-1] and ffn.W8A8.ran == "_fp8_activations_ran"
    assert llama_ffn.A8_LADDER[2:-2] == llama_ffn.W8_LADDER[1:-1]
    big = 64 * 129   # 8256: a multiple of 64 the W8A16 kernels take and the row quantiser does not
    if kind == "ffn":
        net = ffn.FusedExpertsNetwork(64, big, 1, 1).to(BF16).eval()
        refusal = lambda: net.engine_refusal(ffn.W8A8, x, ctx)   # noqa: E731
        shrink = lambda: [setattr(net, n, torch.nn.Parameter(torch.zeros(s, dtype=BF16), requires_grad=False))   # noqa: E731
                          for n, s in (("batched_fc1_w", [1, 64, 64]), ("batched_fc2_w", [1, 64, 64]))]
    else:
        net = llama_ffn.LlamaFFNNetwork(64, big, 1, 1).to(BF16).eval()
        refusal = lambda: net.w8a8_refusal(x, ctx)   # noqa: E731
        shrink = lambda: [setattr(net, n, torch.Size(s)) for n, s in (("W_fc1_full_shape", [1, 64, 64]), ("W_fc3_full_shape", [1, 64, 64]))]   # noqa: E731
    for p in net.parameters():
        p.requires_grad_(False)
    x, ctx = _CudaLike(), types.SimpleNamespace(sharded_count=1, adaptive_degree=1, megablocks_size=0)
    x.is_cuda = False
    net.fp8_activations, net.fp8_weights = False, False
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(net, "w8_cached", lambda: False, raising=False)
    cached = lambda: (monkeypatch.setattr(net, "w8_cached", lambda: True, raising=False),   # noqa: E731
                      monkeypatch.setattr(net._kmajor, "holds", lambda *a: True))
    _walk(refusal, [
        (SWITCH[0], lambda: setattr(net, "fp8_activations", True)),
        (SWITCH[1], lambda: setattr(net, "fp8_weights", True)),
        ("the input is not on the HIP device", lambda: setattr(x, "is_cuda", True)),   # (the W8 ladder's own order: its own tests)
        (TAIL[0], shrink),
        (TAIL[1], cached),
    ])
    net.fp8_weights, net.fp8_frozen = False, True
    assert refusal() is None, "an FP8-resident module counts as FP8 weights"


def test_committed_resource_summary_shows_no_scratch_and_two_workgroups_per_cu():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "expert_gemm_w8a8_kernel_resources.txt")
    rows = [line.split() for line in open(path) if not line.startswith("#")]
    assert len(rows) == 16, "bf16 / fp16 x four activations x plain / gate-up"
    for name, vgprs, agprs, scratch, occupancy, lds in rows:
        assert "expert_gemm_w8a8_kernel" in name and int(scratch) == 0 and int(occupancy) >= 2 and int(lds) == 16384, name
