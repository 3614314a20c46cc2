"""W4A8 without a GPU: the new ladders' order and texts, the engines' trial order, the coverage queries, the ops wrappers' first check."""
import types

import pytest
import torch
from test_expert_gemm_w4_cpu import BF16, L, _CudaLike, _walk  # noqa: F401 (L: the built library, a fixture)


def test_trial_order_puts_w4a8_in_front_of_w4_and_keeps_the_engine_list():
    from tutel_amd.experts import ffn
    assert ffn.ENGINES[:2] == (ffn.W8A8, ffn.W8) and ffn.ENGINES.index(ffn.W4) == ffn.ENGINES.index(ffn.W8) + 1
    assert set(ffn.TRIAL) == set(ffn.ENGINES) and ffn.TRIAL.index(ffn.W4A8) + 1 == ffn.TRIAL.index(ffn.W4) and ffn.TRIAL[:2] == ffn.ENGINES[:2]
    assert ffn.W4A8.ran == "_w4a8_ran" and ffn.W4A8.entry == "tutel_amd_expert_gemm_w4a8"


@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_w4a8_ladder_order(L, monkeypatch, kind):
    """repaired one check at a time: the switch's two rungs, the W4 ladder's own from its second rung on, the W4A8 shape, the capture"""
    from tutel_amd.experts import ffn, llama_ffn
    assert ffn.W4A8.ladder[2:-2] == ffn.W4.ladder[1:-1] and llama_ffn.W4A8_LADDER[2:-2] == llama_ffn.W4_LADDER[1:-1]
    big = 64 * 129   # 8256: a multiple of 64 the W4A16 kernels take and the row quantiser does not
    if kind == "ffn":
        net = ffn.FusedExpertsNetwork(64, big, 1, 1).to(BF16).eval()
        refusal = lambda: net.engine_refusal(ffn.W4A8, x, ctx)   # noqa: E731
        shrink = lambda: [setattr(net, n, torch.nn.Parameter(torch.zeros(s, dtype=BF16), requires_grad=False))   # noqa: E731
                          for n, s in (("batched_fc1_w", [1, 64, 64]), ("batched_fc2_w", [1, 64, 64]))]
    else:
        net = llama_ffn.LlamaFFNNetwork(64, big, 1, 1).to(BF16).eval()
        refusal = lambda: net.w4a8_refusal(x, ctx)   # noqa: E731
        shrink = lambda: [setattr(net, n, torch.Size(s)) for n, s in (("W_fc1_full_shape", [1, 64, 64]), ("W_fc3_full_shape", [1, 64, 64]))]   # noqa: E731
    net.requires_grad_(False)
    x, ctx = _CudaLike(), types.SimpleNamespace(sharded_count=1, adaptive_degree=1, megablocks_size=0)
    x.is_cuda = False
    assert net.w4a8 is False and net.fp4_weights is False, "off by default"
    net.fp8_weights = True
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(net, "w4_cached", lambda: False, raising=False)
    cached = lambda: (monkeypatch.setattr(net, "w4_cached", lambda: True, raising=False),   # noqa: E731
                      monkeypatch.setattr(net._kmajor, "holds", lambda *a: True))
    _walk(refusal, [
        ("w4a8 is off (TUTEL_AMD_W4A8)", lambda: setattr(net, "w4a8", True)),
        ("w4a8 applies on top of fp4_weights or an FP4-resident module", lambda: setattr(net, "fp4_weights", True)),
        ("fp8_weights is on as well (one weight format per module)", lambda: setattr(net, "fp8_weights", False)),
        ("the input is not on the HIP device", lambda: setattr(x, "is_cuda", True)),   # (the W4 ladder's own order: its own tests)
        ("the shape is not covered by the W4A8 kernels (M and H multiples of 64, at most 8192)", shrink),
        ("the quantised weights are not cached yet: run one eager forward before capturing a graph", cached),
    ])
    if kind == "ffn":
        assert net.admitted_engine(x, ctx) is ffn.W4A8
        net.w4a8 = False
        assert net.admitted_engine(x, ctx) is ffn.W4
    net.w4a8, net.fp4_weights, net.fp4_frozen = True, False, True
    assert refusal() is None, "an FP4-resident module counts as FP4 weights"


def test_wrappers_refuse_host_tensors_and_answer_the_coverage_queries(L):
    from tutel_amd import _lib, ops
    from tutel_amd.experts import w4
    E, R, N, K = 2, 4, 32, 64
    ci, si = w4.pack(torch.zeros([E, N, K // 2], dtype=torch.uint8), torch.full([E, N, K // 32], 127, dtype=torch.uint8))
    aq, sa = torch.zeros([E, R, K], dtype=torch.uint8), torch.ones([E * R])
    assert ops.gemm_w4a8_supported(torch.float32, N, K) is False and ops.gemm_w4a8_supported(BF16, N, K) is True
    assert ops.gemm_w4a8_glu_supported(BF16, 16, K) is True and ops.gemm_w4a8_glu_supported(BF16, 24, K) is False
    with pytest.raises(_lib.TutelAmdError, match="no CPU fallback"):
        ops.expert_gemm_w4a8(aq, sa, ci, si, None, N, K, BF16)
    with pytest.raises(_lib.TutelAmdError, match="no CPU fallback"):
        ops.expert_gemm_w4a8_glu(aq, sa, ci, si, N // 2, K, BF16)
