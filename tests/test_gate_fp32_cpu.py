"""The fp32 gate projection inside the native call (an fp32 gate over 16-bit tokens), without a GPU: what the host side hands the
library with the projection in the call (the recorder of tests/test_native_args_cpu.py), when the layer picks it
(MOELayer._native_gate_weight, switch _NATIVE_GATE_FP32), and what the C side refuses before any HIP call (bogus pointers, as
tests/test_gemm_refusals_cpu.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gemm_refusals_cpu as R   # noqa: E402
import test_native_args_cpu as A     # noqa: E402
from test_native_args_cpu import rec  # noqa: E402,F401  (the recorder fixture)

F32, F16, BF16 = 0, 1, 2


def _fp32_gate_layer(kind="ffn"):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": A.K, "capacity_factor": 0.0, "fp32_gate": True},
                              experts={"type": kind, "num_experts_per_device": A.E, "hidden_size_per_expert": A.H}, model_dim=A.M)
    finally:
        torch.set_default_dtype(old)
    assert layer.gates[0].wg.weight.dtype == torch.float32 and next(layer.experts.parameters()).dtype == torch.bfloat16
    return layer.eval()


def _check_call(call, Tn, splits):
    m = call["structs"][0]
    assert m["logits"] is None and m["gate_w"] == "gates.0.wg.weight+0"
    assert m["logits_dtype"] == F32 and m["ep"]["dtype"] == BF16
    assert m["gate_partial_bytes"] == 4 * splits * Tn * A.E and m["gate_partials"] == "ws.gate_partials+0"
    assert m["l_aux"] == "fresh" and m["ep"]["gates"] == "ws.gates+0"
    bufs = call["workspace"]["buffers"]
    assert bufs["gates"][1] == "torch.float32" and bufs["gate_partials"] == [[splits * Tn * A.E], "torch.float32"]


def _forward(layer, route, Tn, seed, rec):   # noqa: F811
    from tutel_amd.impls import ep_native
    gate_w = layer.gates[0].wg.weight
    x, _ = A._inputs(Tn, seed)
    spec = torch.empty([Tn, A.E], dtype=torch.float32, device="meta")
    rec.named = {"x": x, "gates.0.wg.weight": gate_w}
    with torch.no_grad():
        if route == "padded":
            y, l_aux, cnt, used = ep_native.forward_from_logits(layer, x, spec, A.K, 128, 1, True, True, gate_w=gate_w)
            assert layer.last_logits.dtype == torch.float32 and tuple(layer.last_logits.shape) == (Tn, A.E)
        else:
            y, l_aux, cnt, cap = ep_native.forward_packed(layer, x, spec, A.K, True, 0, 1, gate_w=gate_w)
    assert l_aux.dtype == torch.float32 and y.dtype == torch.bfloat16
    call = rec.calls[-1]
    assert call["entry"] == {"padded": "tutel_amd_moe_forward", "packed": "tutel_amd_moe_forward_packed",
                             "packed_glu": "tutel_amd_moe_forward_packed_glu"}[route]
    assert (call["structs"][0]["logits_out"] == "fresh") == (route == "padded")
    return call


@pytest.mark.parametrize("route", ["padded", "packed", "packed_glu"])
def test_forward_names_the_fp32_gate_weight_and_sizes_the_partial_sums(rec, route):   # noqa: F811
    from tutel_amd import ops
    for i, Tn in enumerate((A.T, A.T2)):
        layer = _fp32_gate_layer("llama_ffn" if route == "packed_glu" else "ffn")
        layer._keep_routing = True
        rec.layer = layer
        S = ops.gate_proj_f32w_splits(Tn, A.M, A.E, torch.bfloat16)
        assert S >= 1
        _check_call(_forward(layer, route, Tn, i, rec), Tn, S)
        assert all("torch.float32" in k for k in map(str, layer._ep_workspaces)), "the workspace key carries the logits dtype"
    # a second, smaller batch on the workspace of the first: the partial sums stay where they are, large enough
    S2 = ops.gate_proj_f32w_splits(200, A.M, A.E, torch.bfloat16)
    m = _forward(layer, route, 200, 7, rec)["structs"][0]
    assert m["gate_partials"] == "ws.gate_partials+0" and m["gate_partial_bytes"] >= 4 * S2 * 200 * A.E and m["logits_dtype"] == F32
    assert len(rec.calls) == 3 and "unknown" not in str(rec.calls) and layer._ep_workspace_allocations == 1


class _FakeCudaTokens:
    """what _native_gate_weight asks of the tokens, answered as a [T, M] device tensor would"""

    def __init__(self, T, M, dtype, device, ptr=1 << 20):
        self.shape, self.dtype, self.device, self.is_cuda, self.requires_grad, self._ptr = (T, M), dtype, device, True, False, ptr

    def dim(self):
        return 2

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._ptr


def test_the_layer_picks_the_fp32_projection_only_when_asked_and_covered(monkeypatch):
    from tutel_amd.impls import moe_layer as ML
    pick = ML.MOELayer._native_gate_weight
    layer = _fp32_gate_layer()
    gate = layer.gates[0]
    w = gate.wg.weight.requires_grad_(False)
    x = _FakeCudaTokens(300, A.M, torch.bfloat16, w.device)
    assert ML._NATIVE_GATE_FP32 == (int(os.environ.get("TUTEL_AMD_NATIVE_GATE_FP32", "0")) != 0), "off unless the environment asks for it"
    monkeypatch.setattr(ML, "_NATIVE_GATE_FP32", False)
    assert pick(gate, x) is None
    monkeypatch.setattr(ML, "_NATIVE_GATE_FP32", True)
    assert pick(gate, x) is w
    assert pick(gate, _FakeCudaTokens(300, A.M, torch.float16, w.device)) is w
    assert pick(gate, _FakeCudaTokens(300, A.M, torch.float32, w.device)) is None          # fp32 tokens: F.linear
    assert pick(gate, _FakeCudaTokens(300, A.M + 8, torch.bfloat16, w.device)) is None      # M % 64
    assert pick(gate, _FakeCudaTokens(300, A.M, torch.bfloat16, w.device, ptr=(1 << 20) + 8)) is None
    assert pick(gate, _FakeCudaTokens(300, A.M, torch.bfloat16, torch.device("meta"))) is None
    w.requires_grad_(True)
    assert pick(gate, x) is None
    with torch.no_grad():
        assert pick(gate, x) is w
    w.requires_grad_(False)
    h = gate.register_forward_hook(lambda *a: None)
    assert pick(gate, x) is None
    h.remove()
    assert pick(gate, x) is w
    gate.bfloat16()                                                                         # cast as a whole: widened per call
    assert pick(gate, x) is None
    # the 16-bit gate's rule is what it was, with the switch on or off
    plain = A._layer()
    wp = plain.gates[0].wg.weight.requires_grad_(False)
    assert pick(plain.gates[0], _FakeCudaTokens(300, A.M, torch.bfloat16, wp.device)) is wp
    assert pick(plain.gates[0], _FakeCudaTokens(300, A.M, torch.float16, wp.device)) is None


def _call(L, case):
    name, args = case
    rc = getattr(L, name)(*args)
    return rc, L.tutel_amd_last_error().decode()


MIXED = dict(logits=None, gate_w=R.Q[17], logits_dtype=F32)   # fp32 gate over the bf16 tokens of R.ep_args
WIDE = dict(T=4096, M=2048, num_experts=64)                   # a shape at which the two kernels split differently


def test_mixed_project_call_refusals():
    from tutel_amd import _lib
    _lib.build()
    L = _lib.lib()
    for shape in (R.BIG, WIDE):
        T, M, E = shape["T"], shape["M"], shape["num_experts"]
        S = L.tutel_amd_gate_proj_f32w_splits(T, M, E, BF16)
        assert S >= 1
        want = "gate_partials must hold %d x %d x %d floats" % (S, T, E)
        assert _call(L, R.moe(shape, **MIXED)) == (-1, "tutel_amd_moe_forward: " + want)
        assert _call(L, R.packed_fwd(shape, **MIXED)) == (-1, "tutel_amd_moe_forward_packed: " + want)
        assert _call(L, R.packed_fwd(shape, w_up=R.Q[33], **MIXED)) == (-1, "tutel_amd_moe_forward_packed: " + want)
        # one float short is still refused
        short = dict(MIXED, gate_partials=R.Q[19], gate_partial_bytes=4 * S * T * E - 4)
        assert _call(L, R.moe(shape, **short)) == (-1, "tutel_amd_moe_forward: " + want)
    assert L.tutel_amd_gate_proj_f32w_splits(4096, 2048, 64, BF16) != L.tutel_amd_gate_proj_splits(4096, 2048, 64, BF16), \
        "WIDE is there to tell the two queries apart"
    # a shape the kernel does not cover (E % 4 != 0)
    six = dict(T=256, M=2048, num_experts=6)
    assert _call(L, R.moe(six, **MIXED)) == (-1, "tutel_amd_moe_forward: the in-call gate projection does not cover T=256, M=2048, E=6, dtype=2 "
                                                "(pass logits)")
    assert _call(L, R.packed_fwd(six, **MIXED)) == (-1, "tutel_amd_moe_forward_packed: the in-call gate projection does not cover T=256, M=2048, "
                                                       "E=6 (pass logits)")
    # every other mismatch keeps its refusal: a 16-bit gate in the other 16-bit dtype, fp32 tokens under an fp32 gate's weight
    assert _call(L, R.moe(logits_dtype=F16, **R.PROJECT))[1].endswith("needs the gate in the token dtype (1 vs 2)")
    assert "needs the gate in the token dtype" in _call(L, R.packed_fwd(logits_dtype=F16, **R.PROJECT))[1]


def test_entry_point_argument_checks():
    """tutel_amd_gate_proj_f32w carries the checks of tutel_amd_gate_proj; tutel_amd_gate_topk_partials takes TUTEL_F32"""
    from tutel_amd import _lib
    _lib.build()
    L = _lib.lib()
    Q = R.Q
    assert L.tutel_amd_gate_proj_f32w_splits(128, 2048, 64, F32) == 0 and L.tutel_amd_gate_proj_splits(128, 2048, 64, F32) == 0
    for T, M, E in [(128, 2048, 256), (128, 2040, 64), (128, 2048, 6), (0, 2048, 64)]:
        assert L.tutel_amd_gate_proj_f32w_splits(T, M, E, BF16) == 0
    for T, M, E in [(1, 64, 4), (4096, 2048, 64), (257, 2048, 128), (64, 1 << 20, 128)]:
        for dt in (BF16, F16):
            assert 1 <= L.tutel_amd_gate_proj_f32w_splits(T, M, E, dt) <= 64
    assert L.tutel_amd_gate_proj_f32w(Q[0], Q[1], BF16, 128, 2048, 6, Q[2], 1 << 30, None) == _lib.ENOTSUP
    assert b"tutel_amd_gate_proj_f32w: shape not covered" in L.tutel_amd_last_error()
    assert L.tutel_amd_gate_proj_f32w(Q[0], Q[1], F32, 128, 2048, 64, Q[2], 1 << 30, None) == _lib.ENOTSUP
    assert L.tutel_amd_gate_proj_f32w(None, None, BF16, 0, 2048, 64, None, 0, None) == 0
    assert L.tutel_amd_gate_proj_f32w(Q[0], None, BF16, 128, 2048, 64, Q[2], 1 << 30, None) == -1
    assert L.tutel_amd_last_error() == b"tutel_amd_gate_proj_f32w: null pointer"
    assert L.tutel_amd_gate_proj_f32w(Q[0], Q[1] + 8, BF16, 128, 2048, 64, Q[2], 1 << 30, None) == -1
    assert L.tutel_amd_last_error() == b"tutel_amd_gate_proj_f32w: x, wg and partials must be 16-byte aligned"
    S = L.tutel_amd_gate_proj_f32w_splits(128, 2048, 64, BF16)
    assert L.tutel_amd_gate_proj_f32w(Q[0], Q[1], BF16, 128, 2048, 64, Q[2], 4 * S * 128 * 64 - 1, None) == -1
    assert b"partials buffer too small" in L.tutel_amd_last_error()
    # the consumer: fp32 passes the dtype check (and fails the next one it is handed here); fp64 does not
    assert L.tutel_amd_gate_topk_partials(Q[0], 65, F32, 128, 64, 2, 1, None, None, Q[1], Q[2], Q[3], 1 << 20, None, 0, None) == -1
    assert L.tutel_amd_last_error() == b"tutel_amd_gate_topk_partials: bad split count 65"
    assert L.tutel_amd_gate_topk_partials(Q[0], 4, 3, 128, 64, 2, 1, None, None, Q[1], Q[2], Q[3], 1 << 20, None, 0, None) == -1
    assert b"the logits dtype must be" in L.tutel_amd_last_error()


def test_split_ranges_follow_the_header():
    """ops.gate_proj_f32w_ranges: S contiguous ascending ranges of whole 64-wide panels, L = 64 * ceil(M / 64 / S), none empty"""
    from tutel_amd import ops
    for T in (1, 64, 300, 4096, 20000):
        for M in (64, 192, 256, 1024, 2048, 4096, 8192, 64 * 129, 1 << 17):
            for E in (4, 64, 128):
                S = ops.gate_proj_f32w_splits(T, M, E, torch.float16)
                r = ops.gate_proj_f32w_ranges(T, M, E, torch.float16)
                assert 1 <= S <= 64 and len(r) == S and r[0][0] == 0 and r[-1][1] == M
                L = 64 * -(-(M // 64) // S)
                assert all(a == s * L and b == min(M, a + L) and b > a for s, (a, b) in enumerate(r))
