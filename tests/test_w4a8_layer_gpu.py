"""W4A8 in the layer (experts.w4a8 on top of fp4_weights or an FP4-resident module, off by default): the switched-on forward's experts
equal, bit for bit, the four ops called by hand on the experts' recorded input with the MODULE's images, biases and activation --
quantise, fc1 (gate / up), quantise, fc2 (W_fc3) -- and each product is within the 16-bit GEMM's bar of float64 over the rows quantised
on the CPU and the exactly dequantised MXFP4 weights (per product over the kernel's own hidden rows: tests/test_fp8_activations_layer_gpu.py
says why); the switched-off forward is the W4A16 layer bit for bit; the packed dropless forward keeps W4A16 and says why."""
import pytest
import torch
from test_expert_gemm_w4_gpu import _act64, _encode, _gemm_tol
from test_fp8_activations_layer_gpu import E, H, M, _ids, _layer as _fp8_layer

pytestmark = pytest.mark.gpu


def _layer(kind, dtype, cf, frozen=False):
    # the W8A8 layer test's layer, tokens and record of the experts' own call: its input (tokens and slot map where fc1 gathers) and output
    layer, x, rec = _fp8_layer(kind, dtype, cf)
    layer.experts.fp8_weights, layer.experts.fp4_weights = False, True
    if frozen:
        layer.experts.fp4_freeze()
    return layer, x, rec


def _forward(layer, x, on):
    layer.experts.w4a8 = on
    with torch.no_grad():
        return layer(x).clone()


def _by_hand(kind, ex, rec):
    """the experts' ops on the recorded input -> (y, [(rows, codes, scales, image channels, bias, act, product)] per GEMM)"""
    from tutel_amd import ops
    (c1, s1), (c2, s2) = ex.w4_params()
    x, R, sm = rec["x"], rec["R"], rec["slot_map"]
    glu = kind != "ffn"
    b1, b2, act = (None, None, "silu") if glu else (ex.batched_fc1_bias.detach(), ex.batched_fc2_bias.detach(), "relu")
    xq, sx = ops.quantize_rows_a8(x.reshape(-1, M))
    a = xq if sm is not None else xq.view(E, -1, M)
    h = (ops.expert_gemm_w4a8_glu(a, sx, c1, s1, H, M, x.dtype, act=act) if glu else
         ops.expert_gemm_w4a8(a, sx, c1, s1, b1, H, M, x.dtype, act=act, slot_map=sm, R=R))
    hq, sh = ops.quantize_rows_a8(h.view(-1, H))
    y = ops.expert_gemm_w4a8(hq.view(E, -1, H), sh, c2, s2, b2, M, H, x.dtype)
    rows = x if sm is None else _encode(x.cpu(), sm.cpu(), E, R)
    return y, [(rows, c1, s1, 2 * H if glu else H, b1, act, h), (h, c2, s2, M, b2, "none", y)]


def _check_products(products, dtype):
    """each product against float64 over its rows quantised on the CPU and the image dequantised exactly"""
    from tutel_amd.experts import w4, w8
    for n, (rows, codes, scales, N, bias, act, got) in enumerate(products):
        rows, got = rows.cpu(), got.cpu().double()
        Kd = rows.shape[-1]
        q, s = w8.quantize_e4m3(rows.reshape(1, -1, Kd), True)
        dq = (q.double() * s.double().unsqueeze(2)).view(rows.shape)
        pre = torch.einsum("erk,enk->ern", dq, w4.dequantize(*w4.unpack(codes.cpu(), scales.cpu(), N, Kd)).double())
        if N != got.shape[-1]:   # the gate / up image
            g, u = w8.deinterleave_gate_up(pre.transpose(1, 2))
            want = _act64(g, act).to(dtype).double().transpose(1, 2) * u.transpose(1, 2)
        else:
            want = _act64(pre + (bias.cpu().double().unsqueeze(1) if bias is not None else 0), act)
        print(f"product {n} {dtype}: max abs error {float((got - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3f}")
        torch.testing.assert_close(got, want, **_gemm_tol(dtype))


@pytest.mark.parametrize("frozen", [False, True], ids=["derived", "frozen"])
@pytest.mark.parametrize("cf", [1.0, 0.0], ids=["padded", "dropless"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], **_ids)
@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_switch_on_is_the_four_ops_by_hand_and_switch_off_is_w4a16(kind, dtype, cf, frozen):
    layer, x, rec = _layer(kind, dtype, cf, frozen)
    w4a16 = _forward(layer, x, False)
    assert layer._w4a8_ran is None and layer._fp4_weights_ran is True
    on = _forward(layer, x, True)
    assert layer._w4a8_ran is True, layer._w4a8_ran
    y, products = _by_hand(kind, layer.experts, rec)
    assert torch.equal(rec["y"].view(torch.int16), y.view(torch.int16)), "the experts' output against the four ops by hand"
    _check_products(products, dtype)
    assert torch.equal(on, _forward(layer, x, True)), "a second forward"
    assert torch.equal(_forward(layer, x, False), w4a16) and not torch.equal(on, w4a16), "switch off again: the W4A16 layer's bits"


@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_packed_dropless_forward_keeps_w4a16_and_says_why(kind):
    layer, x, _ = _layer(kind, torch.bfloat16, 0.0)
    layer.dropless_packed = layer.dropless_packed_fp4 = True
    off = _forward(layer, x, False)
    assert layer._dropless_packed_ran is True and layer._fp4_weights_ran is True and layer._w4a8_ran is None
    on = _forward(layer, x, True)
    assert layer._dropless_packed_ran is True and layer._fp4_weights_ran is True and layer._w4a8_ran == "the packed dropless forward has no W4A8 GEMM"
    assert torch.equal(on, off), "the W4A16 bits"
