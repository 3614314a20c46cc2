"""FP8 activations in the layer (switch experts.fp8_activations on top of fp8_weights or an FP8-resident module, off by default): the
switched-on forward's experts equal, bit for bit, the four ops called by hand -- quantise, fc1 (gate / up), quantise, fc2 (W_fc3) -- and
each product is within the 16-bit GEMM's bar of float64 over both dequantised operands; the switched-off forward is the W8A16 one and
names the switch; a graph replays; the packed dropless forward keeps W8A16 and says why.

The float64 reference is taken per product over the kernel's own hidden rows: a reference that quantised its OWN hidden rows would
differ from the kernel's by whole e4m3 steps wherever an fp32-accumulation difference moves a value across a rounding boundary, which
is a property of quantisation, not an error of either side."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_layer_gpu as TL                                          # noqa: E402
from test_expert_gemm_w8_gpu import _act64, _encode, _gemm_tol       # noqa: E402
from test_swiglu_packed_gpu import make_layer as make_llama_layer    # noqa: E402

pytestmark = pytest.mark.gpu

T, M, H, E, K = 64, 128, 128, 4, 2
DTYPES = [torch.bfloat16, torch.float16]
OFF = "fp8_activations is off (TUTEL_AMD_FP8_ACTIVATIONS)"
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))


def _layer(kind, dtype, cf, frozen=False, **kw):
    layer = (TL.make_layer if kind == "ffn" else make_llama_layer)(M, H, E, K, cf, dtype, **kw).eval()
    layer.experts.fp8_weights = True
    if frozen:
        layer.experts.fp8_freeze()
    x = torch.randn([T, M], generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    # the experts' own call of a forward: its input (the tokens with a slot map where fc1 gathers, else the buckets) and its output
    rec, ex = {}, layer.experts
    if kind == "ffn":
        real = ex.forward_engine

        def forward_engine(engine, x, R=None, slot_map=None):
            rec.update(x=x, R=R, slot_map=slot_map, y=real(engine, x, R, slot_map))
            return rec["y"]
        ex.forward_engine = forward_engine
    else:
        ex.register_forward_hook(lambda m, args, y: rec.update(x=args[0].contiguous(), R=None, slot_map=None, y=y))
    return layer, x, rec


def _forward(layer, x, on):
    layer.experts.fp8_activations = on
    with torch.no_grad():
        return layer(x).clone()


def _by_hand(kind, ex, rec, a8):
    """the experts' ops on the recorded input -> (y, [(rows, codes, row scales, image, channel scales, bias, act, product)] per GEMM)"""
    from tutel_amd import ops
    (i1, s1), (i2, s2) = ex.w8_params()
    x, R, sm = rec["x"], rec["R"], rec["slot_map"]
    glu = kind != "ffn"
    b1, b2, act = (None, None, "silu") if glu else (ex.batched_fc1_bias.detach(), ex.batched_fc2_bias.detach(), "relu")
    if not a8:
        h = ops.expert_gemm_w8_glu(x, i1, s1, H, M, act=act) if glu else ops.expert_gemm_w8(x, i1, s1, b1, H, M, act=act, slot_map=sm, R=R)
        return ops.expert_gemm_w8(h, i2, s2, b2, M, H), None
    xq, sx = ops.quantize_rows_a8(x.reshape(-1, M))
    a = xq if sm is not None else xq.view(E, -1, M)
    h = (ops.expert_gemm_w8a8_glu(a, sx, i1, s1, H, M, x.dtype, act=act) if glu else
         ops.expert_gemm_w8a8(a, sx, i1, s1, b1, H, M, x.dtype, act=act, slot_map=sm, R=R))
    hq, sh = ops.quantize_rows_a8(h.view(-1, H))
    y = ops.expert_gemm_w8a8(hq.view(E, -1, H), sh, i2, s2, b2, M, H, x.dtype)
    rows = x if sm is None else _encode(x.cpu(), sm.cpu(), E, R)
    return y, [(rows, i1, s1, b1, act, h), (h, i2, s2, b2, "none", y)]


def _check_products(kind, products, dtype):
    """each product against float64 over both operands quantised on the CPU and dequantised exactly"""
    from tutel_amd.experts import w8
    for n, (rows, image, scale, bias, act, got) in enumerate(products):
        rows, got = rows.cpu(), got.cpu()
        Kd = rows.shape[-1]
        q, s = w8.quantize_e4m3(rows.reshape(1, -1, Kd), True)
        dq = (q.double() * s.double().unsqueeze(2)).view(rows.shape)
        N = scale.shape[1]
        wq = w8.unpack(image.cpu(), N, Kd).double() * scale.cpu().double().unsqueeze(2)
        pre = torch.einsum("erk,enk->ern", dq, wq)
        if kind != "ffn" and n == 0:
            g, u = w8.deinterleave_gate_up(pre.transpose(1, 2))
            want = _act64(g, act).to(dtype).double().transpose(1, 2) * u.transpose(1, 2)
        else:
            want = _act64(pre + (bias.cpu().double().unsqueeze(1) if bias is not None else 0), act)
        print(f"{kind} product {n} {dtype}: max abs error {float((got.double() - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3f}")
        torch.testing.assert_close(got.double(), want, **_gemm_tol(dtype))


@pytest.mark.parametrize("frozen", [False, True], ids=["derived", "frozen"])
@pytest.mark.parametrize("cf", [1.0, 0.0], ids=["padded", "dropless"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_switch_on_is_the_four_ops_by_hand_and_switch_off_is_w8a16(kind, dtype, cf, frozen):
    layer, x, rec = _layer(kind, dtype, cf, frozen)
    on = _forward(layer, x, True)
    assert layer._fp8_activations_ran is True, layer._fp8_activations_ran
    y, products = _by_hand(kind, layer.experts, rec, True)
    assert torch.equal(rec["y"].view(torch.int16), y.view(torch.int16)), "the experts' output against the four ops by hand"
    assert bool(torch.isfinite(on.float()).all()) and float(on.abs().max()) > 0
    _check_products(kind, products, dtype)
    again = _forward(layer, x, True)
    assert torch.equal(on, again), "a second forward"
    off = _forward(layer, x, False)
    assert layer._fp8_activations_ran == OFF and layer._fp8_weights_ran is True
    assert torch.equal(rec["y"], _by_hand(kind, layer.experts, rec, False)[0]), "switch off: the W8A16 ops' bits"
    assert not torch.equal(on, off)


@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_graph_capture_replays_the_eager_forward(kind):
    from tutel_amd.impls.graph import GraphedForward
    layer, x, _ = _layer(kind, torch.bfloat16, 1.0)
    eager = _forward(layer, x, True)
    other = (x * 0.5).contiguous()
    eager_other = _forward(layer, other, True)
    with torch.no_grad():
        g = GraphedForward(layer, x)
    assert layer._fp8_activations_ran is True
    for _ in range(3):
        assert torch.equal(g(other), eager_other), "a replay on the second batch"
        assert torch.equal(g(x), eager), "a replay against the eager forward"


@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_packed_dropless_forward_keeps_w8a16_and_says_why(kind):
    layer, x, _ = _layer(kind, torch.bfloat16, 0.0)
    layer.dropless_packed = layer.dropless_packed_fp8 = True
    off = _forward(layer, x, False)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True
    on = _forward(layer, x, True)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True
    assert layer._fp8_activations_ran == "the packed dropless forward has no W8A8 GEMM"
    assert torch.equal(on, off), "the W8A16 bits"
