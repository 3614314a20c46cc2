"""W8A8 on the packed dropless forward (layer.dropless_packed_w8a8 on top of dropless_packed, dropless_packed_fp8, fp8_weights or an
FP8-resident module, and experts.fp8_activations): output, l_aux, dispatch_count and routing are the BITS of the non-packed dropless
W8A8 forward, the layer reports that W8A8 ran, and a HIP graph of it replays on fresh tokens; with the switch off W8A16 runs and says why;
a W8A8 ladder refusal leaves its reason and yields the packed W8A16 bits.  The FP8-activations layer test's layers and sizes."""
import pytest
import torch
from test_fp8_activations_layer_gpu import _forward, _layer

pytestmark = pytest.mark.gpu
KINDS = pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])


@pytest.mark.parametrize("frozen", [False, True], ids=["derived", "frozen"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@KINDS
def test_switch_on_and_graphed_are_the_bits_of_the_dropless_w8a8_forward(kind, dtype, frozen):
    from tutel_amd.impls.graph import GraphedForward
    layer, x, _ = _layer(kind, dtype, 0.0, frozen)
    layer.experts.fp8_activations = layer._keep_routing = True
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(4)).to(dtype).cuda()

    def run(tokens, packed):
        layer.dropless_packed = layer.dropless_packed_fp8 = layer.dropless_packed_w8a8 = packed
        with torch.no_grad():
            y = layer(tokens)
        assert layer._fp8_activations_ran is True and layer._dropless_packed_ran is (True if packed else None), (
            layer._fp8_activations_ran, layer._dropless_packed_ran)
        return [t.detach().clone() for t in (y, layer.l_aux.float(), layer.dispatch_count, *layer.last_routing)]

    want, want_other = run(x, False), run(other, False)
    assert bool(torch.isfinite(want[0].float()).all()) and float(want[0].abs().max()) > 0
    got = run(x, True)
    assert len(got) == len(want) == 5 and all(torch.equal(u, v) for u, v in zip(got, want)), "output, l_aux, dispatch_count, idx, loc"
    layer._keep_routing = False
    g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
    assert layer._fp8_activations_ran is True and layer._dropless_packed_ran is True, "the capture took the packed W8A8 forward"
    for _ in range(2):
        assert torch.equal(g(other), want_other[0]) and torch.equal(g(x), want[0]), "a replay against the eager forward"


@KINDS
def test_switch_off_and_a_ladder_refusal_run_packed_w8a16_and_say_why(kind, monkeypatch):
    from tutel_amd import ops
    layer, x, _ = _layer(kind, torch.bfloat16, 0.0)
    layer.dropless_packed = layer.dropless_packed_fp8 = True
    w8a16 = _forward(layer, x, False)
    assert _forward(layer, x, True).equal(w8a16) and layer._fp8_activations_ran == "the packed dropless forward has no W8A8 GEMM"
    layer.dropless_packed_w8a8 = True
    assert not _forward(layer, x, True).equal(w8a16) and layer._fp8_activations_ran is True
    # one rung of the W8A8 ladder refuses: its reason stays, the packed W8A16 forward runs
    monkeypatch.setattr(ops, "quantize_rows_a8_supported", lambda dtype, K: False)
    got = _forward(layer, x, True)
    assert layer._dropless_packed_ran is True and layer._fp8_weights_ran is True
    assert isinstance(layer._fp8_activations_ran, str) and "W8A8" in layer._fp8_activations_ran, layer._fp8_activations_ran
    assert torch.equal(got, w8a16), "the packed W8A16 bits"
