"""W4A8 on the packed dropless forward (layer.dropless_packed_w4a8 on top of dropless_packed, dropless_packed_fp4, fp4_weights or an
FP4-resident module, and experts.w4a8): output, l_aux, dispatch_count and routing are the BITS of the non-packed dropless W4A8 forward,
the layer reports that W4A8 ran, and a HIP graph of it replays on fresh tokens.  The W4A8 layer test's layers and sizes."""
import pytest
import torch
from test_w4a8_layer_gpu import _layer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("frozen", [False, True], ids=["derived", "frozen"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", ["ffn", "llama_ffn"])
def test_switch_on_and_graphed_are_the_bits_of_the_dropless_w4a8_forward(kind, dtype, frozen):
    from tutel_amd.impls.graph import GraphedForward
    layer, x, _ = _layer(kind, dtype, 0.0, frozen)
    layer.experts.w4a8 = layer._keep_routing = True
    other = torch.randn(x.shape, generator=torch.Generator().manual_seed(4)).to(dtype).cuda()

    def run(tokens, packed):
        layer.dropless_packed = layer.dropless_packed_fp4 = layer.dropless_packed_w4a8 = packed
        with torch.no_grad():
            y = layer(tokens)
        assert layer._w4a8_ran is True and layer._dropless_packed_ran is (True if packed else None), (layer._w4a8_ran, layer._dropless_packed_ran)
        return [t.detach().clone() for t in (y, layer.l_aux.float(), layer.dispatch_count, *layer.last_routing)]

    want, want_other = run(x, False), run(other, False)
    assert bool(torch.isfinite(want[0].float()).all()) and float(want[0].abs().max()) > 0
    got = run(x, True)
    assert len(got) == len(want) == 5 and all(torch.equal(u, v) for u, v in zip(got, want)), "output, l_aux, dispatch_count, idx, loc"
    layer._keep_routing = False
    g = GraphedForward(layer, x, capacity_factor=0.0, dropless_packed=True)
    assert layer._w4a8_ran is True and layer._dropless_packed_ran is True, "the capture took the packed W4A8 forward"
    for _ in range(2):
        assert torch.equal(g(other), want_other[0]) and torch.equal(g(x), want[0]), "a replay against the eager forward"
