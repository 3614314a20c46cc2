"""MXFP4 expert weights on the packed dropless forward (layer.dropless_packed_fp4 on top of dropless_packed and experts.fp4_weights),
`ffn` and SwiGLU experts, bf16 and fp16: output, l_aux, dispatch_count and routing are the BITS of the padded dropless FP4 forward,
before and after fp4_freeze() and under a HIP graph; with the switch off every forward and every raise is what it was.
T = 512, E = 4, k = 2, M = H = 128.  A constant token feature that the gate weighs +8 / -8 acts as a gate bias: expert 0 is every
token's first choice (512 rows: two table tiles) and expert 3 nobody's."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, M, E, K = 512, 128, 4, 2
NO_GEMM = "the packed dropless forward has no FP4 GEMM"
cases = pytest.mark.parametrize("kind,dtype", [(k, d) for k in ("ffn", "llama_ffn") for d in (torch.bfloat16, torch.float16)],
                                ids=lambda v: str(v).replace("torch.", ""))


def _layer(kind, dtype, hidden=128, **kw):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": K, "capacity_factor": 0.0, "fp32_gate": True},
                              experts={"type": kind, "num_experts_per_device": E, "hidden_size_per_expert": hidden}, model_dim=M, **kw)
    finally:
        torch.set_default_dtype(old)
    g = torch.Generator().manual_seed(5 + hidden)
    with torch.no_grad():
        for p in layer.experts.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.09).to(p.dtype))
        wg = torch.randn([E, M], generator=g) * 0.1
        wg[0, 0], wg[3, 0] = 8.0, -8.0
        layer.gates[0].wg.weight.copy_(wg)
    layer = layer.requires_grad_(False).cuda().eval()
    layer._keep_routing = layer.experts.fp4_weights = True
    return layer


def _batch(dtype, seed):
    x = torch.randn([T, M], generator=torch.Generator().manual_seed(seed)) * 0.5
    x[:, 0] = 4.0
    return x.to(dtype).cuda()


def _run(layer, x, switch, packed):
    """one forward -> [y, l_aux, dispatch_count, idx, loc]"""
    layer.dropless_packed_fp4, layer.dropless_packed = switch, packed
    layer.last_routing = ()
    with torch.no_grad():
        y = layer(x)
    return [t.detach().clone() for t in (y, layer.l_aux.float(), layer.dispatch_count, *layer.last_routing)]


def _same_bits(a, b, what):
    assert len(a) == len(b) == 5, what
    for u, v, part in zip(a, b, ("output", "l_aux", "dispatch_count", "idx", "loc")):
        bits = torch.int16 if u.element_size() == 2 else torch.int32
        assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u.view(bits), v.view(bits)), f"{what}: {part}"


@cases
def test_switch_on_frozen_and_graphed_are_the_bits_of_the_padded_fp4_forward(kind, dtype):
    from tutel_amd.impls.graph import GraphedForward
    layer = _layer(kind, dtype)
    batches = [_batch(dtype, 1), _batch(dtype, 2)]
    padded = [_run(layer, b, False, False) for b in batches]
    assert layer._fp4_weights_ran is True and layer._dropless_packed_ran is None, "the padded dropless FP4 forward"
    assert int(padded[0][2].max()) > 256 and int(padded[0][2].min()) == 0, "an expert above 256 rows and an empty one"
    assert bool(torch.isfinite(padded[0][0].float()).all()) and float(padded[0][0].abs().max()) > 0
    for step in ("switched on", "frozen"):   # FP4-resident: the same bits
        if step == "frozen":
            layer.experts.fp4_freeze()
        _same_bits(_run(layer, batches[0], True, True), padded[0], f"{kind} {step}")
        assert layer._fp4_weights_ran is True and layer._dropless_packed_ran is True, (layer._fp4_weights_ran, layer._dropless_packed_ran)
    layer._keep_routing = False
    g = GraphedForward(layer, batches[0], capacity_factor=0.0, dropless_packed=True)   # (a capture proves that nothing is read back)
    assert layer._fp4_weights_ran is True and layer._dropless_packed_ran is True, "the capture took the FP4 forward"
    for b, want in 2 * list(zip(batches, padded)):
        assert torch.equal(g(b).view(torch.int16), want[0].view(torch.int16)), "a replay against the eager padded FP4 forward"


@cases
def test_switch_off_changes_nothing(kind, dtype):
    layer, x = _layer(kind, dtype), _batch(dtype, 1)
    off = _run(layer, x, False, True)
    if kind == "llama_ffn":   # the one-call 16-bit packed forward, with its recorded reason
        assert layer._dropless_packed_ran is True and layer._fp4_weights_ran == NO_GEMM
        layer.experts.fp4_weights = False
        _same_bits(off, _run(layer, x, False, True), "the 16-bit packed forward")
        layer.experts.fp4_weights = True
    else:                     # `ffn` experts admitted to the W4 engine keep the padded dropless forward
        assert layer._dropless_packed_ran is None and layer._fp4_weights_ran is True
        _same_bits(off, _run(layer, x, False, False), "the padded FP4 forward")
    layer.experts.fp4_freeze()
    with pytest.raises(RuntimeError, match=NO_GEMM):
        _run(layer, x, False, True)


@cases
def test_a_refusal_is_recorded_on_a_switched_module_and_raises_on_a_frozen_one(kind, dtype):
    x = _batch(dtype, 1)
    # H = 96: the W4 ladder refuses; a prescore layer: the ladder admits it, the packed layout does not.  The forward is the one without the switch
    for kw, ran, word in ((dict(hidden=96), "_fp4_weights_ran", "multiple"), (dict(is_postscore=False), "_dropless_packed_ran", "is_postscore")):
        layer = _layer(kind, dtype, **kw)
        today = _run(layer, x, False, True)
        _same_bits(_run(layer, x, True, True), today, f"{kind} {kw}")
        assert isinstance(getattr(layer, ran), str) and word in getattr(layer, ran), (kw, getattr(layer, ran))
    layer.experts.fp4_freeze()
    with pytest.raises(RuntimeError, match="dropless_packed_fp4 is on and .*is_postscore"):
        _run(layer, x, True, True)
