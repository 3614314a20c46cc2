"""tutel_amd_expert_gemm_w4a8_packed / _glu_packed and tutel_amd_quantize_rows_a8_bounded on the MI355X.  One launch of six experts with
0, 1, 33, 128, 129 and 300 rows (an empty expert, one group, a ragged group, an exact half, a row over a half, more than a table tile),
N = 160 (H = 80: a ragged channel tile with a clamped wave), K = 64, 192, 320 (one tile, a half-used scale dword, more K-tiles than the
ring holds), in both window forms: (a) every packed row is the padded kernel's bits for the same quantised row, scale and expert, (b) it
is within the 16-bit GEMM's bar of float64 over the CPU-quantised rows and the exactly dequantised image, (c) D past offsets[E] and
around it keeps its sentinel.  The rows past offsets[E] of a plain A hold the NaN code with a NaN scale."""
import functools

import pytest
import torch
from _packed_fuzz import layout_from_rows, moat_intact, moated
from test_expert_gemm_w4_gpu import _act64, _gemm_tol

pytestmark = pytest.mark.gpu
ROWS, N, H, KS, FILL = [0, 1, 33, 128, 129, 300], 160, 80, (64, 192, 320), 1234.0
dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


@functools.lru_cache(maxsize=None)
def _problem(dtype, glu, gather, K):
    """computed once, never modified: the layout, its offsets, the quantised rows the kernel reads (codes, scales), the packed image, the
    bias and the float64 pre-activations [used, channels] of the live packed rows (GLU: gate channels first, then up) with their experts"""
    from tutel_amd.experts import w4, w8
    lay, idx, _ = layout_from_rows(ROWS)
    off, slot = lay.offsets.cpu(), lay.slot_map.cpu().long()
    used, E, C = int(off[-1]), len(ROWS), 2 * H if glu else N
    g = torch.Generator().manual_seed(97 * K + 2 * glu + gather)
    a = torch.randn([idx.shape[1] if gather else lay.rows_bound, K], generator=g).to(dtype)
    if not gather:
        a[used:] = float("nan")
    q, s = w8.quantize_e4m3(a.unsqueeze(0), True)
    codes, scales = w4.quantize_mxfp4((torch.randn([E, C, K], generator=g) / K ** 0.5).to(dtype), True, dtype)
    bias = None if glu else torch.randn([E, N], generator=g).to(dtype)
    sel = slot[:used] % a.shape[0] if gather else torch.arange(used)
    assert not gather or int(slot[:used].min()) >= 0, "alignment 1: no pad rows"
    expert = torch.repeat_interleave(torch.arange(E), off[1:] - off[:-1])
    pre = torch.einsum("rk,rnk->rn", (q[0].double() * s[0].double().unsqueeze(1))[sel], w4.dequantize(codes, scales).double()[expert])
    if glu:
        codes, scales = w8.interleave_gate_up(codes[:, :H], codes[:, H:]), w8.interleave_gate_up(scales[:, :H], scales[:, H:])
    else:
        pre = pre + bias.double()[expert]
    return lay, off, sel, q[0].view(torch.uint8), s[0].contiguous(), w4.pack(codes, scales), bias, pre


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gathered"])
@pytest.mark.parametrize("glu", [False, True], ids=["bias_relu", "glu_silu"])
@dtypes
@pytest.mark.parametrize("form", ["halves", "wide"])
def test_packed_rows_are_the_padded_kernels_bits_within_the_bar_of_float64(form, dtype, glu, gather, monkeypatch):
    from tutel_amd import ops
    monkeypatch.setenv("TUTEL_AMD_W4A8_PACKED_TILE", form)   # (the library reads it at every call)
    for K in KS:
        lay, off, sel, q, s, image, bias, pre = _problem(dtype, glu, gather, K)
        q, s, ci, si, b = (None if t is None else t.cuda() for t in (q, s, *image, bias))
        out = moated(torch.full([lay.rows_bound, H if glu else N], FILL, dtype=dtype), fill=FILL, device=torch.device("cuda"))
        kw = dict(gather=gather, zero_row=torch.zeros([K], dtype=torch.uint8, device="cuda") if gather else None, out=out)
        got = (ops.expert_gemm_w4a8_glu_packed(q, s, ci, si, H, K, dtype, lay, act="silu", **kw) if glu else
               ops.expert_gemm_w4a8_packed(q, s, ci, si, b, N, K, dtype, lay, act="relu", **kw))
        torch.cuda.synchronize()
        assert got is out
        moat_intact(out, "D")
        assert bool((out[int(off[-1]):] == FILL).all()), f"K={K}: a row at or past offsets[E] was written"
        for e in range(len(ROWS)):   # (a) the padded kernel on each expert's own quantised rows
            lo, hi = int(off[e]), int(off[e + 1])
            if hi > lo:
                rq, rs = q[sel[lo:hi].cuda()].unsqueeze(0), s[sel[lo:hi].cuda()].contiguous()
                one = (ops.expert_gemm_w4a8_glu(rq, rs, ci[e:e + 1], si[e:e + 1], H, K, dtype, act="silu") if glu else
                       ops.expert_gemm_w4a8(rq, rs, ci[e:e + 1], si[e:e + 1], b[e:e + 1], N, K, dtype, act="relu"))
                assert torch.equal(out[lo:hi], one[0]), f"K={K}: expert {e}'s packed rows against the padded kernel"
        have, want = out[:int(off[-1])].cpu().double(), _act64(pre[:, :H] if glu else pre, "relu" if not glu else "silu")   # (b)
        if glu:
            # the contract rounds the gate to the dtype before the product.  The kernel's gate is an fp32 sum of K <= 320 products: within
            # its accumulation error (below 2^-13 relative at these sizes) of a rounding boundary it may take either neighbour, a whole
            # ulp apart, so the gate is rounded from three points and the nearest result is the reference; elsewhere the three agree
            wants = torch.stack([(want * f).to(dtype).double() * pre[:, H:] for f in (1 - 2.0 ** -13, 1.0, 1 + 2.0 ** -13)])
            want = wants.gather(0, (wants - have).abs().argmin(0, keepdim=True))[0]
        print(f"{form} K={K}: max abs error {float((have - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3f}")
        torch.testing.assert_close(have, want, **_gemm_tol(dtype))


@pytest.mark.parametrize("live", [21, 99], ids=["bound_inside_a_workgroup", "bound_past_the_rows"])
@pytest.mark.parametrize("K", [64, 576, 2112])   # the three compiled row lengths
@dtypes
def test_bounded_quantiser_writes_the_unbounded_bits_below_the_bound_and_nothing_from_it_on(dtype, K, live):
    from tutel_amd import ops
    rows = 37
    x = torch.randn([rows, K], generator=torch.Generator().manual_seed(K)).to(dtype).cuda()
    q0, s0 = ops.quantize_rows_a8(x)
    x[live:] = float("nan")   # rows that must not be read as data: were they, their NaN code and scale would replace the poison
    q, s = torch.full([rows, K], 0xA5, dtype=torch.uint8, device="cuda"), torch.full([rows], -7.0, device="cuda")
    assert ops.quantize_rows_a8(x, out=q, scale=s, rows_dev=torch.tensor([0, live], dtype=torch.int32, device="cuda")[1:]) is not None
    n = min(live, rows)
    assert torch.equal(q[:n], q0[:n]) and torch.equal(s[:n], s0[:n]), "rows below the bound: the unbounded kernel's bits"
    assert bool((q[n:] == 0xA5).all()) and bool((s[n:] == -7.0).all()), "rows at and past the bound keep their poison"
