"""tutel_amd_expert_gemm_w8a8_packed / _glu_packed on the MI355X.  One launch of six experts with 0, 1, 33, 128, 129 and 300 rows (an empty
expert, one group, a ragged group, an exact half, a row over a half, more than a table tile), N = 160 (H = 80: a ragged channel tile with
a clamped wave), K = 64, 192, 320 (one tile, fewer than the ring, more K-tiles than the ring holds), in both window forms: (a) every packed
row is the padded kernel's bits for the same quantised row, scale and expert, (b) it is within the 16-bit GEMM's bar of float64 over the
CPU-quantised rows and the exactly dequantised image, (c) D past offsets[E] and around it keeps its sentinel, (d) the rows of a plain A
from offsets[E] on hold the NaN code with a NaN scale, so a kernel that read one would fail (b).  Those six experts reach the wide form's
K loops for 1, 2, 4, 5 and 8 live 32-row groups; a second launch of 70, 190 and 200 rows reaches the loops for 3, 6 and 7."""
import functools

import pytest
import torch
from _packed_fuzz import layout_from_rows, moat_intact, moated
from test_expert_gemm_w4_gpu import _act64, _gemm_tol

pytestmark = pytest.mark.gpu
ROWS, N, H, KS, FILL = {"six": (0, 1, 33, 128, 129, 300), "groups_3_6_7": (70, 190, 200)}, 160, 80, (64, 192, 320), 1234.0


@functools.lru_cache(maxsize=None)
def _problem(rows, dtype, glu, gather, K):
    """computed once, never modified: the layout, its offsets, the rows' indices, the quantised rows the kernel reads (codes, scales),
    the image and its channel scales, the bias and the float64 pre-activations [used, channels] of the live packed rows (GLU: gate
    channels first, then up)"""
    from tutel_amd.experts import w8
    lay, idx, _ = layout_from_rows(list(ROWS[rows]))
    off, slot = lay.offsets.cpu(), lay.slot_map.cpu().long()
    used, E, C = int(off[-1]), len(ROWS[rows]), 2 * H if glu else N
    g = torch.Generator().manual_seed(89 * K + 2 * glu + gather)
    nrow = idx.shape[1] if gather else used
    q, s = w8.quantize_e4m3(torch.randn([1, nrow, K], generator=g).to(dtype), True)
    q, s = q[0].view(torch.uint8), s[0].contiguous()
    sel = slot[:used] % nrow if gather else torch.arange(used)
    assert not gather or int(slot[:used].min()) >= 0, "alignment 1: no pad rows"
    wq, ws = w8.quantize_e4m3((torch.randn([E, C, K], generator=g) / K ** 0.5).to(dtype), True)
    bias = None if glu else torch.randn([E, N], generator=g).to(dtype)
    expert = torch.repeat_interleave(torch.arange(E), off[1:] - off[:-1])
    pre = torch.einsum("rk,rnk->rn", (q.view(torch.float8_e4m3fn).double() * s.double().unsqueeze(1))[sel],
                       (wq.double() * ws.double().unsqueeze(2))[expert])
    if glu:
        wq, ws = w8.interleave_gate_up(wq[:, :H], wq[:, H:]), w8.interleave_gate_up(ws[:, :H], ws[:, H:]).contiguous()
    else:
        pre = pre + bias.double()[expert]
    if not gather:   # (d) the rows from offsets[E] on, up to rows_bound and eight past it
        extra = lay.rows_bound + 8 - used
        q, s = torch.cat([q, torch.full([extra, K], 0x7F, dtype=torch.uint8)]), torch.cat([s, torch.full([extra], float("nan"))])
    return lay, off, sel, q, s, w8.pack(wq), ws, bias, pre


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gathered"])
@pytest.mark.parametrize("glu", [False, True], ids=["bias_relu", "glu_silu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("form", ["halves", "wide"])
@pytest.mark.parametrize("rows", list(ROWS))
def test_packed_rows_are_the_padded_kernels_bits_within_the_bar_of_float64(rows, form, dtype, glu, gather, monkeypatch):
    from tutel_amd import ops
    monkeypatch.setenv("TUTEL_AMD_W8A8_PACKED_TILE", form)   # (the library reads it at every call)
    for K in KS:
        lay, off, sel, q, s, image, scale, bias, pre = _problem(rows, dtype, glu, gather, K)
        q, s, image, scale, b = (None if t is None else t.cuda() for t in (q, s, image, scale, bias))
        used = int(off[-1])
        out = moated(torch.full([lay.rows_bound, H if glu else N], FILL, dtype=dtype), fill=FILL, device=torch.device("cuda"))
        kw = dict(gather=gather, zero_row=torch.zeros([K], dtype=torch.uint8, device="cuda") if gather else None, out=out)
        got = (ops.expert_gemm_w8a8_glu_packed(q, s, image, scale, H, K, dtype, lay, act="silu", **kw) if glu else
               ops.expert_gemm_w8a8_packed(q, s, image, scale, b, N, K, dtype, lay, act="relu", **kw))
        torch.cuda.synchronize()
        assert got is out
        moat_intact(out, "D")   # (c)
        assert bool((out[used:] == FILL).all()), f"K={K}: a row at or past offsets[E] was written"
        for e in range(len(ROWS[rows])):   # (a) the padded kernel on each expert's own quantised rows
            lo, hi = int(off[e]), int(off[e + 1])
            if hi > lo:
                rq, rs = q[sel[lo:hi].cuda()].unsqueeze(0), s[sel[lo:hi].cuda()].contiguous()
                one = (ops.expert_gemm_w8a8_glu(rq, rs, image[e:e + 1], scale[e:e + 1], H, K, dtype, act="silu") if glu else
                       ops.expert_gemm_w8a8(rq, rs, image[e:e + 1], scale[e:e + 1], b[e:e + 1], N, K, dtype, act="relu"))
                assert torch.equal(out[lo:hi], one[0]), f"K={K}: expert {e}'s packed rows against the padded kernel"
        have, want = out[:used].cpu().double(), _act64(pre[:, :H] if glu else pre, "relu" if not glu else "silu")   # (b)
        if glu:
            # the contract rounds the gate to the dtype before the product.  The kernel's gate is an fp32 sum of K <= 320 products: within
            # its accumulation error (below 2^-13 relative at these sizes) of a rounding boundary it may take either neighbour, a whole
            # ulp apart, so the gate is rounded from three points and the nearest result is the reference; elsewhere the three agree
            wants = torch.stack([(want * f).to(dtype).double() * pre[:, H:] for f in (1 - 2.0 ** -13, 1.0, 1 + 2.0 ** -13)])
            want = wants.gather(0, (wants - have).abs().argmin(0, keepdim=True))[0]
        print(f"{form} K={K}: max abs error {float((have - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3f}")
        torch.testing.assert_close(have, want, **_gemm_tol(dtype))
