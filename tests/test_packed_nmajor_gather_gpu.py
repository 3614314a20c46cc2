"""The n-major packed grouped GEMM with its rows gathered through the packed slot map (ops.expert_gemm_packed(..., w_kmajor=False,
gather=True)) on the MI355X.  The packed ffn training step gathers with k-major weights only; a step that keeps its weights as stored
([E, K, N], as SwiGLU experts do) needs this form, which no other test launches.  Pinned bit for bit against the same call on a
materialised packed copy of the tokens.  Every operand sits in a guard band (tests/_packed_fuzz.py::moated): NaN around the inputs, a
sentinel around the outputs, a valid entry naming a NaN token row around the slot map."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_fuzz as F   # noqa: E402
from tutel_amd import ops   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_nmajor_packed_gemm_gathers_its_rows(dtype, act):
    from tutel_amd.impls import ep_native
    torch.manual_seed(3)
    T, E, k, M, N = 700, 16, 2, 192, 128
    x = torch.randn(T, M, device="cuda").to(dtype)
    idx = torch.randint(0, E, [k, T], dtype=torch.int32, device="cuda")
    idx[1] = (idx[0] + 1) % E
    free = T // 2
    idx[:, free] = -1                           # one token nobody routes: its row is NaN, and the slot map's band names it
    x[free] = float("nan")
    idx = idx.contiguous()
    loc, cnt, _, _, _ = ops.compute_location(idx, E)
    plan, why = ep_native.packed_plan(T, E, k, M, 128, 128, dtype, 0, 8)
    assert plan is not None, why
    lay = ops.packed_layout(cnt, idx, loc, 0, 8, plan["rows_bound"], plan["tiles_bound"], 0)
    used = int(lay.offsets[-1])
    smap = lay.slot_map
    assert F.free_token(smap.cpu().numpy(), T) == free
    xp = torch.zeros(lay.rows_bound, M, device="cuda", dtype=dtype)
    ok = smap >= 0
    xp[ok] = x[(smap[ok] % T).long()]
    xp[used:] = float("nan")                    # rows at and past offsets[E]: never read
    assert not bool(torch.isnan(xp[:used]).any())
    lay.slot_map = F.moated(smap, fill=free)
    x, xp = F.moated(x), F.moated(xp)
    assert int((~ok[:used]).sum()) > 0          # pad rows inside the live range: the zero row is read
    w = F.moated((torch.randn(E, M, N, device="cuda") / M ** 0.5).to(dtype))          # [K][N] as stored
    b = F.moated(torch.randn(E, N, device="cuda").to(dtype))
    zero = F.moated(torch.zeros(M, device="cuda", dtype=dtype))
    got = F.moated(torch.full([lay.rows_bound, N], 3.0, device="cuda", dtype=dtype), fill=F.OUT_FILL)
    ref = F.moated(torch.full([lay.rows_bound, N], 3.0, device="cuda", dtype=dtype), fill=F.OUT_FILL)
    ops.expert_gemm_packed(x, w, b, False, lay, act=act, gather=True, zero_row=zero, out=got)
    ops.expert_gemm_packed(xp, w, b, False, lay, act=act, out=ref)
    for t, what in ((got, "out"), (ref, "out of the materialised launch"), (x, "x"), (xp, "packed x"), (w, "w"), (b, "bias"), (zero, "zero_row"),
                    (lay.slot_map, "slot_map")):
        F.moat_intact(t, what)
    assert bool((got[used:] == 3.0).all()) and bool((ref[used:] == 3.0).all())          # rows at or past offsets[E] keep their pre-fill
    assert torch.equal(got[:used], ref[:used])
    assert float(got[:used].float().abs().max()) > 0
    # and against float64 on the live rows of one expert with rows (one rounding of an fp32 sum over K = 192)
    off = lay.offsets.cpu()
    e = int(torch.argmax(off[1:] - off[:-1]))
    r0, r1 = int(off[e]), int(off[e + 1])
    exact = xp[r0:r1].double() @ w[e].double() + b[e].double()
    exact = exact.clamp(min=0) if act == "relu" else exact
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    mag = xp[r0:r1].double().abs() @ w[e].double().abs() + b[e].double().abs()
    assert bool(((got[r0:r1].double() - exact).abs() <= 1.01 * u * exact.abs() + M * 2.0 ** -24 * mag + 2.0 ** -24).all())
