"""Dropless training of ffn experts on the packed layout (impls/packed_train.py, csrc/packed_train.hip) on the MI355X: the new
kernels against float64 and against the padded kernels, whole training steps against today's padded step and an fp64 autograd
reference, determinism, graph capture of forward + backward, and the refusals."""
import pytest
import torch

from tutel_amd import ops

from _packed_fuzz import bgrad_bound, layout_from_rows as _layout_from_rows, ref_bgrad   # shared with the packed fuzzers

pytestmark = pytest.mark.gpu


# ---- kernels -------------------------------------------------------------------------------------------------------------------


def _wgrad_ref(a, b, off):
    E = off.numel() - 1
    out, bound = [], []
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        A, B = a[r0:r1].double(), b[r0:r1].double()
        out.append(A.t() @ B)
        bound.append(A.abs().t() @ B.abs())
    return torch.stack(out), torch.stack(bound)


ROWS = {1: [[3000]], 8: [[0, 1, 17, 255, 256, 0, 300, 33]],
        64: [[(e * 37) % 200 for e in range(64)], [0] * 63 + [777]],
        128: [[(e * 11) % 45 + (e == 5) for e in range(128)]]}


@pytest.mark.parametrize("E", [1, 8, 64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_wgrad_kernel_against_float64(E, dtype):
    torch.manual_seed(E)
    shapes = [(128, 192), (192, 128)] + ([(2048, 128)] if E <= 8 else [])
    for rows in ROWS[E]:
        lay, idx, loc = _layout_from_rows(rows)
        off = lay.offsets.cpu()
        used = int(off[-1])
        for Na, Nb in shapes:
            a = torch.randn(lay.rows_bound, Na, device="cuda").to(dtype)
            b = torch.randn(lay.rows_bound, Nb, device="cuda").to(dtype)
            a[used:] = float("nan")   # rows past off[E]: never read
            b[used:] = float("nan")
            got = ops.expert_wgrad_packed(a, b, lay)
            ref, bnd = _wgrad_ref(a, b, off)
            err = (got.double() - ref).abs()
            # (+ 2^-24: one rounding in fp16's subnormal range, below 2^-14)
            viol = err - (2 ** -8 * ref.abs() + 2 ** -12 * bnd + (2 ** -24 if dtype == torch.float16 else 0))
            w = int(viol.argmax())
            assert bool((viol <= 0).all()), (Na, Nb, rows, [int(v) for v in torch.unravel_index(torch.tensor(w), viol.shape)],
                                             float(err.view(-1)[w]), float(ref.view(-1)[w]), float(bnd.view(-1)[w]), float(got.view(-1)[w]))
            for e in range(E):
                if rows[e] == 0:
                    assert bool((got[e] == 0).all())
            assert torch.equal(got, ops.expert_wgrad_packed(a, b, lay))   # deterministic
            db = ops.expert_bgrad_packed(b, lay)
            # n_e rows summed in fp32 in order, rounded once: u |ref| + n_e 2^-24 sum |B| (tests/_packed_fuzz.py::bgrad_bound) -- for all
            # but the 3000-row expert far inside the earlier floor of 1e-3 (1 + |ref|), which still holds beside it: a lost row shows
            dref, mag, n_e = ref_bgrad(b.cpu(), off)
            bound = torch.minimum(bgrad_bound(dref, mag, n_e, dtype), 2 ** -8 * dref.abs() + 1e-3 * (1 + dref.abs()))
            assert bool(((db.double().cpu() - dref).abs() <= bound).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_wgrad_kernel_gathered_operand(dtype):
    """B read through the packed slot map (x of dW1): equals the product over a materialised packed copy, bit for bit"""
    torch.manual_seed(3)
    T, E, k, M = 700, 16, 2, 192
    x = torch.randn(T, M, device="cuda").to(dtype)
    idx = torch.randint(0, E, [k, T], dtype=torch.int32, device="cuda")
    idx[1] = (idx[0] + 1) % E
    loc, cnt, _, _, _ = ops.compute_location(idx.contiguous(), E)
    from tutel_amd.impls import ep_native
    plan, _ = ep_native.packed_plan(T, E, k, M, 128, 128, dtype, 0, 8)
    lay = ops.packed_layout(cnt, idx.contiguous(), loc, 0, 8, plan["rows_bound"], plan["tiles_bound"], 0)
    smap = lay.slot_map
    xp = torch.zeros(lay.rows_bound, M, device="cuda", dtype=dtype)
    ok = smap >= 0
    xp[ok] = x[(smap[ok] % T).long()]
    a = torch.randn(lay.rows_bound, 128, device="cuda").to(dtype)
    zero = torch.zeros(M, device="cuda", dtype=dtype)
    got = ops.expert_wgrad_packed(a, x, lay, gather="b", zero_row=zero)
    assert torch.equal(got, ops.expert_wgrad_packed(a, xp, lay))
    got_a = ops.expert_wgrad_packed(x, a, lay, gather="a", zero_row=zero)
    assert torch.equal(got_a, ops.expert_wgrad_packed(xp, a, lay))


def _padded_rows(buf, off, E, C):
    out = torch.zeros(E, C, buf.shape[1], dtype=buf.dtype, device=buf.device)
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        out[e, :r1 - r0] = buf[r0:r1]
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_nmajor_and_gated_packed_gemm_against_padded(dtype):
    torch.manual_seed(5)
    rows = [0, 40, 256, 300, 1, 129, 0, 64]
    lay, _, _ = _layout_from_rows(rows)
    off = lay.offsets.cpu()
    E, K, N = len(rows), 256, 384
    C = max(rows)
    a = torch.randn(lay.rows_bound, K, device="cuda").to(dtype)
    w_nm = (torch.randn(E, K, N, device="cuda") / 16).to(dtype)       # [K][N] as stored
    b = torch.randn(E, N, device="cuda").to(dtype)
    got = ops.expert_gemm_packed(a, w_nm, b, False, lay)
    ref = ops.expert_gemm(_padded_rows(a, off, E, C), w_nm, b, False)
    w_km = (torch.randn(E, N, K, device="cuda") / 16).to(dtype)       # [N][K]
    mul = (torch.randn(lay.rows_bound, N, device="cuda") > 0).to(dtype)
    got_g = ops.expert_gemm_packed(a, w_km, None, True, lay, mul=mul)
    ref_g = ops.expert_gemm(_padded_rows(a, off, E, C), w_km, None, True, mul=_padded_rows(mul, off, E, C))
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 == r0:
            continue
        exact = ref[e, :r1 - r0].double()
        # K orders may differ from the padded launch's kernel choice: the GEMM bar
        assert bool(((got[r0:r1].double() - exact).abs() <= 2 ** -7 * exact.abs() + 2e-2).all())
        exact = ref_g[e, :r1 - r0].double()
        assert bool(((got_g[r0:r1].double() - exact).abs() <= 2 ** -7 * exact.abs() + 2e-2).all())
        assert bool((got_g[r0:r1][mul[r0:r1] == 0] == 0).all())


def test_packed_gate_grad_and_decodes_against_padded():
    torch.manual_seed(7)
    T, E, k, M = 500, 16, 2, 256
    dtype = torch.bfloat16
    idx = torch.randint(0, E, [k, T], dtype=torch.int32, device="cuda")
    idx[1] = (idx[0] + 3) % E
    idx = idx.contiguous()
    loc, cnt, stats, _, _ = ops.compute_location(idx, E)
    C = int(stats[0])
    from tutel_amd.impls import ep_native
    plan, _ = ep_native.packed_plan(T, E, k, M, 128, 128, dtype, 0, 1)
    lay = ops.packed_layout(cnt, idx, loc, 0, 1, plan["rows_bound"], plan["tiles_bound"], 0)
    off = lay.offsets.cpu()
    gates = torch.rand(k, T, device="cuda")
    dy = torch.randn(T, M, device="cuda").to(dtype)
    yp = torch.randn(lay.rows_bound, M, device="cuda").to(dtype)
    pad = _padded_rows(yp, off, E, C).view(E * C, M)
    assert torch.equal(ops.gate_grad_packed(dy, yp, idx, loc, lay), ops.gate_grad(dy, pad, idx, loc, C))
    assert torch.equal(ops.fast_decode_packed(yp, idx, loc, gates, lay), ops.fast_decode(pad, idx, loc, gates, C))
    assert torch.equal(ops.fast_decode_packed(yp, idx, loc, None, lay), ops.fast_decode(pad, idx, loc, None, C))
    # decode's backward: the encode through the packed slot map -- zeros in pad rows
    enc = ops.fast_encode(dy, lay.slot_map, gates, lay.rows_bound)
    ref = ops.fast_encode(dy, ops.slot_map(idx, loc, E, C), gates, E * C).view(E, C, M)
    used = int(off[-1])
    assert torch.equal(_padded_rows(enc, off, E, C), ref)
    assert bool((enc[used:] == 0).all())


# ---- layer steps ---------------------------------------------------------------------------------------------------------------
def make_layer(M, H, E, k, cf, dtype, fp32_gate=False, bias=True, seed=0):
    from tutel import moe
    torch.manual_seed(seed)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": k, "capacity_factor": cf, "fp32_gate": fp32_gate},
                              experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H,
                                       "activation_fn": lambda t: torch.nn.functional.relu(t),
                                       "has_fc1_bias": bias, "has_fc2_bias": bias},
                              model_dim=M)
    finally:
        torch.set_default_dtype(old)
    layer = layer.cuda().train()
    layer._keep_routing = True
    return layer


def _params(layer):
    ex = layer.experts
    ps = [("wg", layer.gates[0].wg.weight), ("w1", ex.batched_fc1_w), ("w2", ex.batched_fc2_w)]
    if ex.batched_fc1_bias is not None:
        ps += [("b1", ex.batched_fc1_bias), ("b2", ex.batched_fc2_bias)]
    return ps


def _step(layer, x, R, packed, x_grad=True):
    layer.dropless_packed = packed
    layer.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(x_grad)
    y = layer(xi)
    loss = (y.float() * R).sum() + y.l_aux.float()
    loss.backward()
    out = {"y": y.detach().clone(), "l_aux": y.l_aux.detach().clone(), "cnt": layer.dispatch_count.clone(),
           "ran": layer._dropless_packed_ran, "routing": tuple(t.clone() for t in layer.last_routing)}
    out["cap"] = layer.dropless_capacity.clone() if out["ran"] is True else int(layer.protected_shape[1])
    for n, p in _params(layer):
        out[n] = p.grad.detach().clone()
    out["x"] = xi.grad.detach().clone() if x_grad else None
    return out


def _reference(layer, x, R, idx, loc, limit):
    """fp64 autograd over the same routing"""
    ex = layer.experts
    P = {n: p.detach().double().requires_grad_(True) for n, p in _params(layer)}
    xd = x.double().requires_grad_(True)
    logits = xd @ P["wg"].t()
    scores = torch.softmax(logits, dim=1)
    k, T = idx.shape
    E = ex.batched_fc1_w.shape[0]
    gl = [scores.gather(1, idx[j].long().unsqueeze(-1)).squeeze(-1) for j in range(k)]
    if k > 1:
        den = torch.clamp(sum(gl), min=torch.finfo(torch.float64).eps)
        gl = [g / den for g in gl]
    y = torch.zeros(T, ex.output_dim, dtype=torch.float64, device=x.device)
    for j in range(k):
        for e in range(E):
            sel = ((idx[j] == e) & (loc[j] < limit)).nonzero().squeeze(-1)
            if sel.numel() == 0:
                continue
            h = xd[sel] @ P["w1"][e].t()
            if "b1" in P:
                h = h + P["b1"][e]
            o = torch.relu(h) @ P["w2"][e]
            if "b2" in P:
                o = o + P["b2"][e]
            y = y.index_add(0, sel, gl[j][sel].unsqueeze(-1) * o)
    ce = torch.zeros(E, dtype=torch.float64, device=x.device).index_add(0, idx[0].long(), torch.full([T], E / T, dtype=torch.float64, device=x.device))
    l_aux = torch.sum(scores.sum(0) * ce) / T
    ((y * R.double()).sum() + l_aux).backward()
    out = {"y": y.detach(), "x": xd.grad}
    out.update({n: p.grad for n, p in P.items()})
    return out


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


def _check_step(T, E, k, cf, dtype, fp32_gate, bias, x_grad, M=256, H=256, same_token=False, seed=0):
    layer = make_layer(M, H, E, k, cf, dtype, fp32_gate=fp32_gate, bias=bias, seed=seed)
    x = torch.randn(T, M, device="cuda").to(dtype)
    if same_token:
        x = x[:1].expand(T, M).contiguous()
    R = torch.randn(T, M, device="cuda")
    pad = _step(layer, x, R, False, x_grad)
    pk = _step(layer, x, R, True, x_grad)
    assert pk["ran"] is True, pk["ran"]
    assert pad["ran"] is None
    assert torch.equal(pk["cnt"], pad["cnt"]) and torch.equal(pk["l_aux"], pad["l_aux"])
    assert all(torch.equal(a, b) for a, b in zip(pk["routing"], pad["routing"]))
    assert pk["cap"].dtype == torch.int32 and int(pk["cap"]) == pad["cap"]
    spe = (T + E - 1) // E
    limit = k * int(-cf * spe) if cf < 0 else 1 << 30
    ref = _reference(layer, x, R, pk["routing"][0], pk["routing"][1], limit)
    # y's elementwise bar, or within twice the padded step's error where that one misses it too (the gates are rounded to the
    # logits' dtype in both paths, the reference's are not)
    err = (pk["y"].double() - ref["y"]).abs()
    err_pad = (pad["y"].double() - ref["y"]).abs()
    assert bool((err <= 2 ** -7 * ref["y"].abs() + 2e-3).all()) or float(err.max()) <= 2 * float(err_pad.max()), \
        (float(err.max()), float(err_pad.max()))
    for n in ["y", "wg", "w1", "w2"] + (["b1", "b2"] if bias else []) + (["x"] if x_grad else []):
        if float(ref[n].double().norm()) == 0:
            assert float(pk[n].double().norm()) == 0 and float(pad[n].double().norm()) == 0
            continue
        e_pk, e_pad = _rel(pk[n], ref[n]), _rel(pad[n], ref[n])
        assert e_pk <= max(2 ** -7, 2 * e_pad), (n, e_pk, e_pad)
    # determinism: a second packed step gives the same bits
    pk2 = _step(layer, x, R, True, x_grad)
    for n in ["y", "wg", "w1", "w2"] + (["b1", "b2"] if bias else []) + (["x"] if x_grad else []):
        assert torch.equal(pk[n], pk2[n]), n
    return layer


CASES = [(1, 8, 1, 0.0), (333, 8, 2, 0.0), (333, 64, 4, -0.5), (700, 16, 2, -1.0), (2000, 128, 2, 0.0), (517, 32, 1, -2.0)]


@pytest.mark.parametrize("T,E,k,cf", CASES)
def test_packed_step_shapes(T, E, k, cf):
    _check_step(T, E, k, cf, torch.bfloat16, False, True, True, seed=T + E)
    _check_step(T, E, k, cf, torch.bfloat16, False, True, True, same_token=True, seed=T + E + 1)   # every token on k experts


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fp32_gate", [False, True])
@pytest.mark.parametrize("bias,x_grad", [(True, True), (False, False)])
def test_packed_step_variants(dtype, fp32_gate, bias, x_grad):
    _check_step(600, 16, 2, 0.0, dtype, fp32_gate, bias, x_grad, M=192, H=320, seed=11)


def test_sgd_loss_curves_agree():
    torch.manual_seed(2)
    losses = {}
    x = torch.randn(512, 128, device="cuda").to(torch.bfloat16)
    for packed in (False, True):
        layer = make_layer(128, 256, 8, 2, 0.0, torch.bfloat16, seed=4)
        layer.dropless_packed = packed
        opt = torch.optim.SGD(layer.parameters(), lr=0.05)
        cur = []
        for _ in range(5):
            opt.zero_grad()
            y = layer(x)
            loss = y.float().square().mean() + y.l_aux.float()
            loss.backward()
            opt.step()
            cur.append(float(loss))
        losses[packed] = cur
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 2 ** -7 * abs(a) + 1e-3, (losses[False], losses[True])


def test_graph_capture_of_training_step():
    """forward + backward captured once, replayed over batches whose maximum load differs: each replay equals an eager packed step"""
    T, M, E, k = 1024, 256, 16, 2
    layer = make_layer(M, 256, E, k, 0.0, torch.bfloat16, seed=9)
    layer.dropless_packed = True
    params = [p for _, p in _params(layer)]
    static_x = torch.randn(T, M, device="cuda").to(torch.bfloat16)

    def step():
        for p in params:
            p.grad = None
        y = layer(static_x)
        loss = y.float().square().mean() + y.l_aux.float()
        loss.backward()
        return y, y.l_aux

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    assert layer._dropless_packed_ran is True
    g = torch.cuda.CUDAGraph()
    for p in params:
        p.grad = None
    with torch.cuda.graph(g):
        sy, sl = step()
    sgrads = [p.grad for p in params]
    torch.manual_seed(1)
    batches = [torch.randn(T, M, device="cuda").to(torch.bfloat16),
               (torch.randn(T, M, device="cuda") * 3).to(torch.bfloat16),
               torch.randn(1, M, device="cuda").to(torch.bfloat16).expand(T, M).contiguous()]   # all tokens on k experts
    for xb in batches:
        static_x.copy_(xb)
        g.replay()
        torch.cuda.synchronize()
        ry, rl, rg = sy.clone(), sl.clone(), [t.clone() for t in sgrads]
        ey, el = step()
        assert torch.equal(ry, ey) and torch.equal(rl, el)
        for a, p in zip(rg, params):
            assert torch.equal(a, p.grad)


def test_configs2_shape_against_fp64():
    """T = 4096, M = H = 2048, E = 64, top-2, bf16, dropless: gradients of the weights against the fp64 reference"""
    T, M, H, E, k = 4096, 2048, 2048, 64, 2
    layer = make_layer(M, H, E, k, 0.0, torch.bfloat16, seed=1)
    x = torch.randn(T, M, device="cuda").to(torch.bfloat16)
    R = torch.randn(T, M, device="cuda") / 64
    pk = _step(layer, x, R, True, True)
    assert pk["ran"] is True
    ref = _reference(layer, x, R, pk["routing"][0], pk["routing"][1], 1 << 30)
    for n in ("y", "x", "w1", "b1", "w2", "b2", "wg"):
        assert _rel(pk[n], ref[n]) <= 2 ** -7, (n, _rel(pk[n], ref[n]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(layer, x, R, why):
    torch.manual_seed(123)   # (gate noise draws from the generator)
    pad = _step(layer, x, R, False)
    torch.manual_seed(123)
    pk = _step(layer, x, R, True)
    assert isinstance(pk["ran"], str) and why in pk["ran"], pk["ran"]
    for n in ("y", "l_aux", "w1", "w2", "wg", "x"):
        assert torch.equal(pad[n], pk[n]), n


def test_refusals_keep_the_padded_step():
    x = torch.randn(256, 128, device="cuda").to(torch.bfloat16)
    R = torch.randn(256, 128, device="cuda")
    layer = make_layer(128, 256, 8, 2, 0.0, torch.bfloat16)
    layer.is_postscore = False
    _refused(layer, x, R, "is_postscore")
    layer = make_layer(128, 256, 8, 2, 0.0, torch.bfloat16)
    layer.batch_prioritized_routing = True
    _refused(layer, x, R, "batch-prioritised")
    layer = make_layer(128, 256, 8, 2, 0.0, torch.bfloat16)
    layer.is_gshard_loss = False
    layer.gates[0].gate_noise = 1.0
    _refused(layer, x, R, "gate noise")
    layer = make_layer(128, 256, 8, 2, 0.0, torch.bfloat16)
    layer.experts.activation_fn = torch.nn.functional.gelu
    layer.experts._act_cache.clear()
    _refused(layer, x, R, "ReLU")
    layer = make_layer(128, 100 * 8 // 8 + 60, 8, 2, 0.0, torch.bfloat16)   # H = 160: not a multiple of 64
    _refused(layer, x, R, "multiples of 64")
