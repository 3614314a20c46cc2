"""Packed dropless training under torch.autocast over fp32 master weights (impls/packed_train.py) on the MI355X: the fp32-output
weight / bias gradient kernels against float64 and against their 16-bit siblings, the fp16 overflow the fp32 form removes, whole
autocast steps against the padded step and an fp64 autograd reference, graph capture with the master -> compute-copy cast inside
the graph, and a GradScaler run."""
import pytest
import torch

from tutel_amd import ops

from _packed_fuzz import layout_from_rows, ref_bgrad, ref_wgrad

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


# ---- kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [[3000], [0, 1, 17, 255, 256, 0, 300, 33]], ids=["E1", "E8"])
def test_f32_gradients_against_float64_and_16bit_siblings(dtype, rows):
    """(a) rounding the fp32 result once gives the 16-bit entry point's bits: the same sum; (b) against fp64, per element,
    |err| <= 2^-23 |ref| + 2 n_e 2^-24 (|A|^T |B|): products of two 16-bit values are exact in fp32, each of the n_e fp32 additions
    loses at most half an ulp of a partial sum bounded by |A|^T |B|, and the factor 2 covers the MFMA's grouping of 16 products;
    (c) experts without rows are exact zeros; (d) a second call gives the same bits; (e) the bias gradient alike,
    |err| <= n_e 2^-24 sum |B| + 2^-23 |ref|."""
    torch.manual_seed(len(rows))
    lay, _, _ = layout_from_rows(rows)
    off = lay.offsets.cpu()
    used = int(off[-1])
    assert used == sum(rows)
    n_e = torch.tensor(rows, dtype=torch.float64)
    for Na, Nb in [(128, 192), (192, 128)]:
        a = torch.randn(lay.rows_bound + 64, Na, device="cuda").to(dtype)
        b = torch.randn(lay.rows_bound + 64, Nb, device="cuda").to(dtype)
        a[used:] = float("nan")   # rows at and past off[E]: never read
        b[used:] = float("nan")
        got = ops.expert_wgrad_packed(a, b, lay, out_dtype=torch.float32)
        assert got.dtype == torch.float32 and got.shape == (len(rows), Na, Nb)
        assert torch.equal(got.to(dtype), ops.expert_wgrad_packed(a, b, lay))                          # (a)
        ref, bnd = ref_wgrad(a.cpu(), b.cpu(), off)
        err = (got.double().cpu() - ref).abs()
        viol = err - (2 ** -23 * ref.abs() + 2 * n_e.view(-1, 1, 1) * 2 ** -24 * bnd)
        w = int(viol.argmax())
        assert bool((viol <= 0).all()), (Na, Nb, [int(v) for v in torch.unravel_index(torch.tensor(w), viol.shape)],   # (b)
                                         float(err.view(-1)[w]), float(ref.view(-1)[w]), float(bnd.view(-1)[w]))
        for e, n in enumerate(rows):
            if n == 0:
                assert bool((got[e] == 0).all())                                                       # (c)
        assert torch.equal(got, ops.expert_wgrad_packed(a, b, lay, out_dtype=torch.float32))           # (d)
        db = ops.expert_bgrad_packed(b, lay, out_dtype=torch.float32)                                  # (e)
        assert db.dtype == torch.float32 and torch.equal(db.to(dtype), ops.expert_bgrad_packed(b, lay))
        dref, mag, n = ref_bgrad(b.cpu(), off)
        assert bool(((db.double().cpu() - dref).abs() <= n.unsqueeze(1) * 2 ** -24 * mag + 2 ** -23 * dref.abs()).all())
        assert torch.equal(db, ops.expert_bgrad_packed(b, lay, out_dtype=torch.float32))
    with pytest.raises(Exception, match="float32"):
        ops.expert_wgrad_packed(a, b, lay, out_dtype=torch.float64)


def test_f32_gradient_survives_the_fp16_overflow():
    """300 rows of 16 * 16: 76800 is past fp16's 65504 and exact in the fp32 accumulator"""
    lay, _, _ = layout_from_rows([300])
    a = torch.full([lay.rows_bound, 128], 16.0, device="cuda", dtype=torch.float16)
    b = torch.full([lay.rows_bound, 128], 16.0, device="cuda", dtype=torch.float16)
    assert bool(torch.isinf(ops.expert_wgrad_packed(a, b, lay)).all())
    got = ops.expert_wgrad_packed(a, b, lay, out_dtype=torch.float32)
    assert got.dtype == torch.float32 and bool((got == 76800.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_gradient_gathered_operand(dtype):
    """an operand read through the packed slot map: equal to the product over a materialised packed copy, bit for bit"""
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
    f32 = torch.float32
    got = ops.expert_wgrad_packed(a, x, lay, gather="b", zero_row=zero, out_dtype=f32)
    assert got.dtype == f32 and torch.equal(got, ops.expert_wgrad_packed(a, xp, lay, out_dtype=f32))
    got_a = ops.expert_wgrad_packed(x, a, lay, gather="a", zero_row=zero, out_dtype=f32)
    assert got_a.dtype == f32 and torch.equal(got_a, ops.expert_wgrad_packed(xp, a, lay, out_dtype=f32))


# ---- layer steps under autocast --------------------------------------------------------------------------------------------------
def make_layer(M, H, E, k, cf, bias=True, seed=0):
    """an fp32 layer (fp32 master weights), as examples/helloworld_amp.py builds it"""
    from tutel import moe
    assert torch.get_default_dtype() == torch.float32
    torch.manual_seed(seed)
    layer = moe.moe_layer(gate_type={"type": "top", "k": k, "capacity_factor": cf},
                          experts={"type": "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H,
                                   "activation_fn": lambda t: torch.nn.functional.relu(t),
                                   "has_fc1_bias": bias, "has_fc2_bias": bias},
                          model_dim=M)
    layer = layer.cuda().train()
    layer._keep_routing = True
    return layer


def _params(layer):
    ex = layer.experts
    ps = [("wg", layer.gates[0].wg.weight), ("w1", ex.batched_fc1_w), ("w2", ex.batched_fc2_w)]
    if ex.batched_fc1_bias is not None:
        ps += [("b1", ex.batched_fc1_bias), ("b2", ex.batched_fc2_bias)]
    return ps


def _step(layer, x, R, packed, amp, x_grad=True):
    layer.dropless_packed = packed
    layer.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(x_grad)
    with torch.autocast("cuda", dtype=amp):
        y = layer(xi)
        loss = (y.float() * R).sum() + y.l_aux.float()
    loss.backward()
    out = {"y": y.detach().clone(), "l_aux": y.l_aux.detach().clone(), "cnt": layer.dispatch_count.clone(),
           "ran": layer._dropless_packed_ran, "routing": tuple(t.clone() for t in layer.last_routing)}
    out["cap"] = layer.dropless_capacity.clone() if out["ran"] is True else int(layer.protected_shape[1])
    for n, p in _params(layer):
        out[n] = p.grad.detach().clone()
        out[n + ".dtype"] = p.grad.dtype
    out["x"] = xi.grad.detach().clone() if x_grad else None
    return out


def _reference(layer, x, R, idx, loc, limit, amp):
    """fp64 autograd over the same routing, on what the step computes with: the tokens and the experts' masters rounded to the
    autocast dtype (the compute copies); the gate projects with its fp32 weight as it is (autocast off around it)"""
    ex = layer.experts
    P = {n: (p.detach() if n == "wg" else p.detach().to(amp)).double().requires_grad_(True) for n, p in _params(layer)}
    xd = x.to(amp).double().requires_grad_(True)
    scores = torch.softmax(xd @ P["wg"].t(), dim=1)
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


def _check_step(T, E, k, cf, amp, bias, x_grad, M=192, H=320, same_token=False, seed=0):
    layer = make_layer(M, H, E, k, cf, bias=bias, seed=seed)
    x = torch.randn(T, M, device="cuda")
    if same_token:
        x = x[:1].expand(T, M).contiguous()
    R = torch.randn(T, M, device="cuda")
    pad = _step(layer, x, R, False, amp, x_grad)
    pk = _step(layer, x, R, True, amp, x_grad)
    assert pk["ran"] is True, pk["ran"]
    assert pad["ran"] is None
    assert torch.equal(pk["cnt"], pad["cnt"]) and torch.equal(pk["l_aux"], pad["l_aux"])
    assert all(torch.equal(a, b) for a, b in zip(pk["routing"], pad["routing"]))
    assert pk["cap"].dtype == torch.int32 and int(pk["cap"]) == pad["cap"]
    names = ["wg", "w1", "w2"] + (["b1", "b2"] if bias else [])
    for n in names:
        assert pk[n + ".dtype"] == torch.float32, n
    spe = (T + E - 1) // E
    limit = k * int(-cf * spe) if cf < 0 else 1 << 30
    ref = _reference(layer, x, R, pk["routing"][0], pk["routing"][1], limit, amp)
    for n in ["y"] + names + (["x"] if x_grad else []):
        if float(ref[n].double().norm()) == 0:
            assert float(pk[n].double().norm()) == 0 and float(pad[n].double().norm()) == 0
            continue
        e_pk, e_pad = _rel(pk[n], ref[n]), _rel(pad[n], ref[n])
        assert e_pk <= max(2 ** -7, 2 * e_pad), (n, e_pk, e_pad)
    pk2 = _step(layer, x, R, True, amp, x_grad)   # determinism: a second packed step gives the same bits
    for n in ["y"] + names + (["x"] if x_grad else []):
        assert torch.equal(pk[n], pk2[n]), n


@pytest.mark.parametrize("amp", DTYPES)
@pytest.mark.parametrize("T,E,k,cf", [(1, 8, 1, 0.0), (333, 8, 2, 0.0), (700, 16, 2, -1.0)])
def test_autocast_step_shapes(T, E, k, cf, amp):
    _check_step(T, E, k, cf, amp, True, True, seed=T + E)


@pytest.mark.parametrize("amp", DTYPES)
@pytest.mark.parametrize("bias,x_grad,same_token", [(True, True, True),      # every token on the same k experts
                                                    (False, False, False), (True, False, False), (False, True, False)])
def test_autocast_step_variants(bias, x_grad, same_token, amp):
    _check_step(333, 8, 2, 0.0, amp, bias, x_grad, same_token=same_token, seed=5 + bias + 2 * x_grad)


def test_graph_capture_recasts_the_masters_on_every_replay():
    """forward + backward captured once under bf16 autocast over fp32 masters; between replays the masters change in place (an
    optimizer step outside the graph): every replay equals an eager packed step on the CURRENT masters, so the cast to the compute
    copies runs inside the graph -- one cached across replays would keep the first step's weights"""
    T, M, E, k = 1024, 256, 16, 2
    amp = torch.bfloat16
    layer = make_layer(M, 256, E, k, 0.0, seed=9)
    layer.dropless_packed = True
    params = [p for _, p in _params(layer)]
    static_x = torch.randn(T, M, device="cuda")
    R = torch.randn(T, M, device="cuda") / 16

    def step():
        for p in params:
            p.grad = None
        with torch.autocast("cuda", dtype=amp):
            y = layer(static_x)
            loss = (y.float() * R).sum() + y.l_aux.float()
        loss.backward()
        return y, y.l_aux

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    assert layer._dropless_packed_ran is True, layer._dropless_packed_ran
    g = torch.cuda.CUDAGraph()
    for p in params:
        p.grad = None
    with torch.cuda.graph(g):
        sy, sl = step()
    sgrads = [p.grad for p in params]
    assert all(t.dtype == torch.float32 for t in sgrads)
    torch.manual_seed(1)
    batches = [torch.randn(T, M, device="cuda"), torch.randn(T, M, device="cuda") * 3,
               torch.randn(1, M, device="cuda").expand(T, M).contiguous()]   # all tokens on k experts
    caps = []
    for xb in batches:
        static_x.copy_(xb)
        g.replay()
        torch.cuda.synchronize()
        ry, rl, rg = sy.clone(), sl.clone(), [t.clone() for t in sgrads]
        ey, el = step()
        caps.append(int(layer.dropless_capacity))
        assert torch.equal(ry, ey) and torch.equal(rl, el)
        for a, p in zip(rg, params):
            assert torch.equal(a, p.grad)
        # the optimizer step, outside the graph; it must move the 16-bit compute copies, or the replay above proves nothing
        experts = list(layer.experts.parameters())
        before = [p.detach().to(amp) for p in experts]
        with torch.no_grad():
            for p in params:
                p.add_(p.grad, alpha=-0.05)
        assert all(not torch.equal(b, p.detach().to(amp)) for b, p in zip(before, experts))
    assert caps[2] == T and caps[0] < T and caps[1] < T, caps   # the maximum load differs: the last batch puts every token on k experts


def test_grad_scaler_fp16_packed_against_padded():
    """five SGD steps under fp16 autocast with a GradScaler: the loss curves of the packed and the padded path agree (the bar of
    test_sgd_loss_curves_agree) and the scaler ends at the same scale: the packed path skips no step the padded path takes"""
    torch.manual_seed(2)
    x = torch.randn(512, 128, device="cuda")
    losses, scales = {}, {}
    for packed in (False, True):
        layer = make_layer(128, 256, 8, 2, 0.0, seed=4)
        layer.dropless_packed = packed
        opt = torch.optim.SGD(layer.parameters(), lr=0.05)
        scaler = torch.amp.GradScaler("cuda")
        cur = []
        for _ in range(5):
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16):
                y = layer(x)
                loss = y.float().square().mean() + y.l_aux
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            cur.append(float(loss))
        assert layer._dropless_packed_ran is (True if packed else None), layer._dropless_packed_ran
        losses[packed], scales[packed] = cur, float(scaler.get_scale())
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 2 ** -7 * abs(a) + 1e-3, (losses[False], losses[True])
    assert scales[True] == scales[False], scales
