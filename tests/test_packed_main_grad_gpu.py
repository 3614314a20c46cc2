"""Accumulating the packed weight / bias gradients into an fp32 main_grad across micro-batches, on the MI355X: the accumulating
kernels bit for bit against D + G (G from the fp32-output kernels), against float64, the layer's switch against autograd's own
accumulation into p.grad, graph capture of one micro-step replayed over several batches, the refusals, and the switch left off."""
import contextlib

import pytest
import torch

from tutel_amd import ops
from tutel_amd.impls import packed_train

from _packed_fuzz import layout_from_rows
from test_packed_train_gpu import _params, _reference, _rel, make_layer

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 130]      # an empty expert, a single row, two full 64-row steps and a tail
NA, NB = 72, 200        # a partial tile below 128; a full tile and a partial one past 128


def _prefill(shape, seed):
    """random fp32 values, a quarter of them of magnitude ~1e6 (so that adding a gradient of order 1..100 rounds)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.randn(shape, device="cuda", generator=g)
    big = torch.rand(shape, device="cuda", generator=g) < 0.25
    return torch.where(big, d * 1e6, d)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_acc(fn, shape, empty, seed):
    """fn(out_dtype=...) / fn(accumulate_into=...): D_after == D_before + G bit for bit, the experts in `empty` untouched, run twice"""
    G = fn(out_dtype=torch.float32)
    assert G.shape == shape and G.dtype == torch.float32
    D0 = _prefill(shape, seed)
    for e in empty:
        D0[e].view(-1)[::3] = -0.0          # an add of +0.0 would turn these into +0.0: only an untouched slice keeps them
    D = D0.clone()
    ret = fn(accumulate_into=D)
    assert ret.data_ptr() == D.data_ptr() and ret.shape == D.shape
    assert torch.equal(D, D0 + G)
    assert not torch.equal(D, D0) and bool(((D0 + G) != D0 + G.double()).any())     # the pre-fill makes the fp32 add round
    for e in empty:
        assert bool((G[e] == 0).all())
        assert torch.equal(_bits(D[e]), _bits(D0[e]))
    D2 = D0.clone()
    fn(accumulate_into=D2)
    assert torch.equal(_bits(D2), _bits(D))
    # a flat target of the same size is taken as it is
    D3 = D0.clone().view(-1)
    fn(accumulate_into=D3)
    assert torch.equal(_bits(D3), _bits(D).view(-1))
    return G, D0, D


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_acc_kernels_bit_for_bit(dtype):
    torch.manual_seed(0)
    lay, _, _ = layout_from_rows(ROWS)
    E = len(ROWS)
    a = torch.randn(lay.rows_bound, NA, device="cuda").to(dtype)
    b = torch.randn(lay.rows_bound, NB, device="cuda").to(dtype)
    used = int(lay.offsets[-1])
    a[used:] = float("nan")      # rows past off[E]: never read
    b[used:] = float("nan")
    _check_acc(lambda **kw: ops.expert_wgrad_packed(a, b, lay, **kw), (E, NA, NB), [0], 1)
    _check_acc(lambda **kw: ops.expert_wgrad_packed(b, a, lay, **kw), (E, NB, NA), [0], 2)
    _check_acc(lambda **kw: ops.expert_bgrad_packed(b, lay, **kw), (E, NB), [0], 3)
    wide = torch.randn(lay.rows_bound, 520, device="cuda").to(dtype)                 # three blocks of 256 columns, the last partial
    wide[used:] = float("nan")
    _check_acc(lambda **kw: ops.expert_bgrad_packed(wide, lay, **kw), (E, 520), [0], 4)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_acc_kernel_gathered_operands(dtype):
    """either operand read through a slot map with -1 pad rows (alignment 8: 0, 1, 130 rows become 0, 8, 136)"""
    torch.manual_seed(1)
    lay, idx, _ = layout_from_rows(ROWS, align=8)
    smap = lay.slot_map[:int(lay.offsets[-1])]
    assert int((smap < 0).sum()) == 7 + 6 and int((smap >= 0).sum()) == sum(ROWS)
    E, T = len(ROWS), idx.shape[1]
    x_a = torch.randn(T, NA, device="cuda").to(dtype)
    x_b = torch.randn(T, NB, device="cuda").to(dtype)
    a = torch.randn(lay.rows_bound, NA, device="cuda").to(dtype)
    b = torch.randn(lay.rows_bound, NB, device="cuda").to(dtype)
    zero = torch.zeros(max(NA, NB), device="cuda", dtype=dtype)
    _check_acc(lambda **kw: ops.expert_wgrad_packed(x_a, b, lay, gather="a", zero_row=zero, **kw), (E, NA, NB), [0], 5)
    G, _, _ = _check_acc(lambda **kw: ops.expert_wgrad_packed(a, x_b, lay, gather="b", zero_row=zero, **kw), (E, NA, NB), [0], 6)
    # the gathered G is the product over a materialised packed copy (pad rows zero)
    xp = torch.zeros(lay.rows_bound, NB, device="cuda", dtype=dtype)
    ok = lay.slot_map >= 0
    xp[ok] = x_b[(lay.slot_map[ok] % T).long()]
    assert torch.equal(G, ops.expert_wgrad_packed(a, xp, lay, out_dtype=torch.float32))


def test_two_accumulations_keep_the_order():
    torch.manual_seed(2)
    dtype = torch.bfloat16
    lays = [layout_from_rows(r)[0] for r in (ROWS, [130, 0, 1])]
    ops_ = []
    for lay in lays:
        a = torch.randn(lay.rows_bound, NA, device="cuda").to(dtype)
        b = torch.randn(lay.rows_bound, NB, device="cuda").to(dtype)
        ops_.append((a, b, lay))
    D0 = _prefill((3, NA, NB), 7)
    d0 = _prefill((3, NB), 8)
    G = [ops.expert_wgrad_packed(a, b, lay, out_dtype=torch.float32) for a, b, lay in ops_]
    g = [ops.expert_bgrad_packed(b, lay, out_dtype=torch.float32) for _, b, lay in ops_]
    D, d = D0.clone(), d0.clone()
    for a, b, lay in ops_:
        ops.expert_wgrad_packed(a, b, lay, accumulate_into=D)
        ops.expert_bgrad_packed(b, lay, accumulate_into=d)
    assert torch.equal(D, (D0 + G[0]) + G[1])
    assert torch.equal(d, (d0 + g[0]) + g[1])


def test_three_accumulated_batches_against_float64():
    torch.manual_seed(3)
    dtype = torch.bfloat16
    E, Na, Nb = 8, 136, 200
    batches = [[40, 300, 128, 77, 193, 64, 257, 101], [300, 41, 65, 250, 63, 129, 90, 200], [99, 100, 288, 45, 160, 222, 70, 131]]
    D = torch.zeros(E, Na, Nb, device="cuda")
    d = torch.zeros(E, Nb, device="cuda")
    ref = torch.zeros(E, Na, Nb, device="cuda", dtype=torch.float64)
    dref = torch.zeros(E, Nb, device="cuda", dtype=torch.float64)
    for rows in batches:
        lay, _, _ = layout_from_rows(rows)
        off = lay.offsets.cpu()
        a = torch.randn(lay.rows_bound, Na, device="cuda").to(dtype)
        b = torch.randn(lay.rows_bound, Nb, device="cuda").to(dtype)
        ops.expert_wgrad_packed(a, b, lay, accumulate_into=D)
        ops.expert_bgrad_packed(b, lay, accumulate_into=d)
        for e in range(E):
            r0, r1 = int(off[e]), int(off[e + 1])
            assert r1 - r0 == rows[e]
            ref[e] += a[r0:r1].double().t() @ b[r0:r1].double()
            dref[e] += b[r0:r1].double().sum(0)
    print("rel wgrad", _rel(D, ref), "rel bgrad", _rel(d, dref))
    assert _rel(D, ref) <= 2 ** -7
    assert _rel(d, dref) <= 2 ** -7


# ---- layer ---------------------------------------------------------------------------------------------------------------------
T, M, H, E, K = 333, 128, 192, 8, 2
EXPERT = ("w1", "b1", "w2", "b2")


def _batches(n, dtype, seed):
    torch.manual_seed(seed)
    xs = [(torch.randn(T, M, device="cuda") * (1 + i)).to(dtype) for i in range(n)]
    Rs = [torch.randn(T, M, device="cuda") for _ in range(n)]
    return xs, Rs


def _micro_steps(layer, xs, Rs, amp, main_grad, packed=True):
    """the micro-steps of one optimizer step: gradients accumulate in p.grad (autograd) or, with the switch, in p.main_grad"""
    layer.dropless_packed = packed
    layer.dropless_packed_main_grad = main_grad
    layer.zero_grad(set_to_none=True)
    outs = []
    for x, R in zip(xs, Rs):
        xi = x.clone().requires_grad_(True)
        with (torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()):
            y = layer(xi)
            loss = (y.float() * R).sum() + y.l_aux.float()
        loss.backward()
        outs.append({"y": y.detach().clone(), "l_aux": y.l_aux.detach().clone(), "cnt": layer.dispatch_count.clone(),
                     "x": xi.grad.detach().clone(), "ran": layer._dropless_packed_ran,
                     "routing": tuple(t.clone() for t in layer.last_routing)})
    return outs


def _same_outputs(a, b):
    for sa, sb in zip(a, b):
        for n in ("y", "l_aux", "cnt", "x"):
            assert torch.equal(sa[n], sb[n]), n


def test_layer_fp32_masters_under_autocast():
    layer = make_layer(M, H, E, K, 0.0, torch.float32, seed=21)
    xs, Rs = _batches(3, torch.float32, 22)
    P = dict(_params(layer))
    A = _micro_steps(layer, xs, Rs, torch.bfloat16, False)
    assert all(s["ran"] is True for s in A)
    grads = {n: p.grad.detach().clone() for n, p in P.items()}
    assert all(grads[n].dtype == torch.float32 for n in EXPERT)
    packed_train.attach_main_grads(layer)
    B = _micro_steps(layer, xs, Rs, torch.bfloat16, True)
    assert all(s["ran"] is True for s in B)
    _same_outputs(A, B)
    assert torch.equal(P["wg"].grad, grads["wg"]) and not hasattr(P["wg"], "main_grad")
    for n in EXPERT:
        assert P[n].grad is None, n
        assert P[n].grad_added_to_main_grad is True, n
        assert float(grads[n].abs().max()) > 0
        assert torch.equal(P[n].main_grad, grads[n]), n          # the same fp32 adds in the same order
    # a second optimizer step accumulates from zero again
    packed_train.zero_main_grads(layer)
    assert all(P[n].grad_added_to_main_grad is False for n in EXPERT)
    _micro_steps(layer, xs, Rs, torch.bfloat16, True)
    for n in EXPERT:
        assert torch.equal(P[n].main_grad, grads[n]), n


def test_layer_bf16_parameters_accumulate_in_fp32():
    layer = make_layer(M, H, E, K, 0.0, torch.bfloat16, seed=23)
    xs, Rs = _batches(3, torch.bfloat16, 24)
    P = dict(_params(layer))
    A = _micro_steps(layer, xs, Rs, None, False)
    grads = {n: p.grad.detach().clone() for n, p in P.items()}
    assert all(grads[n].dtype == torch.bfloat16 for n in EXPERT)
    packed_train.attach_main_grads(layer)
    B = _micro_steps(layer, xs, Rs, None, True)
    assert all(s["ran"] is True for s in A + B)
    _same_outputs(A, B)
    assert torch.equal(P["wg"].grad, grads["wg"])
    ref = None
    for x, R, s in zip(xs, Rs, B):
        r = _reference(layer, x, R, s["routing"][0], s["routing"][1], 1 << 30)
        ref = r if ref is None else {n: ref[n] + r[n] for n in r}
    for n in EXPERT:
        assert P[n].grad is None and P[n].grad_added_to_main_grad is True, n
        assert P[n].main_grad.dtype == torch.float32
        e_main, e_grad = _rel(P[n].main_grad, ref[n]), _rel(grads[n], ref[n])
        print(n, "main_grad", e_main, "16-bit p.grad", e_grad)
        assert e_main <= 2 ** -7, (n, e_main)
        assert e_main <= e_grad, (n, e_main, e_grad)      # the fp32 sum is no further from fp64 than the 16-bit one


def test_graph_capture_of_one_micro_step_replayed_over_batches():
    Tg, Mg, Eg = 1024, 256, 16
    layer = make_layer(Mg, 256, Eg, 2, 0.0, torch.bfloat16, seed=9)
    layer.dropless_packed = True
    layer.dropless_packed_main_grad = True
    packed_train.attach_main_grads(layer)
    P = dict(_params(layer))
    static_x = torch.randn(Tg, Mg, device="cuda").to(torch.bfloat16)

    def step():
        P["wg"].grad = None
        y = layer(static_x)
        loss = y.float().square().mean() + y.l_aux.float()
        loss.backward()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    assert layer._dropless_packed_ran is True
    g = torch.cuda.CUDAGraph()
    P["wg"].grad = None
    with torch.cuda.graph(g):
        step()
    ptrs = {n: P[n].main_grad.data_ptr() for n in EXPERT}
    torch.manual_seed(1)
    batches = [torch.randn(Tg, Mg, device="cuda").to(torch.bfloat16),
               (torch.randn(Tg, Mg, device="cuda") * 3).to(torch.bfloat16),
               torch.randn(1, Mg, device="cuda").to(torch.bfloat16).expand(Tg, Mg).contiguous()]   # all tokens on k experts
    packed_train.zero_main_grads(layer)       # the warm-up and the capture accumulated too
    for xb in batches:
        static_x.copy_(xb)
        g.replay()
    torch.cuda.synchronize()
    replayed = {n: P[n].main_grad.clone() for n in EXPERT}
    wg_replayed = P["wg"].grad.clone()
    packed_train.zero_main_grads(layer)
    for xb in batches:
        static_x.copy_(xb)
        step()
    for n in EXPERT:
        assert P[n].main_grad.data_ptr() == ptrs[n] and P[n].grad is None
        assert float(replayed[n].abs().max()) > 0
        assert torch.equal(replayed[n], P[n].main_grad), n
    assert torch.equal(wg_replayed, P["wg"].grad)       # the router's ordinary gradient: the last batch's


def _expect_raise(layer, x, why):
    P = dict(_params(layer))
    before = {n: P[n].main_grad.clone() for n in EXPERT if hasattr(P[n], "main_grad")}
    layer.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match=why) as ei:
        layer(x.clone().requires_grad_(True))
    for n, p in P.items():
        assert p.grad is None, n
        if n in before:
            assert torch.equal(_bits(p.main_grad), _bits(before[n])), n
    return str(ei.value)


def test_refusals_raise_instead_of_the_padded_step():
    x = torch.randn(T, M, device="cuda").to(torch.bfloat16)
    layer = make_layer(M, H, E, K, 0.0, torch.bfloat16, seed=25)
    layer.dropless_packed = True
    layer.dropless_packed_main_grad = True
    _expect_raise(layer, x, "main_grad")
    assert "no main_grad" in layer._dropless_packed_ran
    packed_train.attach_main_grads(layer)
    for p in layer.experts.parameters():
        p.main_grad.fill_(1.5)
    layer.is_postscore = False
    msg = _expect_raise(layer, x, "is_postscore")
    assert packed_train.unsupported(layer, layer.gates[0], T, E, K, M, torch.bfloat16, 0.0, 1) in msg
    layer.is_postscore = True
    layer.experts.batched_fc2_w.main_grad = layer.experts.batched_fc2_w.main_grad.to(torch.bfloat16)
    _expect_raise(layer, x, "main_grad.*bfloat16")


def test_switch_off_ignores_attached_main_grads():
    """attributes alone change nothing: with the switch off, a step after attach_main_grads equals a step before it, bit for bit"""
    xs, Rs = _batches(1, torch.float32, 26)
    for dtype, amp in ((torch.float32, torch.bfloat16), (torch.bfloat16, None)):
        layer = make_layer(M, H, E, K, 0.0, dtype, seed=27)
        x = [xs[0].to(dtype)]
        P = dict(_params(layer))
        before = _micro_steps(layer, x, Rs, amp, False)
        grads = {n: p.grad.detach().clone() for n, p in P.items()}
        packed_train.attach_main_grads(layer)
        after = _micro_steps(layer, x, Rs, amp, False)
        assert before[0]["ran"] is True and after[0]["ran"] is True
        _same_outputs(before, after)
        for n, p in P.items():
            assert torch.equal(p.grad, grads[n]), n
        for n in EXPERT:
            assert int((P[n].main_grad != 0).sum()) == 0 and P[n].grad_added_to_main_grad is False
