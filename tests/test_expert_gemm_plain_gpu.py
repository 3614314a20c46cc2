"""The PLAIN form of the 128 x 256 ring GEMM kernel (csrc/expert_gemm_plain.hip) against the general kernel it stands in for: the same
launch with the switch off (tutel_amd_gemm_plain(0)) and on (1) must write the same bits -- the K loop, the rotation and the epilogue
arithmetic are shared, only the address arithmetic around them differs -- and tutel_amd_expert_gemm_last_form must name the kernel
that ran.  Every operand and the output sit inside guard bands (tests/_packed_fuzz.py).  Launches the predicate does not admit keep
the general kernel, and their bits, whatever the switch says."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _packed_fuzz import OUT_FILL, moat_intact, moated  # noqa: E402

pytestmark = pytest.mark.gpu
GENERAL, PLAIN = 0, 1
# (E, R, N, K): one K-tile (the prologue's `t < nk` guards); two N-tiles and three K-tiles; rows past R; 256 blocks (no-allocate weight loads)
SHAPES = [(3, 128, 256, 64), (5, 128, 512, 192), (7, 72, 256, 128), (64, 128, 1024, 64)]


def _operands(E, R, N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn([E, R, K], generator=g).to(dtype)
    w = ((torch.rand([E, N, K], generator=g) * 2 - 1) / 8).to(dtype)
    b = torch.randn([E, N], generator=g).to(dtype)
    return moated(a, device="cuda"), moated(w, device="cuda"), moated(b, device="cuda")


def _slot_map(E, R, T, seed):
    """slots up to 2 T - 1 (the second choice of a token), -1 entries (empty slots: the zero row)"""
    rnd = np.random.default_rng(seed)
    s = rnd.integers(0, 2 * T, E * R).astype(np.int32)
    s[rnd.random(E * R) < 0.2] = -1
    s[0], s[-1], s[1] = 2 * T - 1, -1, 0
    return torch.from_numpy(s)


def _both(run, want_plain=True):
    """run() with the switch off and on -> the two outputs; the form query must name the kernel each time"""
    from tutel_amd import ops
    was = ops.gemm_plain(-2)
    outs = []
    try:
        for mode in (0, 1):
            ops.gemm_plain(mode)
            n0 = ops.expert_gemm_last_form()[1]
            outs.append(run())
            form, n1 = ops.expert_gemm_last_form()
            plain = bool(mode) and want_plain
            assert form == (PLAIN if plain else GENERAL), (mode, form)
            assert [n1[0] - n0[0], n1[1] - n0[1]] == ([0, 1] if plain else [1, 0]), (mode, n0, n1)
    finally:
        ops.gemm_plain(was)
    torch.cuda.synchronize()
    return outs


def _forced_ring():
    from tutel_amd import _lib, ops
    ops.set_option(_lib.OPT_GEMM_IMPL, 4)     # the small grids do not cover the chip: the ring kernel by request


def _auto():
    from tutel_amd import _lib, ops
    ops.set_option(_lib.OPT_GEMM_IMPL, -1)
    ops.set_option(_lib.OPT_GEMM_STORE, -1)


ACTS = {0: ["none", "relu", "gelu"], 1: ["none", "relu", "silu"], 2: ["none", "relu"], 3: ["none", "relu"]}   # gelu and silu once each


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_plain_rows_keep_every_bit(si, dtype):
    from tutel_amd import ops
    E, R, N, K = SHAPES[si]
    a, w, b = _operands(E, R, N, K, dtype, 100 + si)
    try:
        _forced_ring()
        for act in ACTS[si] if dtype == torch.bfloat16 else ["none", "relu"]:
            for bias in (b, None):
                def run():
                    out = moated(torch.full([E, R, N], OUT_FILL).to(dtype), fill=OUT_FILL, device="cuda")
                    ops.expert_gemm(a, w, bias, True, act=act, out=out, d_layout=(R * N, 0, R, N))
                    return out
                o0, o1 = _both(run)
                assert torch.equal(o0, o1), (act, bias is not None)
                for o in (o0, o1):
                    moat_intact(o, "the output")
                    assert not bool((o == OUT_FILL).all(dim=-1).any()), "every row of every expert is written"
        # against fp32 arithmetic, so that two equal outputs are also right ones
        ref = torch.relu(torch.matmul(a.float(), w.float().transpose(1, 2)) + b.float().unsqueeze(1))
        got = _both(lambda: ops.expert_gemm(a, w, b, True, act="relu"))[1].float()
        ulp = 2 ** -7 if dtype == torch.bfloat16 else 2 ** -10
        assert bool(((got - ref).abs() <= ulp * ref.abs() + 2e-3).all())
        for t in (a, w, b):
            moat_intact(t)
    finally:
        _auto()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_gathered_rows_keep_every_bit(si, dtype):
    """rows gathered through a slot map (fused fast_encode): -1 entries read the zero row, slots up to 2 T - 1 name token q % T"""
    from tutel_amd import _lib, ops
    E, R, N, K = SHAPES[si]
    T = 200
    _, w, b = _operands(E, R, N, K, dtype, 200 + si)
    x = moated(torch.randn([T, K], generator=torch.Generator().manual_seed(si)).to(dtype), device="cuda")
    smap = moated(_slot_map(E, R, T, 300 + si), fill=0, device="cuda")
    try:
        _forced_ring()
        for act, bias in (("relu", b), ("none", None)):
            for gather_opt in (-1, 0):      # slot-map entries through the scalar cache, or as vector loads
                ops.set_option(_lib.OPT_GEMM_GATHER, gather_opt)
                o0, o1 = _both(lambda: ops.expert_gemm_gather(x, smap, w, bias, True, act, R))
                assert torch.equal(o0, o1), (act, gather_opt)
        q = smap.cpu().long()
        rows = torch.where((q >= 0).unsqueeze(1), x.cpu().float()[q.clamp(min=0) % T], torch.zeros(1, K)).view(E, R, K)
        ref = torch.matmul(rows, w.cpu().float().transpose(1, 2))
        ulp = 2 ** -7 if dtype == torch.bfloat16 else 2 ** -10
        assert bool(((o1.cpu().float() - ref).abs() <= ulp * ref.abs() + 2e-3).all())
        for t in (x, smap, w, b):
            moat_intact(t)
    finally:
        ops.set_option(_lib.OPT_GEMM_GATHER, -1)
        _auto()


def test_launches_that_are_not_admitted_keep_the_general_kernel():
    """an exchange layout (rows of two source ranks: a_rpw < R, d_rpw < R), row counts, a gating operand, store policies 0 and 2: the
    general kernel, unchanged bits, whatever the switch says"""
    from tutel_amd import _lib, ops
    E, R, N, K = 5, 128, 512, 192
    dtype = torch.bfloat16
    a, w, b = _operands(E, R, N, K, dtype, 7)
    half = R // 2
    counts = torch.tensor([(R * (e + 1)) // (E + 1) for e in range(E)], dtype=torch.int32).cuda()
    mul = torch.randn([E, R, N], generator=torch.Generator().manual_seed(5)).to(dtype).cuda()

    def full(v=7.0, shape=(E, R, N)):
        return torch.full(shape, v, dtype=dtype).cuda()
    try:
        _forced_ring()
        cases = {
            "a_rpw < R": lambda: ops.expert_gemm(a, w, b, True, act="relu", E_loc=E, R=R, a_layout=(R * K, half * K, half, K)),
            "d_rpw < R": lambda: ops.expert_gemm(a, w, b, True, act="relu", out=full(shape=(2, E, half + 1, N)),
                                                 d_layout=((half + 1) * N, E * (half + 1) * N, half, N)),
            "row_counts": lambda: ops.expert_gemm(a, w, b, True, act="relu", out=full(), d_layout=(R * N, 0, R, N), row_counts=counts, row_align=32),
            "mul": lambda: ops.expert_gemm(a, w, None, True, mul=mul),
        }
        want = _both(lambda: ops.expert_gemm(a, w, b, True, act="relu"))[0]
        for name, run in cases.items():
            o0, o1 = _both(run, want_plain=False)
            assert torch.equal(o0, o1), name
        assert torch.equal(_both(cases["a_rpw < R"], want_plain=False)[1], want)
        for store in (0, 2):
            ops.set_option(_lib.OPT_GEMM_STORE, store)
            o0, o1 = _both(lambda: ops.expert_gemm(a, w, b, True, act="relu"), want_plain=False)
            assert torch.equal(o0, o1) and torch.equal(o1, want), store
    finally:
        _auto()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_fused_location_forward_keeps_every_bit(oracle, dtype):
    """the one-call forward whose fc1 computes the locations itself (the FL instantiation): T = 256, M = 128, H = 256, E = 8, k = 2,
    capacity 64.  Switch off and on: y, idx, loc, the slot map, dispatch_count and l_aux bit for bit; a batch that overflows one expert's
    capacity; three HIP-graph replays."""
    from test_layer_gpu import make_layer
    from tutel_amd import _lib, ops
    from tutel_amd.impls.graph import GraphedForward
    T, M, H, E, k = 256, 128, 256, 8, 2
    x, *weights = oracle.make_problem(T, M, H, E, dtype=dtype, seed=61)
    layer = make_layer(M, H, E, k, 1.0, dtype, weights).eval()
    layer._keep_routing = True
    x_over = x.clone()
    x_over[: T // 2] = x[3]                # half the batch is one token: its two experts get 128 entries each, capacity 64
    was = ops.gemm_plain(-2)
    got = {}
    try:
        _forced_ring()
        for mode in (0, 1):
            ops.gemm_plain(mode)
            for name, xb in (("batch", x), ("overflow", x_over)):
                xd = xb.cuda()
                layer.__dict__.pop("_ep_workspaces", None)
                n0 = ops.expert_gemm_last_form()[1]
                ops.stage_timing(1)
                with torch.no_grad():
                    y = layer(xd)
                torch.cuda.synchronize()
                rep = ops.stage_report()
                ops.stage_timing(0)
                n1 = ops.expert_gemm_last_form()[1]
                assert rep["location"][1] == 0, "the fused-location route ran"
                # fc1 (N = H = 256) is admitted, fc2 (N = M = 128) takes a 128 x 128 kernel
                assert [n1[0] - n0[0], n1[1] - n0[1]] == ([1, 1] if mode else [2, 0]), (mode, n0, n1)
                ws = list(layer._ep_workspaces.values())[0]
                C = int(layer.protected_shape[1])
                assert C == 64
                got[mode, name] = dict(y=y.clone(), l_aux=y.l_aux.clone(), cnt=layer.dispatch_count.clone(), idx=layer.last_routing[0].clone(),
                                       loc=layer.last_routing[1].clone(), smap=ws.slot_map[:E * C].clone())
            with torch.no_grad():
                gf = GraphedForward(layer, x.cuda())
                got[mode, "replays"] = [gf(x.cuda()).clone() for _ in range(3)]
    finally:
        ops.stage_timing(0)
        ops.gemm_plain(was)
        _auto()
    for name in ("batch", "overflow"):
        for field in ("y", "l_aux", "cnt", "idx", "loc", "smap"):
            assert torch.equal(got[0, name][field], got[1, name][field]), (name, field)
    assert int((got[1, "overflow"]["loc"] >= 64).sum()) >= 64, "one expert's capacity overflows"
    for r0, r1 in zip(got[0, "replays"], got[1, "replays"]):
        assert torch.equal(r0, got[0, "batch"]["y"]) and torch.equal(r1, got[1, "batch"]["y"])
