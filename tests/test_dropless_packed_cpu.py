"""The packed dropless layout without a GPU: the host bound of tutel_amd_packed_plan (rows, tiles, workspace bytes) against the exact
need of adversarial routings, the new entry points on the C-ABI boundary, and argument errors reported before anything is enqueued."""
import ctypes
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 256


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def _plan(L, T, E, k, limit, al, M=256, H=256, Mo=256, dtype=2):
    from tutel_amd import _lib
    p = _lib.PackedPlan()
    rc = L.tutel_amd_packed_plan(T, E, k, M, H, Mo, dtype, limit, al, ctypes.byref(p))
    return rc, p


def _exact(counts, limit, al, H=256, Mo=256):
    """rows / tiles / workspace bytes one routing needs (the layout of csrc/dropless.hip, computed independently)"""
    Lr = -(-limit // al) * al if limit > 0 else None
    rows_e = []
    for c in counts:
        kept = min(c, Lr) if Lr is not None else c
        rows_e.append(-(-kept // al) * al)
    rows = sum(rows_e)
    tiles = sum(-(-r // TILE) for r in rows_e)
    a = lambda b: -(-b // 256) * 256
    return rows, tiles, a(rows * 4) + a(tiles * 8) + 256 + a(rows * H * 2) + a(rows * Mo * 2), max(rows_e + [0])


def _adversarial(T, E, k):
    """count vectors a top-k routing of T tokens over E experts can produce (each expert <= T, sum k*T)"""
    n = k * T
    out = []
    out.append([T] * k + [0] * (E - k))                                  # every token on the same k experts
    q, r = divmod(n, E)
    out.append([q + (1 if e < r else 0) for e in range(E)])              # as even as possible (one per expert when k*T <= E)
    if n >= E:                                                           # one row for all but a few, the rest piled on k experts
        rest = n - (E - k)
        pile = [min(T, rest // k + (1 if i < rest % k else 0)) for i in range(k)]
        spill = rest - sum(pile)
        v = pile + [1] * (E - k)
        i = k
        while spill > 0:
            add = min(spill, T - v[i])
            v[i] += add
            spill -= add
            i += 1
        out.append(v)
    # counts just past a multiple of the tile / the alignment: every expert one row into a new tile
    v, left = [0] * E, n
    for e in range(E):
        take = min(T, left, TILE + 1)
        v[e], left = take, left - take
    if left == 0:
        out.append(v)
    return [c for c in out if sum(c) == n and max(c) <= T and len(c) == E]


@pytest.mark.parametrize("al", [1, 4, 128])
def test_host_bound_covers_every_adversarial_routing(L, al):
    for T, E, k in itertools.product([1, 3, 127, 300, 1000, 4096], [8, 64, 128], [1, 2, 4]):
        spe = -(-T // E)
        for limit in [0, k * int(1.0 * spe), k * int(0.3 * spe), 1]:
            rc, p = _plan(L, T, E, k, limit, al)
            assert rc == 0, L.tutel_amd_last_error()
            assert p.tile_rows == TILE
            assert L.tutel_amd_moe_packed_workspace_bytes(T, E, k, 256, 256, 256, 2, limit, al) == p.ws_bytes
            for counts in _adversarial(T, E, k):
                rows, tiles, ws, cap = _exact(counts, limit, al)
                assert rows <= p.rows_bound and tiles <= p.tiles_bound and ws <= p.ws_bytes, (T, E, k, limit, al, counts[:8])


def test_bound_is_tight_for_its_worst_cases(L):
    # one token per expert (k*T <= E): every expert that holds a row pads to the alignment, and the bound is exactly that
    rc, p = _plan(L, 4, 64, 2, 0, 4)
    assert rc == 0 and p.rows_bound == 8 * 4 and _exact([1] * 8 + [0] * 56, 0, 4)[0] == p.rows_bound
    # the headline dropless shape (configs[2]): 8192 entries + 64 x 3 pad rows, 32 full tiles + one partial tile per expert
    rc, p = _plan(L, 4096, 64, 2, 0, 4, M=2048, H=2048, Mo=2048)
    assert rc == 0 and (p.rows_bound, p.tiles_bound, p.row_limit) == (8192 + 64 * 3, 32 + 64, 0)
    # a limit: no expert keeps more than round_up(limit, alignment) rows
    rc, p = _plan(L, 4096, 64, 2, 10, 4)
    assert rc == 0 and p.row_limit == 12 and p.rows_bound == 64 * 12


def test_uncovered_shapes_answer_enotsup(L):
    from tutel_amd import _lib
    cases = [dict(dtype=0), dict(M=100), dict(H=64), dict(Mo=120), dict(H=96)]
    for kw in cases:
        rc, _ = _plan(L, 128, 8, 2, 0, 1, **kw)
        assert rc == _lib.ENOTSUP and b"not covered" in L.tutel_amd_last_error(), kw
    assert _plan(L, 128, 8, 17, 0, 1)[0] == _lib.ENOTSUP             # k > 16
    assert _plan(L, 128, 8192, 2, 0, 1)[0] == _lib.ENOTSUP           # E > 4096
    assert L.tutel_amd_moe_packed_workspace_bytes(128, 8, 2, 256, 256, 256, 0, 0, 1) == 0
    assert _plan(L, -1, 8, 2, 0, 1)[0] not in (0, _lib.ENOTSUP)      # bad sizes are errors
    assert _plan(L, 128, 8, 2, 0, 0)[0] not in (0, _lib.ENOTSUP)


def test_entry_points_declared_exported_bound(L):
    from tutel_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tutel_amd.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tutel_amd_moe_forward_packed", "tutel_amd_moe_packed_workspace_bytes", "tutel_amd_packed_plan"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(raw, name)
    assert "TUTEL_AMD_ABI_VERSION 1" in hdr and L.tutel_amd_abi_version() == 1
    # the ctypes mirrors of the two new structs have the C layout (pointer / size_t fields at natural alignment)
    assert ctypes.sizeof(_lib.PackedArgs) == 32 and ctypes.sizeof(_lib.PackedPlan) == 24


def test_forward_packed_rejects_bad_arguments_before_enqueueing(L):
    from tutel_amd import _lib
    m, pk = _lib.MoeArgs(), _lib.PackedArgs()
    a = m.ep
    a.T, a.M, a.H, a.M_out, a.num_experts, a.world, a.k, a.dtype = 64, 256, 256, 256, 8, 1, 2, _lib.BF16
    a.is_postscore, a.w2_kmajor = 1, 1
    m.alignment, m.logits_dtype = 1, _lib.BF16
    fake = ctypes.c_void_p(0x10000)   # never dereferenced on the host, and nothing may reach the device
    assert L.tutel_amd_moe_forward_packed(None, None, ctypes.byref(pk), None) != 0
    assert L.tutel_amd_moe_forward_packed(fake, ctypes.byref(m), ctypes.byref(pk), None) != 0
    assert b"single rank" in L.tutel_amd_last_error()
    a.world = 2
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) != 0 and b"single rank" in L.tutel_amd_last_error()
    a.world = 1
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) != 0 and b"null" in L.tutel_amd_last_error()
    pk.offsets = pk.capacity = m.dispatch_count = m.ws = fake
    pk.ws, pk.ws_bytes = fake, 16
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) != 0
    assert b"workspace too small" in L.tutel_amd_last_error()
    pk.ws_bytes = L.tutel_amd_moe_packed_workspace_bytes(64, 8, 2, 256, 256, 256, _lib.BF16, 0, 1)
    m.logits = fake
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) != 0 and b"null" in L.tutel_amd_last_error()
    a.x = a.idx = a.loc = a.gates = a.w1 = a.w2 = a.y = a.zero_row = fake
    m.ws_bytes = 1   # routing workspace
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) != 0 and b"routing workspace" in L.tutel_amd_last_error()
    m.ws_bytes = 1 << 20
    a.x = ctypes.c_void_p(0x10008)
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) != 0 and b"aligned" in L.tutel_amd_last_error()
    # shapes the layout does not cover: TUTEL_AMD_ENOTSUP, nothing launched
    a.x, a.is_postscore = fake, 0
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) == _lib.ENOTSUP
    a.is_postscore, a.w2_kmajor = 1, 0
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) == _lib.ENOTSUP
    a.w2_kmajor, a.H = 1, 64
    assert L.tutel_amd_moe_forward_packed(None, ctypes.byref(m), ctypes.byref(pk), None) == _lib.ENOTSUP


def test_python_plan_mirror(L):
    from tutel_amd.impls import ep_native
    import torch
    plan, why = ep_native.packed_plan(4096, 64, 2, 2048, 2048, 2048, torch.bfloat16, 0, 4)
    assert why is None and plan["rows_bound"] == 8384 and plan["tile_rows"] == 256
    plan, why = ep_native.packed_plan(64, 8, 2, 256, 256, 256, torch.float32, 0, 1)
    assert plan is None and "16-bit" in why
