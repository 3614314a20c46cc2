"""Seeded fuzzers of the packed dropless kernels (csrc/dropless.hip, the PACKED grouped GEMMs, csrc/packed_train.hip, the packed decode /
gate gradient of csrc/dispatch.hip), each a `run_*` function returning its failing cases.  Every reference is computed on the CPU from
the operation's definition (tests/_packed_fuzz.py: integer arithmetic for the layout, float64 for the products, the CPU oracle's decode
over the rows laid out padded on the host) on the same rounded inputs -- never the padded kernels, which share their bodies with the
packed ones.  No case is skipped: the generators draw only shapes the entry points cover, and a refusal is a failure.
  layout   ops.packed_layout: offsets, capacity, live tile count, tile table, slot map bit for bit; nothing written past the live tiles
  gemm     ops.expert_gemm_packed vs fp64 (both weight layouts, every activation, bias / gating operand / gather, N from 8), GEMM bar
  grad     ops.expert_wgrad_packed / expert_bgrad_packed vs fp64 with derived bounds
  decode   ops.fast_decode_packed (bit for bit), ops.gate_grad_packed, and the encode through the packed slot map (bit for bit)
  layer    whole dropless layers with dropless_packed (ffn ReLU / GELU / SiLU and SwiGLU experts, megablocks, negative factors, graph replays) vs the oracle
The gemm and grad fuzzers keep every operand in a guard band (F.moated: NaN around inputs, a sentinel around `out=` / `accumulate_into=`,
a valid entry naming a NaN token row around the slot map): a read or store next to an operand fails an assertion.  The forms a SwiGLU
training step needs (n-major gathered, real routings, wide gradients) have their own fuzzer, tests/test_packed_train_forms_gpu.py.
The default run takes 60 cases each, --runslow 600; `python tests/test_packed_fuzz_gpu.py [cases] [seed] [what]` runs any length and
writes packed_<what>_fuzz_<seed>.json beside the records of tests/test_fuzz_gpu.py (the repository's ignored `*_out/` directory)."""
import json
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _packed_fuzz as F   # noqa: E402

DEFAULT_CASES = 60
SEEDS = {"layout": 7070, "gemm": 7071, "grad": 7072, "decode": 7073, "layer": 7074}


def _fail(bad, tag, ex, verbose):
    bad.append(tag + " :: " + (str(ex) or type(ex).__name__)[:300].replace("\n", " "))
    if verbose:
        print("FAIL", bad[-1], flush=True)


def _plan(T, E, k, limit, align):
    from tutel_amd.impls import ep_native
    plan, why = ep_native.packed_plan(T, E, k, 128, 128, 128, torch.bfloat16, limit, align)
    assert plan is not None, f"the plan refuses a drawn case: {why}"
    return plan


def _sentinel_layout(E, plan, device="cuda"):
    from tutel_amd import ops
    lay = ops.PackedLayout(E, plan["rows_bound"], plan["tiles_bound"], plan["row_limit"], device)
    for t in (lay.offsets, lay.tiles, lay.ntiles, lay.capacity, lay.slot_map):
        t.fill_(F.SENTINEL)
    return lay


def _check_layout(lay, ref, plan, idx, loc, T):
    """the device tables against the reference, bit for bit, and the property the decode relies on"""
    rb, tb = plan["rows_bound"], plan["tiles_bound"]
    off = lay.offsets.cpu().numpy().astype(np.int64)
    assert np.array_equal(off, ref["offsets"]), f"offsets differ first at {int(np.nonzero(off != ref['offsets'])[0][0])}"
    assert int(lay.capacity) == ref["capacity"], f"capacity {int(lay.capacity)} vs {ref['capacity']}"
    assert int(lay.ntiles) == ref["ntiles"], f"ntiles {int(lay.ntiles)} vs {ref['ntiles']}"
    assert ref["ntiles"] <= tb and int(ref["offsets"][-1]) <= rb, "the reference layout exceeds the plan's bounds"
    tiles = lay.tiles.cpu().numpy().astype(np.int64).reshape(-1, 2)
    nt = ref["ntiles"]
    assert np.array_equal(tiles[:nt], ref["tiles"]), "tile table"
    assert bool((tiles[nt:] == F.SENTINEL).all()), "a tile-table entry at or past ntiles was written"
    slot = lay.slot_map.cpu().numpy().astype(np.int64)
    assert slot.size == max(rb, 1)
    if rb > 0:
        diff = np.nonzero(slot[:rb] != ref["slot"])[0]
        assert diff.size == 0, f"slot map differs in {diff.size} rows, first row {int(diff[0])}: {int(slot[diff[0]])} vs {int(ref['slot'][diff[0]])}"
    # every kept entry (j, t) is named by row offsets[idx] + loc, and by no other row
    fi, fl = idx.reshape(-1).astype(np.int64), loc.reshape(-1).astype(np.int64)
    q = np.nonzero(ref["keep"].reshape(-1))[0]
    assert np.array_equal(slot[off[fi[q]] + fl[q]], q), "a kept entry is not at offsets[idx] + loc"
    assert int((slot[:rb] >= 0).sum()) == q.size, "a row names an entry that was not kept (or one entry twice)"


def run_layout_fuzz(n_cases, seed, verbose=False):
    """ops.packed_layout on real routings (ops.compute_location on random / skewed / all-on-k expert ids, a share masked) against
    F.ref_layout.  -> list of failure descriptions"""
    from tutel_amd import ops
    bad, seen, t0 = [], set(), time.time()
    for d in F.gen_layout_cases(n_cases, seed):
        tag = F.layout_tag(d)
        try:
            T, E, k = d["T"], d["E"], d["k"]
            idx = F.make_routing(d)
            idx_d = torch.from_numpy(idx).cuda()
            loc_d, cnt_d, _, _, _ = ops.compute_location(idx_d, E)
            loc, cnt = loc_d.cpu().numpy(), cnt_d.cpu().numpy()
            loc_r, cnt_r = F.ref_locations(idx, E)
            assert np.array_equal(cnt, cnt_r) and np.array_equal(loc, loc_r), "compute_location differs from the stable rank"
            plan = _plan(T, E, k, d["limit"], d["align"])
            ref = F.ref_layout(cnt, idx, loc, E, d["limit"], d["align"], plan["rows_bound"])
            seen |= F.layout_classes(d, ref, plan["rows_bound"], idx)
            lay = _sentinel_layout(E, plan)
            ops.packed_layout(cnt_d, idx_d, loc_d, d["limit"], d["align"], plan["rows_bound"], plan["tiles_bound"], plan["row_limit"], out=lay)
            _check_layout(lay, ref, plan, idx, loc, T)
        except Exception as ex:  # noqa: BLE001 -- the sweep reports every failing case
            _fail(bad, tag, ex, verbose)
        if verbose and (d["case"] + 1) % 100 == 0:
            print(f"{d['case'] + 1} layout cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    F.check_promised("layout", seen, F.LAYOUT_PROMISED, n_cases, DEFAULT_CASES)
    return bad


def _rows_layout(d):
    """the case's layout from the library, checked against the offsets its row counts imply"""
    lay, idx, loc = F.layout_from_rows(d["rows"], d["align"])
    off = lay.offsets.cpu()
    assert off.tolist() == F.offsets_from_rows(d["rows"], d["align"]), "offsets of the synthesised layout"
    ref = F.ref_layout(d["rows"], idx.cpu().numpy(), loc.cpu().numpy(), d["E"], 0, d["align"], lay.rows_bound)
    assert np.array_equal(lay.slot_map.cpu().numpy()[:lay.rows_bound], ref["slot"]), "slot map of the synthesised layout"
    assert int(lay.capacity) == ref["capacity"] and int(lay.ntiles) == ref["ntiles"], "capacity / tile count of the synthesised layout"
    return lay, off


def _moat_slot_map(lay, used, T):
    """rebind the layout's slot map to a copy inside a guard band (F.moated) whose entries name a token row of a T-row array that no live
    row reads -- the caller fills that row with NaN -- or token 0 where every row is read: an index a kernel may follow -> that row | None"""
    free = F.free_token(lay.slot_map.cpu().numpy()[:used], T) if T > 0 else None
    lay.slot_map = F.moated(lay.slot_map, fill=free if free is not None else 0)
    return free


def _moats_intact(*named):
    for what, t in named:
        if t is not None:
            F.moat_intact(t, what)


def _gemm_tol(dtype):
    # the bar of run_gemm_fuzz / test_ops_gpu._gemm_tol for inputs scaled by 1 / sqrt(K)
    return (2 ** -7, 2e-3) if dtype == torch.bfloat16 else (2 ** -10, 3e-4)


def run_gemm_fuzz(n_cases, seed, verbose=False):
    """ops.expert_gemm_packed against fp64 over layouts synthesised from per-expert row counts.  Rows of `a` at or past offsets[E] are
    NaN and `out` is pre-filled: every row below offsets[E] (pad rows included) within the GEMM bar, every row at or past it untouched,
    a second call the same bits, a zero in `mul` an exact zero.  -> list of failure descriptions"""
    from tutel_amd import ops
    bad, seen, t0 = [], set(), time.time()
    for d in F.gen_gemm_cases(n_cases, seed):
        tag = F.gemm_tag(d)
        seen |= F.gemm_classes(d)
        try:
            dtype = F.DTYPES[d["dtype"]]
            E, N, K, kmajor = d["E"], d["N"], d["K"], d["kmajor"]
            g = torch.Generator().manual_seed(d["seed"])
            lay, off = _rows_layout(d)
            used, rb = int(off[-1]), lay.rows_bound
            w = ((torch.rand([E, N, K] if kmajor else [E, K, N], generator=g) * 2 - 1) / math.sqrt(K)).to(dtype)
            bias = torch.randn([E, N], generator=g).to(dtype) if d["bias"] else None
            mul = None
            if d["mul"]:
                mul = torch.randn([rb, N], generator=g)
                mul[torch.rand([rb, N], generator=g) < 0.25] = 0
                mul = mul.to(dtype)
            if d["gather"]:
                x = torch.randn([d["T"], K], generator=g).to(dtype)
                free = _moat_slot_map(lay, used, d["T"])
                if free is not None:
                    x[free] = float("nan")      # the token row the slot map's band names: nothing may read it
                a_rows = F.gathered(x, lay.slot_map.cpu()[:max(used, 1)])
                assert not bool(torch.isnan(a_rows).any())
                a_dev, zero = F.moated(x, device="cuda"), F.moated(torch.zeros([max(K, 8)], dtype=dtype), device="cuda")
            else:
                a_rows = torch.randn([rb, K], generator=g).to(dtype)
                a_rows[used:] = float("nan")
                a_dev, zero = F.moated(a_rows, device="cuda"), None
                _moat_slot_map(lay, used, 0)
            wd, bd, md = (F.moated(t, device="cuda") if t is not None else None for t in (w, bias, mul))

            def run():
                o = F.moated(torch.full([rb, N], 3.0, dtype=dtype, device="cuda"), fill=F.OUT_FILL)
                ops.expert_gemm_packed(a_dev, wd, bd, kmajor, lay, act=d["act"], gather=d["gather"] or None, zero_row=zero, mul=md, out=o)
                F.moat_intact(o, "out")
                return o.cpu()
            got = run()
            _moats_intact(("a", a_dev), ("w", wd), ("bias", bd), ("mul", md), ("zero_row", zero), ("slot_map", lay.slot_map))
            assert bool((got[used:] == 3.0).all()), "a row at or past offsets[E] was written"
            ref = F.ref_gemm(a_rows, w, bias, kmajor, d["act"], mul, off, dtype)
            rtol, atol = _gemm_tol(dtype)
            err = (got[:used].double() - ref).abs()
            viol = err - (atol + rtol * ref.abs())
            if used and not bool((viol <= 0).all()):   # (NaN-safe: a NaN fails the comparison)
                i = int(torch.nan_to_num(viol, nan=float("inf")).argmax())
                r, c = i // N, i % N
                raise AssertionError(f"row {r} column {c}: {float(got[r, c])} vs {float(ref[r, c])} ({int((~(viol <= 0)).sum())} elements beyond the bar)")
            if mul is not None and used:
                assert bool((got[:used][mul[:used] == 0] == 0).all()), "a zero in mul did not give an exact zero"
            assert torch.equal(got.view(torch.int16), run().view(torch.int16)), "a second call gave other bits"
        except Exception as ex:  # noqa: BLE001
            _fail(bad, tag, ex, verbose)
        if verbose and (d["case"] + 1) % 100 == 0:
            print(f"{d['case'] + 1} packed gemm cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    F.check_promised("gemm", seen, F.GEMM_PROMISED, n_cases, DEFAULT_CASES)
    return bad


def _first_violation(viol, shape):
    i = int(torch.nan_to_num(viol, nan=float("inf")).argmax())
    return [int(v) for v in np.unravel_index(i, shape)]


def run_grad_fuzz(n_cases, seed, verbose=False):
    """ops.expert_wgrad_packed and ops.expert_bgrad_packed against fp64: the weight gradient within 2^-8 |ref| + 2^-12 (|A|^T |B|) (+ 2^-24
    for fp16), the bias gradient within u |ref| + n_e 2^-24 sum |B| (F.bgrad_bound); exact zeros for an expert without rows; the same bits
    on a second call; NaN in the rows at or past offsets[E].  -> list of failure descriptions"""
    from tutel_amd import ops
    bad, seen, t0 = [], set(), time.time()
    for d in F.gen_grad_cases(n_cases, seed):
        tag = F.grad_tag(d)
        seen |= F.grad_classes(d)
        try:
            dtype = F.DTYPES[d["dtype"]]
            E, Na, Nb = d["E"], d["Na"], d["Nb"]
            g = torch.Generator().manual_seed(d["seed"])
            lay, off = _rows_layout(d)
            used, rb = int(off[-1]), lay.rows_bound
            slot = lay.slot_map.cpu()[:max(used, 1)]
            free = _moat_slot_map(lay, used, d["T"])

            def operand(N, is_gathered):
                if is_gathered:
                    x = torch.randn([d["T"], N], generator=g).to(dtype)
                    if free is not None:
                        x[free] = float("nan")      # the token row the slot map's band names: nothing may read it
                    rows = F.gathered(x, slot)
                    assert not bool(torch.isnan(rows).any())
                    return F.moated(x, device="cuda"), rows
                t = torch.randn([rb, N], generator=g).to(dtype)
                t[used:] = float("nan")
                return F.moated(t, device="cuda"), t
            a_dev, a_rows = operand(Na, d["gather"] == "a")
            b_dev, b_rows = operand(Nb, d["gather"] == "b")
            gather = None if d["gather"] == "none" else d["gather"]
            zero = F.moated(torch.zeros([max(Na, Nb, 8)], dtype=dtype), device="cuda") if gather else None
            got_d = ops.expert_wgrad_packed(a_dev, b_dev, lay, gather=gather, zero_row=zero)
            got = got_d.cpu()
            ref, bnd = F.ref_wgrad(a_rows, b_rows, off)
            viol = (got.double() - ref).abs() - F.wgrad_bound(ref, bnd, dtype)
            if not bool((viol <= 0).all()):
                e, i, j = _first_violation(viol, viol.shape)
                raise AssertionError(f"dW[{e}][{i}][{j}] = {float(got[e, i, j])} vs {float(ref[e, i, j])} (bound operand {float(bnd[e, i, j]):.3e})")
            empty = torch.tensor([off[e + 1] == off[e] for e in range(E)])
            assert bool((got[empty] == 0).all()), "dW of an expert without rows is not exactly zero"
            assert torch.equal(got_d, ops.expert_wgrad_packed(a_dev, b_dev, lay, gather=gather, zero_row=zero)), "dW: a second call gave other bits"
            if d["gather"] != "b":   # the bias gradient sums packed rows (it has no gathered form)
                db = ops.expert_bgrad_packed(b_dev, lay).cpu()
                dref, mag, n = F.ref_bgrad(b_rows, off)
                viol = (db.double() - dref).abs() - F.bgrad_bound(dref, mag, n, dtype)
                if not bool((viol <= 0).all()):
                    e, j = _first_violation(viol, viol.shape)
                    raise AssertionError(f"db[{e}][{j}] = {float(db[e, j])} vs {float(dref[e, j])} over {int(n[e])} rows (sum |B| {float(mag[e, j]):.3e})")
                assert bool((db[empty] == 0).all()), "db of an expert without rows is not exactly zero"
            # the outputs the caller allocates: the accumulating forms, D + G bit for bit with every band intact
            G = ops.expert_wgrad_packed(a_dev, b_dev, lay, gather=gather, zero_row=zero, out_dtype=torch.float32)
            D = F.moated(torch.full([E, Na, Nb], 0.5, device="cuda"), fill=F.OUT_FILL)
            ops.expert_wgrad_packed(a_dev, b_dev, lay, gather=gather, zero_row=zero, accumulate_into=D)
            F.moat_intact(D, "dW accumulate_into")
            assert torch.equal(D, 0.5 + G), "dW: accumulate_into is not D + G bit for bit"
            if d["gather"] != "b":
                g32 = ops.expert_bgrad_packed(b_dev, lay, out_dtype=torch.float32)
                db_acc = F.moated(torch.full([E, Nb], 0.5, device="cuda"), fill=F.OUT_FILL)
                ops.expert_bgrad_packed(b_dev, lay, accumulate_into=db_acc)
                F.moat_intact(db_acc, "db accumulate_into")
                assert torch.equal(db_acc, 0.5 + g32), "db: accumulate_into is not D + G bit for bit"
            _moats_intact(("a", a_dev), ("b", b_dev), ("zero_row", zero), ("slot_map", lay.slot_map))
        except Exception as ex:  # noqa: BLE001
            _fail(bad, tag, ex, verbose)
        if verbose and (d["case"] + 1) % 100 == 0:
            print(f"{d['case'] + 1} packed grad cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    F.check_promised("grad", seen, F.GRAD_PROMISED, n_cases, DEFAULT_CASES)
    return bad


def run_decode_fuzz(oracle, n_cases, seed, verbose=False):
    """ops.fast_decode_packed against the CPU oracle's fast_decode over the same rows laid out padded on the host, bit for bit;
    ops.gate_grad_packed against oracle.gate_grad (the tolerance of test_ops_gpu.py::test_gate_grad; the rows are scaled by
    sqrt(256 / M) above M = 256 so that the sums keep that test's magnitude), exactly 0 for entries the row limit dropped or the routing
    masked; the decode's backward, fast_encode through the packed slot map, bit for bit.  Rows of `buf` at or past offsets[E] are NaN.
    -> list of failure descriptions"""
    from tutel_amd import ops
    bad, seen, t0 = [], set(), time.time()
    for d in F.gen_decode_cases(n_cases, seed):
        tag = F.decode_tag(d)
        try:
            dtype = F.DTYPES[d["dtype"]]
            T, E, k = d["T"], d["E"], d["k"]
            idx = F.make_routing(d)
            idx_d = torch.from_numpy(idx).cuda()
            loc_d, cnt_d, _, _, _ = ops.compute_location(idx_d, E)
            loc, cnt = loc_d.cpu().numpy(), cnt_d.cpu().numpy()
            plan = _plan(T, E, k, d["limit"], d["align"])
            rb = plan["rows_bound"]
            ref = F.ref_layout(cnt, idx, loc, E, d["limit"], d["align"], rb)
            lay = _sentinel_layout(E, plan)
            ops.packed_layout(cnt_d, idx_d, loc_d, d["limit"], d["align"], rb, plan["tiles_bound"], plan["row_limit"], out=lay)
            _check_layout(lay, ref, plan, idx, loc, T)
            off, used = ref["offsets"], int(ref["offsets"][-1])
            C = max(1, int(ref["kept"].max()))       # the host's padded capacity: an entry is kept iff loc < min(count_e, L) <=> loc < C
            M = F.decode_M(d, E, C)
            tag = tag.replace(f"M={d['M']}", f"M={M}")
            seen |= F.decode_classes(d, ref, rb, M, idx)
            g = torch.Generator().manual_seed(d["seed"])
            buf = (torch.randn([max(rb, 1), M], generator=g) * min(1.0, math.sqrt(256 / M))).to(dtype)
            buf[used:] = float("nan")
            x = torch.randn([T, M], generator=g).to(dtype)
            gates = {"f32": torch.float32, "row": dtype, "none": None}[d["gates"]]
            if gates is not None:
                gates = torch.rand([k, T], generator=g).to(gates)
            pad = F.padded_rows(buf, off, ref["kept"], C)
            idx_t, loc_t = torch.from_numpy(idx), torch.from_numpy(loc)
            # an entry past the row limit has loc >= L >= C: the oracle drops it as the padded path does
            crit = (E, [idx_t[j] for j in range(k)], [loc_t[j] for j in range(k)],
                    [gates[j].float() if gates is not None else torch.ones([T]) for j in range(k)], C, None)
            want = oracle.fast_decode(pad, crit, is_postscore=True)
            buf_d, gates_d = buf.cuda(), gates.cuda() if gates is not None else None
            got = ops.fast_decode_packed(buf_d, idx_d, loc_d, gates_d, lay).cpu()
            if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
                ne = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
                t, c = int(ne[0][0]), int(ne[0][1])
                raise AssertionError(f"decode differs in {ne.shape[0]} elements, first token {t} column {c}: {float(got[t, c])} vs {float(want[t, c])}")
            gg = ops.gate_grad_packed(x.cuda(), buf_d, idx_d, loc_d, lay).cpu()
            keep = torch.from_numpy(ref["keep"])
            for j in range(k):
                torch.testing.assert_close(gg[j], oracle.gate_grad(x, pad, idx_t[j], loc_t[j], C), rtol=1e-5, atol=1e-4, msg=lambda m: f"gate_grad choice {j}: {m}")
            assert bool((gg[~keep] == 0).all()), "the gate gradient of a dropped / masked entry is not exactly zero"
            enc = ops.fast_encode(x.cuda(), lay.slot_map, gates_d, max(rb, 1)).cpu()
            want_enc = F.ref_encode(x, ref["slot"] if rb > 0 else np.array([-1]), gates)
            assert torch.equal(enc.view(torch.int16), want_enc.view(torch.int16)), "encode through the packed slot map (the decode's backward)"
        except Exception as ex:  # noqa: BLE001
            _fail(bad, tag, ex, verbose)
        if verbose and (d["case"] + 1) % 100 == 0:
            print(f"{d['case'] + 1} packed decode cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    F.check_promised("decode", seen, F.DEC_PROMISED, n_cases, DEFAULT_CASES)
    return bad


def _make_fuzz_layer(d, oracle):
    """the case's layer (eval, on the GPU) and its CPU tensors: x, and what the oracle's expert function needs"""
    from tutel import moe
    Fn = torch.nn.functional
    acts = {"relu": Fn.relu, "gelu": Fn.gelu, "silu": Fn.silu}
    dtype = F.DTYPES[d["dtype"]]
    T, M, H, E, k = d["T"], d["M"], d["H"], d["E"], d["k"]
    x, wg, w1, b1, w2, b2 = oracle.make_problem(T, M, H, E, dtype=dtype, seed=d["seed"])
    swiglu = d["experts"] == "swiglu"
    experts = {"type": "llama_ffn" if swiglu else "ffn", "num_experts_per_device": E, "hidden_size_per_expert": H, "activation_fn": acts[d["act"]]}
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        layer = moe.moe_layer(gate_type={"type": "top", "k": k, "capacity_factor": d["cf"], "fp32_gate": d["fp32_gate"]}, experts=experts,
                              model_dim=M, normalize_gate=d["norm"], is_postscore=True)
    finally:
        torch.set_default_dtype(old)
    ex = layer.experts
    with torch.no_grad():
        layer.gates[0].wg.weight.copy_(wg.to(layer.gates[0].wg.weight.dtype))
        if swiglu:
            # nn.Linear-style spread (as make_problem gives the ffn experts), so that the outputs stay below 1 and _close's bar applies
            g = torch.Generator().manual_seed(d["seed"] + 1)
            u1 = ((torch.rand([E, M, H], generator=g) * 2 - 1) / M ** 0.5).to(dtype)
            u2 = ((torch.rand([E, M, H], generator=g) * 2 - 1) / M ** 0.5).to(dtype)
            u3 = ((torch.rand([E, H, M], generator=g) * 2 - 1) / H ** 0.5).to(dtype)
            ex.W_fc1.copy_(u1.reshape(-1)); ex.W_fc2.copy_(u2.reshape(-1)); ex.W_fc3.copy_(u3.reshape(-1))
            ffn = lambda enc: oracle.expert_llama_ffn(enc, u1, u2, u3, act=acts[d["act"]], accum_fp32=True)
        else:
            ex.batched_fc1_w.copy_(w1); ex.batched_fc1_bias.copy_(b1); ex.batched_fc2_w.copy_(w2); ex.batched_fc2_bias.copy_(b2)
            ffn = lambda enc: oracle.expert_ffn(enc, w1, b1, w2, b2, act=acts[d["act"]], accum_fp32=True)
    return layer.cuda().eval(), x, ffn


def run_layer_fuzz(oracle, n_cases, seed, verbose=False):
    """random dropless layers (ffn experts with ReLU / GELU / SiLU, and SwiGLU experts; eval) with dropless_packed = True, the packed
    forward required to have run: the routing it used must be the oracle's on the kernels' own scores, the device capacity the oracle's,
    and y the oracle's encode -> fp32-accumulating experts -> decode on that routing within test_layer_gpu._close.  The padded forward is
    a second opinion only (equal bits); every fourth case is replayed from a GraphedForward captured on ANOTHER batch.  Only shapes the
    layer's own eligibility check covers are drawn (F.gen_layer_cases).  -> list of failure descriptions"""
    from test_layer_gpu import _close
    from tutel_amd import ops
    from tutel_amd.impls.graph import GraphedForward
    bad, seen, t0 = [], set(), time.time()
    for d in F.gen_layer_cases(n_cases, seed):
        tag = F.layer_tag(d)
        seen |= F.layer_classes(d)
        try:
            dtype = F.DTYPES[d["dtype"]]
            T, E, k, cf, mega = d["T"], d["E"], d["k"], d["cf"], d["mega"]
            layer, x, ffn = _make_fuzz_layer(d, oracle)
            layer._keep_routing, layer.last_logits = True, None
            xd = x.cuda()
            layer.dropless_packed = True
            with torch.no_grad():
                y = layer(xd, megablocks_size=mega).clone()
                ran = layer._dropless_packed_ran
                assert ran is True, f"the packed forward did not run: {ran}"
                idx, loc = layer.last_routing
                cnt, cap = layer.dispatch_count.clone(), int(layer.dropless_capacity)
                logits = layer.last_logits if layer.last_logits is not None else layer.gates[0](xd)
                scores = ops.gate_topk(logits.contiguous(), k, apply_softmax=True, want_scores=True)[3].cpu()
            crit, _ = oracle.extract_critical(scores, k, cf, normalize_gate=d["norm"], alignment=mega if (mega > 0 and E > 1) else 1)
            assert torch.equal(idx.cpu(), torch.stack([t.to(torch.int32) for t in crit[1]])), "idx"
            assert torch.equal(loc.cpu(), torch.stack([t.to(torch.int32) for t in crit[2]])), "loc"
            assert torch.equal(cnt.cpu(), crit[5]), "dispatch_count"
            assert cap == crit[4], f"device capacity {cap} vs {crit[4]}"
            enc = oracle.fast_encode(x.to(scores.dtype), crit, True).to(dtype)
            yo = oracle.fast_decode(ffn(enc).to(scores.dtype), crit, True).to(dtype)
            _close(y.view(T, -1), yo, dtype)
            layer.dropless_packed = False
            with torch.no_grad():
                assert torch.equal(layer(xd, megablocks_size=mega), y), "the padded forward gives other bits (second opinion)"
            if d["graph"]:
                with torch.no_grad():
                    gf = GraphedForward(layer, torch.roll(xd, 1, 0) * 2, dropless_packed=True, megablocks_size=mega)   # captured on another batch
                    assert torch.equal(gf(xd), y) and torch.equal(gf(xd), y), "graph replay vs the eager packed forward (twice)"
        except Exception as ex_:  # noqa: BLE001
            _fail(bad, tag, ex_, verbose)
        if verbose and (d["case"] + 1) % 50 == 0:
            print(f"{d['case'] + 1} packed layer cases, {len(bad)} failed, {time.time() - t0:.0f} s", flush=True)
    F.check_promised("layer", seen, F.LAYER_PROMISED, n_cases, DEFAULT_CASES)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_packed_layout_fuzz_vs_integer_reference(n_cases):
    bad = run_layout_fuzz(n_cases, seed=SEEDS["layout"])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_packed_gemm_fuzz_vs_float64(n_cases):
    bad = run_gemm_fuzz(n_cases, seed=SEEDS["gemm"])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_packed_wgrad_bgrad_fuzz_vs_float64(n_cases):
    bad = run_grad_fuzz(n_cases, seed=SEEDS["grad"])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_packed_decode_gate_grad_fuzz_vs_oracle(oracle, n_cases):
    bad = run_decode_fuzz(oracle, n_cases, seed=SEEDS["decode"])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n_cases", [DEFAULT_CASES, pytest.param(10 * DEFAULT_CASES, marks=pytest.mark.slow)])
def test_packed_layer_forward_fuzz_vs_oracle(oracle, n_cases):
    bad = run_layer_fuzz(oracle, n_cases, seed=SEEDS["layer"])
    assert not bad, "\n".join(bad[:20])


if __name__ == "__main__":
    from oracle import moe_oracle
    moe_oracle._lib()
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10 * DEFAULT_CASES
    what = sys.argv[3] if len(sys.argv) > 3 else "layout"
    runners = {"layout": lambda s: run_layout_fuzz(n, s, verbose=True), "gemm": lambda s: run_gemm_fuzz(n, s, verbose=True),
               "grad": lambda s: run_grad_fuzz(n, s, verbose=True), "decode": lambda s: run_decode_fuzz(moe_oracle, n, s, verbose=True),
               "layer": lambda s: run_layer_fuzz(moe_oracle, n, s, verbose=True)}
    assert what in runners, f"what: one of {sorted(runners)}"
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else SEEDS[what]
    failed = runners[what](sd)
    # the run-record directory of tests/test_fuzz_gpu.py's driver: the `*_out/` entry of .gitignore
    out_dir = os.path.join(ROOT, next(ln.strip().rstrip("/") for ln in open(os.path.join(ROOT, ".gitignore")) if ln.strip().endswith("_out/")))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"packed_{what}_fuzz_{sd}.json"), "w") as f:
        json.dump(dict(source="tests/test_packed_fuzz_gpu.py", cases=n, seed=sd, failed=failed), f, indent=1)
    print("cases", n, "failed", len(failed))
    sys.exit(1 if failed else 0)
