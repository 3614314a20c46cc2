"""The function-level and drop-in-surface checks of tests/golden/make_golden.py --check, replayed on any box: the reference's
observations are stored in tests/golden/reference_checks.npz (tests/golden/make_golden_checks.py), this repository's are made here
by the same code (tests/_reference_checks.py) -- routing (top-k with exact 16-bit ties, locations, gates, capacity, dispatch
counts, l_aux) and encode / decode over 4 dtypes x 8 shapes x normalize, cumsum, gate_grad, the dispatcher with masked tokens, the
loss functions, and tutel_amd's MOELayer against the reference's layer (seeded parameters, gates + gate_index, forward-time
overrides, training gradients, reserve_dims + custom expert + result_func, scan_expert_func, deprecated spellings, errors)."""
import os

import numpy as np
import pytest
import torch

import _reference_checks as C

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_checks.npz")


@pytest.fixture(scope="module")
def stored():
    z = np.load(FIXTURE)
    digests = {f[len("scores|"):]: bytes(z[f][0]) for f in z.files if f.startswith("scores|")}
    return C.from_record(z), C.score_inputs(), digests


def _check(obs, ref, names):
    assert set(obs) == names, sorted(set(obs) ^ names)[:5]
    bad = [(n, C.compare(n, v, m, ref[n])) for n, (v, m) in obs.items()]
    bad = [f"{n}: {why}" for n, why in bad if why]
    assert not bad, f"{len(bad)} of {len(obs)} differ from the reference: " + "; ".join(bad[:8])


def test_scores_are_the_generators(stored):
    """the scores made here are the bits the reference routed on (softmax_rows is host-independent), and the 16-bit sweep holds exact
    ties at the k / k+1 boundary -- the case the tie rule exists for"""
    _, scores, digests = stored
    assert set(scores) == set(digests)
    for n in scores:
        assert C.digest(scores[n]).encode() == digests[n], f"{n}: the seeded scores did not regenerate bit-identically"
    for (T, E, k, _) in C.SWEEP_SHAPES:
        if T >= 512:
            for dtype in (torch.bfloat16, torch.float16):
                top = torch.topk(scores[f"sweep_{T}_{E}_{k}"].to(dtype).float(), min(k + 1, E), dim=1).values
                assert bool((top[:, 1:] == top[:, :-1]).any()), (T, E, k, dtype)


def test_oracle_functions_match_the_reference(stored, oracle):
    ref, scores, _ = stored
    obs = C.function_checks(C.OracleImpl(), scores)
    assert sum(1 for n in ref if n.startswith("topk indices ")) == 64
    _check(obs, ref, {n for n in ref if not n.startswith("layer: ")})
    # the "lowest index" tie rule differs from the reference's only on rows where the chosen scores are the same multiset
    for (T, E, k, cf) in C.SWEEP_SHAPES:
        if T < 512:
            continue
        for dtype in (torch.bfloat16, torch.float16):
            sc = scores[f"sweep_{T}_{E}_{k}"].to(dtype)
            li, ri = torch.stack(oracle.topk_indices(sc, k, tie_rule="lowest")), torch.stack(oracle.topk_indices(sc, k))
            rows = (li != ri).any(0)
            s_o, s_r = sc.gather(1, li.t().long())[rows], sc.gather(1, ri.t().long())[rows]
            assert torch.equal(s_o.sort(1)[0], s_r.sort(1)[0]), (T, E, k, dtype)


def test_product_layer_surface_matches_the_reference(stored, monkeypatch):
    ref, _, _ = stored
    obs = C.surface_checks(C.product_build(monkeypatch.setattr))
    _check(obs, ref, {n for n in ref if n.startswith("layer: ")})


def test_product_net_matches_the_reference_over_gloo():
    """tutel_amd.net on two gloo ranks against the reference's tutel.net observations per rank: collective outputs and gradients,
    TutelDistributedOptimizer after three steps, create_groups_from_world (calls the reference cannot run on gloo are not compared)"""
    res = C.run_net("product", FIXTURE)
    for rank, (bad, n) in sorted(res.items()):
        assert n > 50 and not bad, f"rank {rank}: {len(bad)} of {n} differ from the reference: " + "; ".join(bad[:8])
