"""tests/golden/assign_parent_bits.npz is consistent in itself (no GPU): the recorded matching is a minimum-cost assignment of the
recorded cost matrix, rows_sorted is the matching sorted, and the recorded tokens are the feature rows it names."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens_assign_bits", os.path.join(HERE, "golden", "make_goldens_assign_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
FIXTURE = G.load()
WIDE = 8            # cheapest rows per column that the search below looks at


def _f32(bits):
    return np.ascontiguousarray(bits).view(np.float32)


def test_fixture_covers_the_shapes_it_is_meant_to():
    cs = [c for c, _ in FIXTURE]
    assert {c["N"] for c in cs} >= {1, 3, 63, 64, 65, 240, 256}
    assert {c["L"] for c in cs} >= {1, 2, 3, 4}
    assert {c["S"] for c in cs} >= {1, 2, 3, 16, 18, 36, 72, 250}
    assert {c["E"] for c in cs} >= {16, 32, 128, 256}
    work = {sum(c["valid"]) for c in cs if (c["N"], c["L"], c["S"], c["E"]) == (240, 4, 36, 128) and not c["off"] and not c["dup"]}
    assert work >= {0, 1, 3, 4}
    assert any(c["valid"] == [1, 0, 1, 0] for c in cs) and {c["off"] for c in cs} >= {"part", "whole"} and {c["dup"] for c in cs} >= {"pair", "all"}
    assert os.path.getsize(G.FIXTURE) < 100 * 1024


@pytest.mark.parametrize("i", range(len(FIXTURE)))
def test_recorded_matching_is_a_minimum_of_the_recorded_cost(i):
    """Search over the assignments of the valid columns to distinct rows, totals summed in f32 over ascending label index as the
    kernel sums them.  All rows take part where N <= 4 * WIDE; above that the rows are the union of the WIDE cheapest of every valid
    column (an optimal assignment of m <= 4 columns exists inside the m cheapest rows of each; twice as many are searched)."""
    c, rec = FIXTURE[i]
    N, L = c["N"], c["L"]
    cost = _f32(rec["cost"]).reshape(N, L)
    rows = rec["rows_by_col"].astype(np.int64)
    cols = [j for j in range(L) if c["valid"][j]]
    for j in range(L):
        if j in cols:
            assert np.isfinite(cost[:, j]).all() and 0 <= rows[j] < N
        else:
            assert np.isposinf(cost[:, j]).all() and rows[j] == -1
    assert len(set(rows[cols].tolist())) == len(cols)
    assert int(rec["n_valid"][0]) == len(cols)
    if not cols:
        return
    if N <= 4 * WIDE:
        cand = np.arange(N)
    else:
        cand = np.unique(np.concatenate([np.argsort(cost[:, j], kind="stable")[:WIDE] for j in cols]))
    assert set(rows[cols].tolist()) <= set(cand.tolist())
    total = np.zeros((), np.float32)
    idx = []
    for n_, j in enumerate(cols):
        shape = [1] * len(cols)
        shape[n_] = len(cand)
        total = (total + cost[cand, j].reshape(shape)).astype(np.float32)          # f32 + f32, ascending j
        idx.append(np.arange(len(cand)).reshape(shape))
    clash = np.zeros(total.shape, bool)
    for a in range(len(cols)):
        for b in range(a + 1, len(cols)):
            clash |= idx[a] == idx[b]
    best = np.where(clash, np.float32(np.inf), total).min()
    got = np.float32(0)
    for j in cols:
        got = np.float32(got + cost[rows[j], j])
    assert got.view(np.uint32) == np.float32(best).view(np.uint32), (float(got), float(best))


@pytest.mark.parametrize("i", range(len(FIXTURE)))
def test_recorded_rows_sorted_and_tokens_follow_from_the_matching(i):
    c, rec = FIXTURE[i]
    N, L, E = c["N"], c["L"], c["E"]
    _, _, feat = G.case_inputs(c)
    rows = rec["rows_by_col"].astype(np.int64)
    want = sorted(int(r) for r in rows if r >= 0)
    want = np.asarray(want + [-1] * (L - len(want)), np.int64)
    assert np.array_equal(rec["rows_sorted"], want) and np.array_equal(rec["tok_rows_sorted"], want)
    tokens = rec["tokens"].reshape(L + 1, E)
    for l in range(L):
        if want[l] >= 0:
            assert np.array_equal(tokens[l], feat[want[l]].view(np.uint32))
        else:
            assert not tokens[l].any()                                                  # +0.0 in every unused slot
    assert rec["valid"].tolist() == [int(r >= 0) for r in want] + [1]
    rest = N - int((want >= 0).sum())
    if rest:
        # the last token is (sum of all rows - sum of the matched rows) / rest in f32: fewer than N + 8 roundings (N adds, L <= 4 more,
        # one subtraction, one division), each of relative size 2^-24 on a value bounded by sum |feat|
        keep = np.ones(N, bool)
        keep[want[want >= 0]] = False
        ref = feat[keep].astype(np.float64).sum(0) / rest
        bound = (N + 8) * 2.0 ** -24 * np.abs(feat).astype(np.float64).sum(0) / rest
        assert (np.abs(_f32(tokens[L]).astype(np.float64) - ref) <= bound).all()
    # one-to-many: n pairs of (anchor, valid label row), -1 behind them
    n = int(rec["many_n"][0])
    mr, mc = rec["many_rows"], rec["many_cols"]
    assert (mr[n:] == -1).all() and (mc[n:] == -1).all() and ((mr[:n] >= 0) & (mr[:n] < N)).all()
    assert all(c["valid"][int(j)] for j in mc[:n]) and len(set(mr[:n].tolist())) == n
    assert (n == 0) == (sum(c["valid"]) == 0)
