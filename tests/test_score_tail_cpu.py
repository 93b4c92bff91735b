"""Pins the oracles of test_score_tail_gpu.py before the GPU runs:
``cpu_ref.risk_score`` against the specification (models/blast.py), under the
default weights and under 22 distinct dyadic ones, and the preconditions of
the score-gather, rank and histogram cases.  No GPU."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import score_tail_cases as st
from score_tail_cases import DYADIC, WEIGHT_NAMES

from agentbom_amd.ops import cpu_ref, native


def test_dyadic_weights_are_distinct_and_exact():
    values = list(DYADIC.values())
    assert len(values) == 22 and len(set(values)) == 22
    assert all(v > 0 and (v * 64).is_integer() for v in values)
    # thresholds exactly representable: the f64 and the f32 comparison agree
    assert all(np.float32(v) == v for v in values)
    d = DYADIC
    assert d["RISK_AGENT_CAP"] == 4 * d["RISK_AGENT_WEIGHT"]
    assert d["RISK_CRED_CAP"] == 5 * d["RISK_CRED_WEIGHT"]
    assert d["RISK_TOOL_CAP"] == 9 * d["RISK_TOOL_WEIGHT"]
    assert (d["RISK_SCORECARD_TIER1_THRESHOLD"] < d["RISK_SCORECARD_TIER2_THRESHOLD"]
            < d["RISK_SCORECARD_TIER3_THRESHOLD"])


def test_weight_vector_follows_the_config(monkeypatch):
    """risk_weights_array() reads the config live, in the order of the
    formula in models/blast.py."""
    defaults = st.default_weights()
    assert np.array_equal(native.risk_weights_array(),
                          np.array([defaults[k] for k in WEIGHT_NAMES], dtype=np.float32))
    # six fields share 0.5 by default: the reason for the dyadic set
    assert sum(1 for v in defaults.values() if v == 0.5) == 6
    st.set_weights(monkeypatch, DYADIC)
    assert np.array_equal(native.risk_weights_array(),
                          np.array(list(DYADIC.values()), dtype=np.float32))


def _grid_covers(grid, weights):
    assert set(grid["severity"].tolist()) == {5, 4, 3, 2, 0, 1, 6, 255}
    assert set(grid["flags"].tolist()) == set(range(8))
    assert set(grid["reach"].tolist()) == {-1, 0, 1}
    for col, w, cap in (("n_agents", "RISK_AGENT_WEIGHT", "RISK_AGENT_CAP"),
                        ("n_creds", "RISK_CRED_WEIGHT", "RISK_CRED_CAP"),
                        ("n_tools", "RISK_TOOL_WEIGHT", "RISK_TOOL_CAP")):
        at = round(weights[cap] / weights[w])
        assert set(grid[col].tolist()) == {0, 1, at, at + 1, 2**31 + 5}
        assert abs(at * weights[w] - weights[cap]) < 1e-12
    thr = np.float32(weights["EPSS_CRITICAL_THRESHOLD"])
    ep = grid["epss"]
    assert np.any(ep < 0) and np.any(ep == 0) and np.any(ep == thr)
    assert np.any((ep > 0) & (ep < thr)) and np.any(ep > thr)
    sc = grid["scorecard"]
    assert np.any(sc < 0) and np.any(sc == 0)
    for t in ("RISK_SCORECARD_TIER1_THRESHOLD", "RISK_SCORECARD_TIER2_THRESHOLD",
              "RISK_SCORECARD_TIER3_THRESHOLD"):
        edge = np.float32(weights[t])
        assert np.any(sc == edge)
        assert np.any((sc < edge) & (sc > edge - np.float32(0.01)))
        assert np.any((sc > edge) & (sc < edge + np.float32(0.01)))


def test_cpu_ref_equals_the_spec_under_dyadic_weights(monkeypatch):
    """Exact: every term is a multiple of 1/64 (or a cap), so f32 and f64
    agree to the bit.  Some totals fall below 0 and some above 10."""
    st.set_weights(monkeypatch, DYADIC)
    grid = st.risk_grid(DYADIC)
    _grid_covers(grid, DYADIC)
    ref = st.reference_scores(grid)
    spec = st.spec_scores(grid)
    assert ref.dtype == np.float32
    assert np.array_equal(ref.astype(np.float64), spec)
    live = (grid["flags"] & 4) == 0
    assert np.any((spec == 0.0) & live & (grid["reach"] == 0)), "no total below 0"
    assert np.any(spec == 10.0), "no total above 10"
    assert len(np.unique(spec)) > 500


def test_cpu_ref_equals_the_spec_under_default_weights():
    """1e-5, the figure of test_risk_score_matches_python_model: 0.3, 0.1 and
    0.7 are not dyadic, so f32 and f64 differ in the last bits.

    The arrays hold the f32 roundings of the decimal values the spec gets.  On
    the threshold both sides say yes: the spec compares 0.7 >= 0.7, the oracle
    and the kernel f32(0.7) >= f32(0.7)."""
    weights = st.default_weights()
    grid = st.risk_grid(weights)
    _grid_covers(grid, weights)
    ref = st.reference_scores(grid)
    spec = st.spec_scores(grid)
    assert float(np.max(np.abs(ref.astype(np.float64) - spec))) < 1e-5
    assert np.any(spec == 10.0)


def test_swapped_weights_change_the_dyadic_scores(monkeypatch):
    """Under the dyadic weights no two of the 22 fields can trade places
    unnoticed; under the defaults the six 0.5 fields can."""
    st.set_weights(monkeypatch, DYADIC)
    grid = st.risk_grid(DYADIC)
    w = native.risk_weights_array()
    base = cpu_ref.risk_score(*(grid[k] for k in st.KERNEL_COLUMNS), weights=w)
    for a in range(22):
        for b in range(a + 1, 22):
            sw = w.copy()
            sw[[a, b]] = sw[[b, a]]
            got = cpu_ref.risk_score(*(grid[k] for k in st.KERNEL_COLUMNS), weights=sw)
            assert not np.array_equal(got, base), (WEIGHT_NAMES[a], WEIGHT_NAMES[b])


# ── score_gather ────────────────────────────────────────────────────────────

@pytest.mark.parametrize("dyadic", [False, True], ids=["default", "dyadic"])
def test_gather_case_and_oracle(monkeypatch, dyadic):
    weights = DYADIC if dyadic else st.default_weights()
    st.set_weights(monkeypatch, weights)
    c = st.gather_case(weights, n=4620 * 2 + 1)
    assert set(c["a_sev"].tolist()) == set(st.SEVERITIES)
    assert set(c["a_kev"].tolist()) == {0, 1, 2, 255}
    assert set(c["a_impact"].tolist()) == set(range(9))
    thr = np.float32(weights["EPSS_CRITICAL_THRESHOLD"])
    assert thr in c["a_epss"] and np.nextafter(thr, np.float32(0)) in c["a_epss"]
    assert not np.array_equal(c["cred_lut"], c["tool_lut"])
    assert set(c["cred_lut"].tolist()) == set(c["tool_lut"].tolist()) == {0, 1, 2}
    # the class pairs (cred, tool) over the nine impacts cover all but none
    assert len(set(zip(c["cred_lut"].tolist(), c["tool_lut"].tolist()))) >= 6
    for r in (0, 1, 2, 4):
        row = c["counts2d"][r].tolist()
        assert len(set(row)) == 6 and all(v > 1 and all(v % p for p in range(2, v)) for v in row)
    assert np.any(np.diff(c["pos"]) < 0) and np.any(np.diff(c["win_idx"]) < 0)
    d = c["dist"]
    assert st.UNVISITED in d and 0 in d and d[d != st.UNVISITED].max() >= 0x7FFFFFFF
    # every (window, count row, node) combination occurs
    combo = (c["win_idx"] * 7 + c["pos"]) * 11 + c["pkg_nodes"]
    assert len(np.unique(combo)) == 60 * 7 * 11

    scores, n_agents, n_creds, n_tools = st.gather_oracle(c)
    # the oracle against a loop written out finding by finding
    for i in range(0, len(scores), 97):
        w, r, node = int(c["win_idx"][i]), int(c["pos"][i]), int(c["pkg_nodes"][i])
        imp = int(c["a_impact"][w])
        row = c["counts2d"][r]
        creds = {2: row[2], 1: row[3], 0: 0}[int(c["cred_lut"][imp])]
        tools = {2: row[4], 1: row[5], 0: 0}[int(c["tool_lut"][imp])]
        assert (n_agents[i], n_creds[i], n_tools[i]) == (row[1], creds, tools)
        one = cpu_ref.risk_score(
            c["a_sev"][w:w + 1], np.array([row[1]], dtype=np.uint32),
            np.array([creds], dtype=np.uint32), np.array([tools], dtype=np.uint32),
            np.array([2 if c["a_kev"][w] else 0], dtype=np.uint8), c["a_epss"][w:w + 1],
            np.array([-1.0], dtype=np.float32),
            np.array([0 if d[node] == st.UNVISITED else 1], dtype=np.int8))
        assert one[0] == scores[i]
    assert len(np.unique(scores)) > 50
    # a column or a LUT taken for another changes counts and scores
    for a, b in ((2, 3), (4, 5), (2, 4), (1, 2), (0, 1)):
        mixed = dict(c, counts2d=c["counts2d"].copy())
        mixed["counts2d"][:, [a, b]] = mixed["counts2d"][:, [b, a]]
        m_scores, *m_counts = st.gather_oracle(mixed)
        assert not np.array_equal(m_scores, scores), (a, b)
        assert any(not np.array_equal(x, y) for x, y in zip(m_counts, (n_agents, n_creds, n_tools)))
    swapped = st.gather_oracle(dict(c, cred_lut=c["tool_lut"], tool_lut=c["cred_lut"]))
    assert not np.array_equal(swapped[0], scores)
    empty = st.gather_oracle(st.gather_case(weights, n=0))
    assert all(len(a) == 0 for a in empty)


# ── rank ────────────────────────────────────────────────────────────────────

def test_rounding_scores_hit_exact_halves():
    """The rank inputs hold products that are exactly k + 0.5 in f32, for
    even and odd k, where round-half-even and round-half-up part ways."""
    s = st.half_scores()
    prod = s * np.float32(100.0)
    halves = prod[(prod - np.floor(prod)) == np.float32(0.5)]
    k = np.floor(halves).astype(np.int64)
    assert np.sum(k % 2 == 0) >= 10 and np.sum(k % 2 == 1) >= 10
    assert np.any(np.rint(halves) != np.floor(halves + np.float32(0.5)))
    scores = st.rounding_scores()
    assert not np.isnan(scores).any()
    assert np.isposinf(scores).any() and np.isneginf(scores).any()
    assert np.any((scores == 0) & np.signbit(scores)), "no -0.0"
    assert np.float32(10.0) in scores and np.nextafter(np.float32(10), np.float32(11)) in scores
    for k100 in (0, 1, 500, 999, 1000):
        assert np.float32(k100 / 100.0) in scores


def test_rank_oracle_orders_by_bucket_then_index():
    scores = torch.from_numpy(st.rounding_scores().copy())
    order = st.rank_oracle(scores).numpy()
    assert np.array_equal(np.sort(order), np.arange(len(order)))
    q = np.clip(np.rint(scores.numpy() * np.float32(100.0)), 0, 1000).astype(np.int64)
    assert np.array_equal(order, np.lexsort((np.arange(len(q)), 1000 - q)))
    # torch rounds half to even, as rintf does
    assert torch.tensor([0.5, 1.5, 2.5]).round().tolist() == [0.0, 2.0, 2.0]


def test_bins_to_scores_round_trip():
    bins = np.arange(1001)
    s = st.bins_to_scores(bins)
    assert np.array_equal(1000 - np.rint(s * np.float32(100.0)).astype(np.int64), bins)
    assert 488 ^ 1000 == 512


# ── histogram ───────────────────────────────────────────────────────────────

def test_histogram_oracle():
    hist = cpu_ref.severity_histogram(np.array([0, 2, 2], dtype=np.uint32),
                                      np.array([5, 0, 0], dtype=np.uint8), 3)
    assert hist.shape == (3, 6) and hist.dtype == np.uint32
    assert hist[0, 5] == 1 and hist[2, 0] == 2 and hist.sum() == 3
    assert cpu_ref.severity_histogram(np.zeros(0, np.uint32), np.zeros(0, np.uint8), 4).sum() == 0
