"""The kernels of ops/csrc/score.hip and ops/csrc/rank.hip against plain
oracles, all bit-exact: ``native.risk_score`` and ``native.score_gather``
against ``cpu_ref.risk_score`` under the default and under 22 distinct
dyadic weights, ``native.rank_bucket_order`` against the torch key sort it
replaces, ``native.severity_histogram`` against ``cpu_ref``.
test_score_tail_cpu.py pins those oracles against models/blast.py.

Sizes: 600 001 elements is more than the 2048 x 256 threads of the largest
grid, so the grid-stride loops take a second pass, and no multiple of 256."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import score_tail_cases as st
from score_tail_cases import DYADIC

from agentbom_amd.ops import cpu_ref, native

pytestmark = pytest.mark.gpu

BIG = 600_001


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


@pytest.fixture(params=[False, True], ids=["default", "dyadic"])
def weights(request, monkeypatch):
    w = DYADIC if request.param else st.default_weights()
    st.set_weights(monkeypatch, w)
    return w


def _dev(a: np.ndarray, dev):
    """uint32 travels as its int32 bit pattern; torch has no uint32 kernels."""
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ── risk_score ──────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", [1, 255, BIG])
def test_risk_score_bit_exact(weights, n, dev):
    """Kernel and oracle do the same f32 operations in the same order, and
    every multiply feeds fminf, so nothing can contract into an FMA."""
    cols = st.tile(st.risk_grid(weights), n)
    got = native.risk_score(*(_dev(cols[k], dev) for k in st.KERNEL_COLUMNS)).cpu().numpy()
    want = st.reference_scores(cols)
    assert got.shape == want.shape == (n,)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (
        f"{diff.size} scores differ, first at {diff[0]}: {got[diff[0]]!r} != {want[diff[0]]!r}")
    assert np.array_equal(got, want)


# ── score_gather ────────────────────────────────────────────────────────────

@pytest.mark.parametrize("n", [0, 1, BIG])
def test_score_gather_bit_exact(weights, n, dev):
    """Scores bit-exact, counts exact; scorecard is -1, suppressed never set
    and kev any nonzero byte on this route."""
    c = st.gather_case(weights, n=n)
    got = native.score_gather(*(_dev(c[k], dev) for k in st.GATHER_ARGS))
    want = st.gather_oracle(c)
    for name, g, w in zip(("scores", "n_agents", "n_creds", "n_tools"), got, want):
        g = g.cpu().numpy()
        assert g.shape == (n,) and g.dtype == w.dtype, name
        assert np.array_equal(g, w), f"{name}: {int(np.sum(g != w))} of {n} differ"


# ── rank ────────────────────────────────────────────────────────────────────

def _rank_matches(scores: np.ndarray, dev, workspace=None):
    t = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32))
    got = native.rank_bucket_order(t.to(dev), workspace).cpu()
    assert torch.equal(got, st.rank_oracle(t)), f"n={len(scores)}"
    return got


def test_rank_rounds_half_to_even(dev):
    """k / 100 for every k, every f32 whose product with 100 is exactly
    k + 0.5, -0.0, +-inf, 10.0 and the f32 above it.  NaN is left out: the
    oracle's NaN -> int64 conversion is undefined."""
    scores = st.rounding_scores()
    _rank_matches(scores, dev)
    _rank_matches(st.half_scores(), dev)
    _rank_matches(np.tile(scores, 17)[:16_385], dev)


def test_rank_ballot_groups(dev):
    """64 distinct bins in one wave; two bins that differ only in bit 9 of
    the ten ballots (0 and 512; 488 and 1000), alternating."""
    distinct = (np.arange(64) * 15 + 3) % 1001
    assert len(set(distinct.tolist())) == 64
    _rank_matches(st.bins_to_scores(distinct), dev)
    _rank_matches(st.bins_to_scores(distinct[::-1]), dev)
    lane = np.arange(64 * 5 + 9)
    for lo, hi in ((0, 512), (488, 1000)):
        got = _rank_matches(st.bins_to_scores(np.where(lane % 2 == 0, lo, hi)), dev)
        # the low bin first, each in index order
        assert got.tolist() == lane[::2].tolist() + lane[1::2].tolist()
        _rank_matches(st.bins_to_scores(np.where(lane % 3 == 0, hi, lo)), dev)


@pytest.mark.parametrize("n", [255, 256, 257, 16_383, 16_384, 16_385, 16_640])
def test_rank_block_counts(n, dev):
    """Chunk edges, and 64, 65 and 66 blocks, where the block scan starts to
    carry from one 64-block tile into the next."""
    rng = np.random.default_rng(n)
    bins = rng.integers(0, 1001, n)
    bins[::5] = 13            # a heavy bin in every block
    bins[-1] = 13
    _rank_matches(st.bins_to_scores(bins), dev)


def test_rank_workspace_reuse(dev):
    """One workspace for n = 100 001, then 63, then 100 001 again: what the
    larger run left in it must not reach the smaller one, nor the reverse."""
    rng = np.random.default_rng(11)
    big = (rng.random(100_001) * 12.0 - 1.0).astype(np.float32)
    small = (rng.random(63) * 10.0).astype(np.float32)
    ws: dict = {}
    first = _rank_matches(big, dev, ws)
    _rank_matches(small, dev, ws)
    third = _rank_matches(big, dev, ws)
    assert torch.equal(first, third)
    assert set(ws) == {"rank_hist", "rank_scratch"}


# ── severity histogram ──────────────────────────────────────────────────────

def _hist_matches(owner, sev, c, dev):
    owner = np.asarray(owner, dtype=np.uint32)
    sev = np.asarray(sev, dtype=np.uint8)
    got = native.severity_histogram(_dev(owner, dev), _dev(sev, dev), c).cpu().numpy()
    want = cpu_ref.severity_histogram(owner, sev, c)
    assert got.shape == want.shape == (c, 6)
    assert np.array_equal(got.view(np.uint32), want)
    return want


def test_histogram_one_hot_cell(dev):
    """Every finding on one (owner, severity) cell: all atomics on one word."""
    want = _hist_matches(np.full(BIG, 3), np.full(BIG, 4), 5, dev)
    assert want[3, 4] == BIG and want.sum() == BIG


def test_histogram_edges(dev):
    i = np.arange(BIG)
    _hist_matches(np.zeros(BIG), i % 6, 1, dev)                       # C = 1
    assert _hist_matches([], [], 7, dev).sum() == 0                   # n = 0
    c = 1000
    want = _hist_matches(np.where(i % 2 == 0, 0, c - 1), (i // 2) % 6, c, dev)
    assert want[1:c - 1].sum() == 0 and want[0].sum() + want[c - 1].sum() == BIG
