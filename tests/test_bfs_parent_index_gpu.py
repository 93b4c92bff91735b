"""The parent index of the reach BFS's bottom-up pass: the index against a
numpy oracle of its definition, one indexed pass against the row-walking
kernel and the definition of a pass, native.bfs with the index against
cpu_ref.bfs and against the path without it (AGENT_BOM_BFS_PARENT_INDEX=0),
and the engine step.  Every comparison is exact equality.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from bfs_graphs import (
    AGENTS,
    ESTATE_N,
    PARENT_MORE,
    PARENT_NONE,
    SOURCES,
    UNVISITED,
    both_csr,
    bottom_up_oracle,
    estate_edges,
    mixed_dist,
    mixed_graph,
    parent_index_oracle,
)

pytestmark = pytest.mark.gpu

MASK = 0b11          # types 0 and 1 allowed, type 5 masked
KNOB = "AGENT_BOM_BFS_PARENT_INDEX"
# vertices of one pass of bfs_bottom_up_indexed_kernel's largest grid
# (2048 blocks x 256 threads x 4 vertices)
ONE_PASS = 2048 * 256 * 4
SIZES = [1, 3, 4, 5, 255, 256, 257, ONE_PASS + 5]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _to_dev(c, dev):
    return {k: (torch.from_numpy(v).to(dev) if v is not None else None) for k, v in c.items()}


def _index(rev_d, mask, n):
    from agentbom_amd.ops import native

    return native.bfs_parent_index(rev_d, mask, n)


def _words(t):
    return t.cpu().numpy().view(np.uint32)


# ── the index ───────────────────────────────────────────────────────────────

# (parent, child, type); mask 0b11.  Row of vertex:
#   0: no in-edge                        -> none
#   1: 5->1 type 5, 6->1 type 5          -> none (all masked)
#   2: 5->2 type 5, 6->2 type 0          -> 6, bit 31 clear
#   3: 7->3 type 0, 7->3 type 1          -> 7 | bit 31 (same parent twice)
#   4: 5->4 type 1, 6->4 type 0, 7->4 5  -> 5 | bit 31 (different parents)
#   8: 0->8 type 0                       -> 0 (vertex id 0 is a valid parent)
_ROWS = [(5, 1, 5), (6, 1, 5), (5, 2, 5), (6, 2, 0), (7, 3, 0), (7, 3, 1),
         (5, 4, 1), (6, 4, 0), (7, 4, 5), (0, 8, 0)]
_ROWS_N = 9


def _rows_graph(dev, typed=True):
    e = np.asarray(_ROWS, dtype=np.int64)
    fwd, rev = both_csr(e[:, 0], e[:, 1], e[:, 2] if typed else None, _ROWS_N)
    return rev, _to_dev(rev, dev)


def test_index_rows_by_hand(dev):
    rev, rev_d = _rows_graph(dev)
    idx = _index(rev_d, MASK, _ROWS_N)
    assert idx["allowed_mask"] == MASK
    got = _words(idx["first_parent"])
    want = np.array([PARENT_NONE, PARENT_NONE, 6, 7 | PARENT_MORE, 5 | PARENT_MORE,
                     PARENT_NONE, PARENT_NONE, PARENT_NONE, 0], dtype=np.uint32)
    assert np.array_equal(got, want)
    assert np.array_equal(parent_index_oracle(rev, MASK, _ROWS_N), want)


def test_index_without_edge_types(dev):
    """etype=None: every in-edge is allowed, whatever the mask says."""
    rev, rev_d = _rows_graph(dev, typed=False)
    got = _words(_index(rev_d, MASK, _ROWS_N)["first_parent"])
    want = np.array([PARENT_NONE, 5 | PARENT_MORE, 5 | PARENT_MORE, 7 | PARENT_MORE,
                     5 | PARENT_MORE, PARENT_NONE, PARENT_NONE, PARENT_NONE, 0],
                    dtype=np.uint32)
    assert np.array_equal(got, want)
    assert np.array_equal(parent_index_oracle(rev, MASK, _ROWS_N), want)


@pytest.mark.parametrize("n", [1, 257, 70_001])
@pytest.mark.parametrize("mask", [MASK, 0xFFFFFFFF, 0], ids=["mask3", "all", "none"])
def test_index_equals_oracle(dev, n, mask):
    src, dst, et = mixed_graph(n)
    _fwd, rev = both_csr(src, dst, et, n)
    got = _words(_index(_to_dev(rev, dev), mask, n)["first_parent"])
    assert np.array_equal(got, parent_index_oracle(rev, mask, n))


def test_index_mismatch_raises(dev):
    from agentbom_amd.ops import native

    rev, rev_d = _rows_graph(dev)
    idx = _index(rev_d, MASK, _ROWS_N)
    dist = torch.full((_ROWS_N,), -1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        native.bfs_level_bottom_up(rev_d, dist, 0, _ROWS_N, allowed_mask=0xFFFFFFFF,
                                   parent_index=idx)
    with pytest.raises(ValueError):
        native.bfs_level_bottom_up(rev_d, dist, 0, _ROWS_N - 1, allowed_mask=MASK,
                                   parent_index=idx)
    e = np.asarray(_ROWS, dtype=np.int64)
    fwd_d = _to_dev(both_csr(e[:, 0], e[:, 1], e[:, 2], _ROWS_N)[0], dev)
    src = torch.zeros(1, dtype=torch.int32, device=dev)
    for mask, n in ((0xFFFFFFFF, _ROWS_N), (MASK, _ROWS_N - 1)):
        with pytest.raises(ValueError):
            native.bfs(fwd_d["row_off"], fwd_d["col"], src, n, etype=fwd_d["etype"],
                       allowed_mask=mask, edge_src=fwd_d["src"], rev=rev_d, parent_index=idx)
    assert (dist == -1).all()
    with pytest.raises(ValueError):
        native.bfs_parent_index(rev_d, MASK, 2**31 - 1)


# ── one bottom-up pass ──────────────────────────────────────────────────────

@pytest.fixture(scope="module")
def passes(dev):
    """Per size: the reverse CSR, its index, a dist and what one pass at
    level 1 makes of it (from the definition and from the old kernel)."""
    from agentbom_amd.ops import native

    out = {}
    for n in SIZES:
        src, dst, et = mixed_graph(n)
        _fwd, rev = both_csr(src, dst, et, n)
        rev_d = _to_dev(rev, dev)
        dist = mixed_dist(n)
        want, claimed, opened = bottom_up_oracle(rev, MASK, n, dist, 1)
        old = torch.from_numpy(dist.view(np.int32)).to(dev)
        old_counts = native.bfs_level_bottom_up(rev_d, old, 1, n, allowed_mask=MASK)
        assert np.array_equal(_words(old), want)
        assert old_counts == (claimed, opened)
        out[n] = {"rev": rev_d, "index": _index(rev_d, MASK, n), "dist": dist, "want": want,
                  "counts": (claimed, opened)}
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset,index_offset",
                         [(0, "aligned"), (1, "aligned"), (1, "as_dist"), (3, "aligned"),
                          (3, "as_dist")],
                         ids=lambda v: v if isinstance(v, str) else "head%d" % ((4 - v) % 4))
def test_indexed_pass(dev, passes, n, offset, index_offset):
    """dist starts 0, 3 or 1 words before a 16-byte boundary and is longer
    than the graph; the index starts on a boundary or where dist does."""
    from agentbom_amd.ops import native

    p = passes[n]
    backing = torch.full((n + 16,), 123, dtype=torch.int32, device=dev)
    assert backing.data_ptr() % 16 == 0
    dist = backing[offset:offset + n + 7]
    dist[:n] = torch.from_numpy(p["dist"].view(np.int32)).to(dev)
    index = p["index"]
    if index_offset == "as_dist":
        moved = torch.empty(n + 4, dtype=torch.int32, device=dev)
        assert moved.data_ptr() % 16 == 0
        moved[offset:offset + n] = index["first_parent"]
        index = {"first_parent": moved[offset:offset + n], "allowed_mask": MASK}
    counts = native.bfs_level_bottom_up(p["rev"], dist, 1, n, allowed_mask=MASK,
                                        parent_index=index)
    assert counts == p["counts"]
    assert np.array_equal(_words(dist[:n]), p["want"])
    assert (backing[:offset] == 123).all() and (backing[offset + n:] == 123).all()
    if n > 1000:
        assert p["counts"][0] > n // 20 and p["counts"][1] > n // 20


def test_indexed_pass_knob_runs_the_old_kernel(dev, passes, monkeypatch):
    from agentbom_amd.ops import native

    p = passes[257]
    monkeypatch.setenv(KNOB, "0")
    dist = torch.from_numpy(p["dist"].view(np.int32)).to(dev)
    # an index of garbage: the pass must not read it
    junk = {"first_parent": torch.zeros(257, dtype=torch.int32, device=dev),
            "allowed_mask": MASK}
    assert native.bfs_level_bottom_up(p["rev"], dist, 1, 257, allowed_mask=MASK,
                                      parent_index=junk) == p["counts"]
    assert np.array_equal(_words(dist), p["want"])


def test_indexed_pass_rows_by_hand(dev):
    """Frontier = {10} at level 1.  Vertex 0: first parent 11 outside, later
    parent 10 inside (the row walk claims).  1: first parent 11 outside, no
    other (stays open).  2: 11 twice (bit 31, the walk finds nothing, open).
    3: parent 10, visited before the pass (kept).  4: parent 10 (claimed by
    the first parent).  5: only a masked edge from 10 (neither).  6: no
    in-edge."""
    from agentbom_amd.ops import native

    n = 12
    edges = [(11, 0, 0), (10, 0, 1), (11, 1, 0), (11, 2, 0), (11, 2, 1), (10, 3, 0),
             (10, 4, 0), (10, 5, 5)]
    e = np.asarray(edges, dtype=np.int64)
    _fwd, rev = both_csr(e[:, 0], e[:, 1], e[:, 2], n)
    rev_d = _to_dev(rev, dev)
    start = np.full(n, UNVISITED, dtype=np.uint32)
    start[10], start[3] = 1, 0
    want = start.copy()
    want[0], want[4] = 2, 2
    assert bottom_up_oracle(rev, MASK, n, start, 1)[1:] == (2, 2)
    for index in (None, _index(rev_d, MASK, n)):
        dist = torch.from_numpy(start.view(np.int32)).to(dev)
        counts = native.bfs_level_bottom_up(rev_d, dist, 1, n, allowed_mask=MASK,
                                            parent_index=index)
        assert counts == (2, 2)
        assert np.array_equal(_words(dist), want)


# ── native.bfs with the index: r06's level cases ────────────────────────────

def _graph(edges, n, dev):
    e = np.asarray(edges, dtype=np.int64)
    fwd, rev = both_csr(e[:, 0], e[:, 1], e[:, 2], n)
    return {"np": fwd, "fwd": _to_dev(fwd, dev), "rev": _to_dev(rev, dev), "n": n}


def _levels(g, dev, mask, monkeypatch):
    """dist and level count with the index, checked against cpu_ref.bfs and
    against the same call with the knob off."""
    from agentbom_amd.ops import cpu_ref, native

    fwd, c = g["fwd"], g["np"]
    ref = cpu_ref.bfs(c["row_off"], c["col"], np.asarray(SOURCES), g["n"], etype=c["etype"],
                      allowed_mask=mask)
    index = _index(g["rev"], mask, g["n"])
    got = {}
    for knob in ("1", "0"):
        monkeypatch.setenv(KNOB, knob)
        ws: dict = {}
        dist = native.bfs(fwd["row_off"], fwd["col"],
                          torch.tensor(SOURCES, dtype=torch.int32, device=dev), g["n"],
                          etype=fwd["etype"], allowed_mask=mask, edge_src=fwd["src"],
                          rev=g["rev"], workspace=ws, parent_index=index)
        assert np.array_equal(_words(dist), ref)
        got[knob] = ws["levels"]
    assert got["1"] == got["0"]
    return ref, got["1"]


def test_levels_estate_shape(dev, monkeypatch):
    dist, levels = _levels(_graph(estate_edges(), ESTATE_N, dev), dev, 0x1, monkeypatch)
    assert dist.max() == 2
    assert levels == 2


def test_levels_unreached_parent_keeps_the_loop_alive(dev, monkeypatch):
    parent, x = ESTATE_N, ESTATE_N + 1
    g = _graph(estate_edges() + [(parent, x, 0)], ESTATE_N + 2, dev)
    dist, levels = _levels(g, dev, 0x1, monkeypatch)
    assert dist[x] == UNVISITED and dist[parent] == UNVISITED
    assert levels == 3


@pytest.mark.parametrize("parent", [AGENTS, ESTATE_N], ids=["reached", "unreached"])
def test_levels_masked_in_edge(dev, monkeypatch, parent):
    x = ESTATE_N + 1
    g = _graph(estate_edges() + [(parent, x, 5)], ESTATE_N + 2, dev)
    dist, levels = _levels(g, dev, 0x1, monkeypatch)
    assert dist[x] == UNVISITED
    assert levels == 2


# ── the engine ──────────────────────────────────────────────────────────────

def test_step_with_and_without_the_index(dev, monkeypatch):
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=400, n_servers=2000, n_packages=120_000,
                          name_catalog=20_000, seed=99, arena_windows=40_000)
    eng = EstateEngine(est, device=dev)
    assert eng.bfs_parent_index["first_parent"].numel() == eng.N
    steps = [eng.step(), eng.step()]
    assert eng._bfs_ws["levels"] == 2
    monkeypatch.setenv(KNOB, "0")
    steps.append(eng.step())
    assert steps[0]["n_findings"] > 0
    for other in steps[1:]:
        assert other["n_findings"] == steps[0]["n_findings"]
        for key, value in steps[0].items():
            if isinstance(value, torch.Tensor):
                assert other[key].dtype == value.dtype, key
                assert torch.equal(other[key], value), key
