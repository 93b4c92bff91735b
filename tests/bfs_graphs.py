"""Graphs and numpy oracles shared by the parent-index and expand-group tests
of the reach BFS (no GPU needed to import)."""

from __future__ import annotations

import numpy as np

UNVISITED = 0xFFFFFFFF
PARENT_NONE = 0xFFFFFFFF
PARENT_MORE = 0x80000000


def csr(src, dst, et, n):
    """CSR by stable sort on source (as EstateEngine._build_csr); ``et`` None
    gives a graph without edge types."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    row_off = np.zeros(n + 1, dtype=np.int64)
    row_off[1:] = np.cumsum(np.bincount(src, minlength=n))
    out = {"row_off": row_off, "col": dst[order].astype(np.int32),
           "src": src[order].astype(np.int32), "etype": None}
    if et is not None:
        out["etype"] = np.asarray(et, dtype=np.uint8)[order]
    return out


def both_csr(src, dst, et, n):
    """(forward, reverse) host CSRs of an edge list."""
    return csr(src, dst, et, n), csr(dst, src, et, n)


def _allowed(rev, mask):
    if rev["etype"] is None:
        return np.ones(len(rev["col"]), dtype=bool)
    return ((mask >> rev["etype"].astype(np.int64)) & 1).astype(bool)


def _rows(rev, n):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(rev["row_off"]))


def parent_index_oracle(rev, mask, n):
    """first_parent from its definition: the source of the first allowed
    in-edge in reverse-row order, bit 31 when the row holds another allowed
    in-edge, 0xFFFFFFFF when it holds none."""
    ok = _allowed(rev, mask)
    rows = _rows(rev, n)[ok]
    cols = rev["col"].astype(np.int64)[ok]
    out = np.full(n, PARENT_NONE, dtype=np.uint32)
    first_row, first_at = np.unique(rows, return_index=True)  # rows are sorted
    out[first_row] = cols[first_at].astype(np.uint32)
    more = np.bincount(rows, minlength=n) > 1
    out[more] |= np.uint32(PARENT_MORE)
    return out


def bottom_up_oracle(rev, mask, n, dist, cur_level):
    """One bottom-up pass from its definition.  Returns (dist after the pass,
    claimed, open): open = left unvisited with an allowed in-edge."""
    dist = dist.copy()
    ok = _allowed(rev, mask)
    rows = _rows(rev, n)[ok]
    cols = rev["col"].astype(np.int64)[ok]
    unvisited = dist[:n] == UNVISITED
    has_edge = np.zeros(n, dtype=bool)
    has_edge[rows] = True
    hit = np.zeros(n, dtype=bool)
    hit[rows[dist[cols] == cur_level]] = True
    claim = unvisited & hit
    dist[:n][claim] = cur_level + 1
    return dist, int(claim.sum()), int((unvisited & has_edge & ~claim).sum())


def mixed_graph(n, seed=0):
    """n vertices; vertex v has v % 4 in-edges from seeded random parents with
    types from {0, 1, 5}.  Under mask 0b11 that gives rows with no in-edge,
    rows masked entirely, a masked first edge, one and several allowed
    parents.  Returns (src, dst, et)."""
    rng = np.random.default_rng([seed, n])
    k = np.arange(n, dtype=np.int64) % 4
    dst = np.repeat(np.arange(n, dtype=np.int64), k)
    src = rng.integers(0, n, size=len(dst), dtype=np.int64)
    et = rng.choice(np.array([0, 1, 5], dtype=np.uint8), size=len(dst))
    return src, dst, et


def mixed_dist(n, seed=0):
    """A dist for ``mixed_graph``: a third of the vertices at level 1 (the
    frontier), a sixth at level 0, the rest unvisited."""
    rng = np.random.default_rng([seed + 1, n])
    r = rng.integers(0, 6, size=n)
    dist = np.full(n, UNVISITED, dtype=np.uint32)
    dist[r < 2] = 1
    dist[r == 2] = 0
    return dist


# r06's level cases: 4 agents -> 8 servers each -> 20 leaves each.  E = 672,
# the agents' 32 edges stay under E/8 (level 1 sparse), the servers' 640 are
# over it (level 2 bottom-up).  Agents 0-3, servers 4-35, leaves 36-675.
AGENTS, SERVERS, LEAVES = 4, 32, 640
ESTATE_N = AGENTS + SERVERS + LEAVES
SOURCES = tuple(range(AGENTS))


def estate_edges():
    edges = [(a, AGENTS + 8 * a + k, 0) for a in range(AGENTS) for k in range(8)]
    edges += [(AGENTS + s, AGENTS + SERVERS + 20 * s + k, 0)
              for s in range(SERVERS) for k in range(20)]
    return edges


def fan_edges(frontier, degree):
    """0 -> `frontier` vertices -> `degree` distinct leaves each."""
    src = [np.zeros(frontier, dtype=np.int64),
           np.repeat(np.arange(1, frontier + 1, dtype=np.int64), degree)]
    dst = [np.arange(1, frontier + 1, dtype=np.int64),
           frontier + 1 + np.arange(frontier * degree, dtype=np.int64)]
    return np.concatenate(src), np.concatenate(dst), 1 + frontier + frontier * degree
