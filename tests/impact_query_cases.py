"""Inputs, expected values and the one checker for the impact-query tests
(ops/csrc/query.hip, ``impact_query_kernel``).  numpy only: the ``_cpu``
module pins the oracle and the preconditions of every case, the ``_gpu``
module runs the kernel on the same cases.

The kernel's three caps, which the cases sit on:

- the visited set is an 8192-slot LDS hash, ``slot(v) = (v * 2654435761) &
  8191`` in uint32, linear probing, at most 64 probes; a node whose chain
  fails is dropped and the query flagged;
- a level holds at most 2048 new nodes; one past that is reported but not
  expanded, and the query flagged;
- a query reports at most ``max_nodes`` entries; more sets the flag.

2654435761 is odd, so ``slot`` is a bijection on residues mod 8192: ids
below 8192 never collide, ids congruent mod 8192 always do.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

from agentbom_amd.graph.backend import csr_arrays
from agentbom_amd.ops import cpu_ref

IQ_HASH = 8192       # csrc/query.hip
IQ_FRONTIER = 2048
IQ_PROBES = 64
IQ_GRID = 2048       # abom_impact_query caps the grid here
UNBOUNDED = 1 << 30


def slot(v) -> np.ndarray:
    """The kernel's hash, in numpy uint32 (the multiply wraps as on device)."""
    v = np.atleast_1d(np.asarray(v, dtype=np.int64)).astype(np.uint32)
    return (v * np.uint32(2654435761)) & np.uint32(IQ_HASH - 1)


def max_probes(nodes) -> int:
    """Upper bound, over every insertion order, of the probes any of ``nodes``
    needs in an unbounded linear-probe table of IQ_HASH slots.

    The set of occupied slots after all insertions does not depend on the
    order.  A key inserted while the table is a subset of that final set stops
    before the first finally-free slot at or after its home, so it needs at
    most (that slot - home) probes, cyclically."""
    homes = slot(list(nodes)).astype(np.int64)
    assert len(homes) < IQ_HASH
    used = np.zeros(IQ_HASH, dtype=bool)
    for h in homes.tolist():
        while used[h]:
            h = (h + 1) & (IQ_HASH - 1)
        used[h] = True
    worst = 0
    for h in set(homes.tolist()):
        d = 0
        while used[(h + d) & (IQ_HASH - 1)]:
            d += 1
        worst = max(worst, d)
    return worst


class Graph:
    """Host CSR of an edge list; ``etype`` (one code per input edge) is put
    into CSR order the way the engine's builders do."""

    def __init__(self, src, dst, n: int, etype=None):
        self.n = n
        self.src = np.asarray(src, dtype=np.int64)
        self.dst = np.asarray(dst, dtype=np.int64)
        self.row_off, self.col = csr_arrays(self.src, self.dst, n)
        self.etype = None
        if etype is not None:
            order = np.argsort(self.src, kind="stable")
            self.etype = np.asarray(etype, dtype=np.uint8)[order]

    @classmethod
    def from_csr(cls, row_off, col) -> "Graph":
        g = cls([], [], 0)
        g.n, g.row_off, g.col = len(row_off) - 1, np.asarray(row_off), np.asarray(col)
        return g

    def oracle(self, sources, *, masked: bool, mask: int, max_hops: int) -> list[dict]:
        """{node: hop} per source from cpu_ref.impact_query with no node cap;
        one oracle run per distinct source."""
        distinct = sorted(set(int(s) for s in sources))
        ref = cpu_ref.impact_query(
            self.row_off, self.col, np.asarray(distinct, dtype=np.int64),
            etype=self.etype if masked else None, allowed_mask=mask,
            max_hops=max_hops, max_nodes=UNBOUNDED)
        assert not any(trunc for _, trunc in ref)
        by_source = {s: hops for s, (hops, _) in zip(distinct, ref)}
        return [by_source[int(s)] for s in sources]


@dataclass
class Case:
    name: str
    graph: Graph
    sources: np.ndarray           # [Q] node ids
    max_hops: int
    max_nodes: int
    expected_trunc: np.ndarray    # [Q] 0/1
    masked: bool = False          # pass the graph's etype to the kernel
    mask: int = 0xFFFFFFFF
    # truncated queries: the exact count the case derives, per query
    expected_count: dict = field(default_factory=dict)
    # truncated queries: {query: {node: hop}} that must be reported
    must_report: dict = field(default_factory=dict)
    _oracle: Optional[list] = None

    @property
    def oracle(self) -> list[dict]:
        if self._oracle is None:
            self._oracle = self.graph.oracle(
                self.sources, masked=self.masked, mask=self.mask, max_hops=self.max_hops)
        return self._oracle

    def exact(self) -> np.ndarray:
        return np.flatnonzero(np.asarray(self.expected_trunc) == 0)


def fits(hops: dict, max_nodes: int) -> bool:
    """True when the kernel can truncate nothing on this neighbourhood: it is
    no larger than the slab, no level brings more than IQ_FRONTIER new nodes,
    and no probe chain can pass IQ_PROBES."""
    levels = np.bincount(list(hops.values()))
    return (len(hops) <= max_nodes and int(levels[1:].max(initial=0)) <= IQ_FRONTIER
            and max_probes(hops.keys()) <= IQ_PROBES)


def check_case(case: Case, nodes, hops, counts, trunc) -> None:
    """Every query of ``case`` against its oracle; ``nodes`` [Q, max_nodes],
    ``hops`` [Q, max_nodes], ``counts`` [Q], ``trunc`` [Q] as numpy arrays."""
    nodes = np.asarray(nodes).reshape(len(case.sources), -1)
    hops = np.asarray(hops).reshape(len(case.sources), -1)
    assert len(counts) == len(trunc) == len(case.sources)
    for q in range(len(case.sources)):
        check_query(
            nodes[q], hops[q], int(counts[q]), int(trunc[q]),
            source=int(case.sources[q]), oracle=case.oracle[q],
            max_hops=case.max_hops, max_nodes=case.max_nodes,
            expected_trunc=int(case.expected_trunc[q]),
            expected_count=case.expected_count.get(q),
            must_report=case.must_report.get(q),
            where=f"{case.name} query {q}")


def check_query(nodes_row, hops_row, count: int, trunc: int, *, source: int, oracle: dict,
                max_hops: int, max_nodes: int, expected_trunc: int,
                expected_count: Optional[int] = None, must_report: Optional[dict] = None,
                where: str = "") -> None:
    """The one checker.  ``expected_trunc`` is an input; no query is skipped."""
    assert trunc == expected_trunc, f"{where}: truncated {trunc}, expected {expected_trunc}"
    assert 0 < count <= max_nodes, f"{where}: count {count}"
    got_nodes = np.asarray(nodes_row[:count]).astype(np.int64).tolist()
    got_hops = np.asarray(hops_row[:count]).astype(np.int64).tolist()
    assert got_nodes[0] == source and got_hops[0] == 0, f"{where}: entry 0 is not the source"
    got = dict(zip(got_nodes, got_hops))
    if len(got) != count:
        twice = sorted(v for v in got if got_nodes.count(v) > 1)
        where_ = [(i, h) for i, (v, h) in enumerate(zip(got_nodes, got_hops)) if v == twice[0]]
        raise AssertionError(f"{where}: duplicate nodes reported: {twice[:8]}; "
                             f"node {twice[0]} at (entry, hop) {where_}")
    if not expected_trunc:
        assert count == len(oracle), f"{where}: count {count}, oracle {len(oracle)}"
        assert got == oracle, f"{where}: reported neighbourhood differs from the oracle"
        return
    assert expected_count is not None, f"{where}: a truncating case derives its count"
    assert count == expected_count, f"{where}: count {count}, derived {expected_count}"
    for node, hop in got.items():
        assert node in oracle, f"{where}: node {node} outside the true neighbourhood"
        assert oracle[node] <= hop <= max_hops, (
            f"{where}: hop {hop} for node {node}, oracle {oracle[node]}")
    for node, hop in (must_report or {}).items():
        assert got.get(node) == hop, f"{where}: node {node} at hop {got.get(node)}, not {hop}"


# ── graphs ──────────────────────────────────────────────────────────────────

RAND_N = 1000
RAND_SINK = 999       # no out-edges
RAND_SELF = 998       # only a self-loop
RAND_SOURCES = np.array([0, 1, 2, 17, 101, 250, 333, 404, 512, 640, 777, 850, 901,
                         997, RAND_SELF, RAND_SINK], dtype=np.int64)


def _random_edges():
    rng = np.random.default_rng(20240607)
    src = rng.integers(0, RAND_N, 5800)
    dst = rng.integers(0, RAND_N, 5800)
    # parallel edges, self-loops, a cycle through source 0
    src = np.concatenate([src, src[:150], np.arange(0, 40), [0, 1, 2]])
    dst = np.concatenate([dst, dst[:150], np.arange(0, 40), [1, 2, 0]])
    keep = (src != RAND_SINK) & (src != RAND_SELF)
    src = np.concatenate([src[keep], [RAND_SELF]])
    dst = np.concatenate([dst[keep], [RAND_SELF]])
    return src, dst


@lru_cache(maxsize=None)
def random_graph() -> Graph:
    """Seeded digraph, n = 1000, m ~ 6000, etype = edge index % 3."""
    src, dst = _random_edges()
    return Graph(src, dst, RAND_N, etype=np.arange(len(src)) % 3)


def _untruncated(q: int) -> np.ndarray:
    return np.zeros(q, dtype=np.uint8)


# ── case 1: edge-type mask ──────────────────────────────────────────────────

@lru_cache(maxsize=None)
def mask_cases() -> tuple[Case, ...]:
    g = random_graph()
    cases = [Case(f"mask {m:#05b}", g, RAND_SOURCES, 4, 4096, _untruncated(16),
                  masked=True, mask=m) for m in (0b111, 0b101, 0b010, 0)]
    # without etype the mask must be ignored
    cases.append(Case("no etype, mask 0", g, RAND_SOURCES, 4, 4096, _untruncated(16),
                      masked=False, mask=0))
    return tuple(cases)


# ── case 2: hops ────────────────────────────────────────────────────────────

CHAIN_N = 300


@lru_cache(maxsize=None)
def hop_cases() -> tuple[Case, ...]:
    g = random_graph()
    chain = Graph(np.arange(CHAIN_N - 1), np.arange(1, CHAIN_N), CHAIN_N)
    return (
        Case("max_hops 0", g, RAND_SOURCES, 0, 4096, _untruncated(16)),
        Case("max_hops 1", g, RAND_SOURCES, 1, 4096, _untruncated(16)),
        Case("chain, max_hops 255", chain, np.array([0, 44, CHAIN_N - 1]), 255, 512,
             _untruncated(3)),
    )


# ── case 3: max_nodes edges ─────────────────────────────────────────────────

CAP_SOURCE = 17


@lru_cache(maxsize=None)
def max_nodes_cases() -> tuple[Case, ...]:
    g = random_graph()
    size = len(g.oracle([CAP_SOURCE], masked=False, mask=0, max_hops=4)[0])
    one = np.array([CAP_SOURCE], dtype=np.int64)
    # max_nodes = 1: truncated iff the source has a neighbour other than itself
    lone = np.array([CAP_SOURCE, 0, RAND_SELF, RAND_SINK], dtype=np.int64)
    lone_trunc = np.array([1, 1, 0, 0], dtype=np.uint8)
    return (
        Case("max_nodes = S", g, one, 4, size, _untruncated(1)),
        Case("max_nodes = S - 1", g, one, 4, size - 1, np.ones(1, dtype=np.uint8),
             expected_count={0: size - 1}),
        Case("max_nodes = 1", g, lone, 4, 1, lone_trunc, expected_count={0: 1, 1: 1}),
    )


# ── case 5: frontier cap ────────────────────────────────────────────────────

def star_edges(leaves: int, base: int = 0, shared_sink: bool = False):
    """base -> ``leaves`` leaves; leaf i -> its own grandchild, or all leaves
    -> one sink.  Ids base .. base + 2 * leaves (or base + leaves + 1)."""
    leaf = base + 1 + np.arange(leaves)
    below = np.full(leaves, base + leaves + 1) if shared_sink else leaf + leaves
    return (np.concatenate([np.full(leaves, base), leaf]), np.concatenate([leaf, below]))


STAR_MAX_NODES = 8192


@lru_cache(maxsize=None)
def frontier_cases() -> tuple[Case, ...]:
    full, over = IQ_FRONTIER, IQ_FRONTIER + 1
    source = np.zeros(1, dtype=np.int64)
    leaves_at_1 = {v: 1 for v in range(1, over + 1)}
    return (
        Case("star, 2048 leaves", Graph(*star_edges(full), 2 * full + 1), source, 3,
             STAR_MAX_NODES, _untruncated(1)),
        # every leaf is reported; the 2049th is not expanded, so exactly 2048
        # grandchildren follow
        Case("star, 2049 leaves", Graph(*star_edges(over), 2 * over + 1), source, 3,
             STAR_MAX_NODES, np.ones(1, dtype=np.uint8),
             expected_count={0: 1 + over + full}, must_report={0: leaves_at_1}),
        Case("star, 2049 leaves, one sink",
             Graph(*star_edges(over, shared_sink=True), over + 2), source, 3,
             STAR_MAX_NODES, np.ones(1, dtype=np.uint8),
             expected_count={0: 1 + over + 1},
             must_report={0: {**leaves_at_1, over + 1: 2}}),
    )


# ── case 6: probe limit ─────────────────────────────────────────────────────

PROBE_HOME = IQ_HASH - 7          # the chain wraps from slot 8191 to slot 0
PROBE_SOURCE_SLOT = 4000          # far from the chain
PROBE_MAX_NODES = 128


def _id_with_slot(s: int) -> int:
    """The id below 8192 that hashes to slot ``s`` (slot is a bijection there)."""
    return int(np.flatnonzero(slot(np.arange(IQ_HASH)) == s)[0])


PROBE_R = _id_with_slot(PROBE_HOME)
PROBE_FREE_FIT = _id_with_slot(PROBE_SOURCE_SLOT)
PROBE_FREE_OVER = _id_with_slot(PROBE_SOURCE_SLOT + 1)
PROBE_SHARED_FIT = PROBE_R + IQ_HASH * 66      # sources in the chain's own slot
PROBE_SHARED_OVER = PROBE_R + IQ_HASH * 67
PROBE_N = IQ_HASH * 68


def probe_neighbours(k: int) -> np.ndarray:
    return PROBE_R + IQ_HASH * np.arange(k, dtype=np.int64)


@lru_cache(maxsize=None)
def probe_cases() -> tuple[Case, ...]:
    """One source whose neighbours all hash to PROBE_HOME.  A source in a
    free slot leaves the chain 64 slots: 64 neighbours fit, the 65th fails.
    A source in PROBE_HOME takes the first of them: 63 fit, the 64th fails."""
    fan = ((PROBE_FREE_FIT, 64), (PROBE_FREE_OVER, 65),
           (PROBE_SHARED_FIT, 63), (PROBE_SHARED_OVER, 64))
    src = np.concatenate([np.full(k, s) for s, k in fan])
    dst = np.concatenate([probe_neighbours(k) for _, k in fan])
    g = Graph(src, dst, PROBE_N)
    sources = np.array([s for s, _ in fan], dtype=np.int64)
    return (Case("probe limit", g, sources, 2, PROBE_MAX_NODES,
                 np.array([0, 1, 0, 1], dtype=np.uint8),
                 expected_count={1: 65, 3: 64}),)


# ── case 7: two queries per block ───────────────────────────────────────────

BATCH_Q = IQ_GRID + 37
BATCH_STAR = RAND_N                               # the 2049-leaf star of case 5
BATCH_ISOLATED = BATCH_STAR + 2 * (IQ_FRONTIER + 1) + 1
BATCH_N = BATCH_ISOLATED + 37
BATCH_MAX_NODES = 4100                            # the star reports 4098
BATCH_FILL = 128                                  # distinct fill sources


@lru_cache(maxsize=None)
def batch_cases() -> tuple[Case, ...]:
    """Queries q and q + 2048 share a block.  The star truncates (frontier
    cap) and fills half the hash; the isolated node after it must come back
    with count 1 and a clear flag, and the star after an isolated node whole."""
    over = IQ_FRONTIER + 1
    rs, rd = _random_edges()
    ss, sd = star_edges(over, base=BATCH_STAR)
    g = Graph(np.concatenate([rs, ss]), np.concatenate([rd, sd]), BATCH_N)
    star = np.full(37, BATCH_STAR, dtype=np.int64)
    isolated = BATCH_ISOLATED + np.arange(37, dtype=np.int64)
    fill = (np.arange(IQ_GRID - 37, dtype=np.int64) * 7) % BATCH_FILL
    leaves_at_1 = {BATCH_STAR + v: 1 for v in range(1, over + 1)}
    cases = []
    for name, first, last in (("star then isolated", star, isolated),
                              ("isolated then star", isolated, star)):
        sources = np.concatenate([first, fill, last])
        trunc = (sources == BATCH_STAR).astype(np.uint8)
        stars = np.flatnonzero(trunc).tolist()
        cases.append(Case(
            f"2085 queries, {name}", g, sources, 3, BATCH_MAX_NODES, trunc,
            expected_count={q: 1 + over + IQ_FRONTIER for q in stars},
            must_report={q: leaves_at_1 for q in stars}))
    return tuple(cases)


# ── the seed of the visited set ─────────────────────────────────────────────

@lru_cache(maxsize=None)
def seed_cases() -> tuple[Case, ...]:
    """All 256 threads of a block clear the hash, then thread 0 seeds the
    source's slot.  If the seed could land before another wave's clear of
    that slot, the source would leave the visited set and its self-loop would
    report it a second time.  One query per block, every source with a
    self-loop and in one of the 64 slots that the last wave clears last."""
    ids = np.arange(IQ_HASH, dtype=np.int64)
    g = Graph(np.concatenate([ids, ids]), np.concatenate([ids, (ids + 1) % IQ_HASH]), IQ_HASH)
    late = ids[slot(ids) >= IQ_HASH - 64]
    return (Case("seed survives the clear", g, np.resize(late, IQ_GRID), 2, 8,
                 _untruncated(IQ_GRID)),)


# ── case 8: engine path ─────────────────────────────────────────────────────

ENGINE_HOPS = 3
ENGINE_MAX_NODES = 4096


@lru_cache(maxsize=None)
def engine_estate():
    from agentbom_amd.scan.synth import generate_estate

    return generate_estate(n_agents=50, n_servers=200, n_packages=5000,
                           name_catalog=800, seed=3, arena_windows=1600)


def engine_case(row_off, col) -> Case:
    """16 package queries on the engine's reverse CSR (host arrays)."""
    est = engine_estate()
    g = Graph.from_csr(row_off, col)
    sources = np.array([est.pkg_base + i * 313 % est.n_packages for i in range(16)],
                       dtype=np.int64)
    return Case("engine", g, sources, ENGINE_HOPS, ENGINE_MAX_NODES, _untruncated(16))
