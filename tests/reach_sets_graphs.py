"""Hand-built graphs for per-source reach (``reach_hops``).

Each graph is an edge list with typed edges, a source list, a target list and
the UNBOUNDED hop count per (target, source) written by hand (255 = no path).
A BFS cut at ``max_depth`` records exactly the nodes within that distance, so
the expected output at any depth is the hand-written matrix with the cells
above the depth set to 255 (:meth:`ReachGraph.expected`).  Every graph aims at
one way the kernel can go wrong; see the builders.

``random_graph`` has no hand-written result: it is there for the source
counts that cross a lane word, a node's words and a pass (``SOURCE_COUNTS``).
"""

from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np

from agentbom_amd.graph.dependency_reach import _REACH_RELS
from agentbom_amd.graph.types import EntityType, RelationshipType
from agentbom_amd.ops import native

NO = 255
ALL_TYPES = 0xFFFFFFFF
DEPTHS = (0, 1, 3, 16)
# 1 bit, a word less one, a full word, a word and a bit, three words, and one
# source more than a pass of REACH_MAX_WORDS words holds
SOURCE_COUNTS = (1, 63, 64, 65, 130,
                 native.REACH_WORD_SOURCES * native.REACH_MAX_WORDS + 1)


@dataclass
class ReachGraph:
    name: str
    num_nodes: int
    edges: list          # (src, dst, etype)
    sources: list
    targets: list
    dist: list           # [T][S] unbounded hop counts, NO = unreachable
    mask: int = ALL_TYPES

    def csr(self):
        """(row_off int64 [N+1], col int32 [E], etype uint8 [E])."""
        e = np.asarray(self.edges, dtype=np.int64).reshape(-1, 3)
        o = np.argsort(e[:, 0], kind="stable")
        row_off = np.zeros(self.num_nodes + 1, dtype=np.int64)
        np.cumsum(np.bincount(e[:, 0], minlength=self.num_nodes), out=row_off[1:])
        return row_off, e[o, 1].astype(np.int32), e[o, 2].astype(np.uint8)

    def expected(self, max_depth: int) -> np.ndarray:
        d = np.asarray(self.dist, dtype=np.int64).reshape(len(self.targets), len(self.sources))
        return np.where(d <= max_depth, d, NO).astype(np.uint8)


def chain() -> ReachGraph:
    """0 -> 1 -> ... -> 19: longer than max_depth 16, so node 16 is recorded
    from source 0 and node 17 is not; the second source starts at node 5."""
    n = 20
    return ReachGraph(
        "chain", n, [(i, i + 1, 0) for i in range(n - 1)], [0, 5], list(range(n)),
        [[t, t - 5 if t >= 5 else NO] for t in range(n)])


def diamond_cycle() -> ReachGraph:
    """A = 0 reaches 4 over two 2-hop arms, B = 1 in one hop; 2 -> 4 -> 5 -> 2
    is a cycle, so a walk that re-enters seen nodes never ends or relabels."""
    edges = [(0, 2, 0), (0, 3, 0), (2, 4, 0), (3, 4, 0), (1, 4, 0), (4, 5, 0), (5, 2, 0)]
    return ReachGraph(
        "diamond_cycle", 6, edges, [0, 1], [4, 5, 2, 0, 3],
        [[2, 1],
         [3, 2],
         [1, 3],
         [0, NO],
         [1, NO]])


def edge_filter() -> ReachGraph:
    """0 -> 3 directly over type 5, which the mask leaves out; the allowed
    path 0 -> 1 -> 2 -> 3 takes three hops."""
    edges = [(0, 3, 5), (0, 1, 0), (1, 2, 1), (2, 3, 0)]
    return ReachGraph("edge_filter", 4, edges, [0], [3, 1, 2], [[3], [1], [2]],
                      mask=(1 << 0) | (1 << 1))


def source_setup() -> ReachGraph:
    """Sources that are targets (hop 0), source 0 twice, source 2 without
    out-edges and source 3 without any edge."""
    return ReachGraph(
        "source_setup", 5, [(0, 1, 0), (1, 2, 0)], [0, 0, 2, 3, 1], [0, 1, 2, 3],
        [[0, 0, NO, NO, NO],
         [1, 1, NO, NO, 0],
         [2, 2, 0, NO, 1],
         [NO, NO, NO, 0, NO]])


def star() -> ReachGraph:
    """Hub 0 with 300 leaves, far above the degree at which a row goes to the
    wave-per-row expand; 301 -> hub, and leaf 300 -> 302 one level further."""
    leaves = list(range(1, 301))
    edges = [(0, leaf, 0) for leaf in leaves] + [(301, 0, 0), (300, 302, 0)]
    targets = [0] + leaves + [302]
    dist = [[0, 1]] + [[1, 2] for _ in leaves] + [[2, 3]]
    return ReachGraph("star", 303, edges, [0, 301], targets, dist)


# REACH_STAGE (csrc/reach_sets.hip, 4096 entries of a block's LDS append
# queue) less one, exactly, and one more
STAGE_STAR_LEAVES = (4095, 4096, 4097)


def stage_star(leaves: int) -> ReachGraph:
    """Hub 0 with ``leaves`` distinct leaves, every leaf a target: one wave of
    the wave-per-row expand pushes all of them through one block's LDS queue,
    the ones past its capacity straight to the global queue."""
    ids = list(range(1, leaves + 1))
    return ReachGraph(f"stage_star_{leaves}", leaves + 1, [(0, leaf, 0) for leaf in ids],
                      [0], ids, [[1] for _ in ids])


def no_in_edges() -> ReachGraph:
    """Target 2 has out-edges only: its row is all 255."""
    return ReachGraph("no_in_edges", 3, [(0, 1, 0), (2, 1, 0)], [0, 1], [2, 1],
                      [[NO, NO], [1, 0]])


GRAPHS = (chain, diamond_cycle, edge_filter, source_setup, star, no_in_edges)


def random_graph(seed: int = 7):
    """200 nodes, 700 random typed edges (types 0..3, type 3 masked out).
    Returns (num_nodes, row_off, col, etype, mask)."""
    rng = np.random.default_rng(seed)
    n, m = 200, 700
    g = ReachGraph("random", n,
                   list(zip(rng.integers(0, n, m).tolist(), rng.integers(0, n, m).tolist(),
                            rng.integers(0, 4, m).tolist())), [], [], [])
    return (n, *g.csr(), 0b0111)


def random_sources(count: int, num_nodes: int = 200, seed: int = 11) -> np.ndarray:
    """``count`` node ids drawn with replacement: duplicates are part of it."""
    return np.random.default_rng(seed + count).integers(0, num_nodes, count).astype(np.int32)


# small, yet with agents whose row passes the heavy-row degree (checked by the tests)
ESTATE_ARGS = dict(n_agents=200, n_servers=1500, n_packages=3000, name_catalog=600, seed=5)


def estate_agents(estate, count: int = 130, seed: int = 3) -> np.ndarray:
    """``count`` distinct agent node ids, the widest agent first."""
    deg = np.bincount(estate.edge_src[estate.edge_src < estate.n_agents],
                      minlength=estate.n_agents)
    widest = int(np.argmax(deg))
    rest = np.random.default_rng(seed).permutation(estate.n_agents)
    rest = rest[rest != widest][:count - 1]
    return (np.concatenate([[widest], rest]) + estate.agent_base).astype(np.int32)


def edited_demo_graph(demo_graph):
    """The demo graph with one agent's USES edge made non-traversable and one
    server -> package edge made bidirectional."""
    g = copy.deepcopy(demo_graph)
    uses = [e for e in g.edges if e.relationship == RelationshipType.USES
            and g.nodes[e.source].entity_type == EntityType.AGENT]
    uses[0].traversable = False
    back = next(e for e in g.edges if e.relationship in _REACH_RELS
                and g.nodes[e.target].entity_type == EntityType.PACKAGE and not e.bidirectional)
    back.bidirectional = True
    g._adj[back.target].append(g.edges.index(back))
    g._radj[back.source].append(g.edges.index(back))
    return g
