"""Edge lists shared by tests/test_components_cpu.py and
tests/test_components_gpu.py, and an independent labelling to hold the
oracle against.  Every graph is ``(src int32 [E], dst int32 [E], n)``.
"""

from __future__ import annotations

from collections import deque

import numpy as np

from agentbom_amd.graph.container import UnifiedEdge, UnifiedGraph, UnifiedNode
from agentbom_amd.graph.types import EntityType, RelationshipType

RANDOM_SEED = 4


def _edges(pairs, n: int):
    src = np.array([p[0] for p in pairs], dtype=np.int32)
    dst = np.array([p[1] for p in pairs], dtype=np.int32)
    return src, dst, n


def no_edges(n: int):
    return _edges([], n)


def zigzag(n: int = 4097):
    """One chain visiting 0, n-1, 1, n-2, ...: consecutive links alternate
    between a much larger and a much smaller id."""
    order, lo, hi = [], 0, n - 1
    while lo <= hi:
        order.append(lo)
        if lo != hi:
            order.append(hi)
        lo, hi = lo + 1, hi - 1
    assert sorted(order) == list(range(n))
    return _edges(list(zip(order, order[1:])), n)


def contended_root(n: int = 8193):
    """The hub is the largest id and has an edge to each of n-1 leaves: every
    edge hooks the same root at once."""
    return _edges([(n - 1, leaf) for leaf in range(n - 1)], n)


def comb(hub_first: bool, chains: int = 500, length: int = 9):
    """``chains`` disjoint chains of ``length`` nodes; one node of largest id
    is joined to the last node of every chain.  The hub's edges come first or
    last in the edge list."""
    hub = chains * length
    teeth = [(c * length + i, c * length + i + 1)
             for c in range(chains) for i in range(length - 1)]
    spine = [(hub, c * length + length - 1) for c in range(chains)]
    return _edges(spine + teeth if hub_first else teeth + spine, hub + 1)


def sparse_random(seed: int = RANDOM_SEED):
    """n=1031, m=600: 540 uniform edges, 20 self-loops, 40 parallel copies
    (half of them reversed)."""
    rng = np.random.default_rng(seed)
    n = 1031
    src = rng.integers(0, n, 540)
    dst = rng.integers(0, n, 540)
    loops = rng.integers(0, n, 20)
    par = rng.integers(0, 540, 40)
    par_src = np.concatenate([src[par[:20]], dst[par[20:]]])
    par_dst = np.concatenate([dst[par[:20]], src[par[20:]]])
    src = np.concatenate([src, loops, par_src])
    dst = np.concatenate([dst, loops, par_dst])
    shuffle = rng.permutation(600)
    assert len(src) == 600
    return src[shuffle].astype(np.int32), dst[shuffle].astype(np.int32), n


GRAPHS = {
    "no_edges_130": lambda: no_edges(130),
    "single_node": lambda: no_edges(1),
    "zigzag_4097": zigzag,
    "zigzag_4097_reversed": lambda: (lambda s, d, n: (d, s, n))(*zigzag()),
    "contended_root_8193": contended_root,
    "comb_hub_first": lambda: comb(True),
    "comb_hub_last": lambda: comb(False),
    "sparse_random": sparse_random,
}

# graphs that are one component: every label is 0
ALL_ZERO = ("zigzag_4097", "zigzag_4097_reversed", "contended_root_8193",
            "comb_hub_first", "comb_hub_last")


def bfs_labels(src, dst, n: int) -> np.ndarray:
    """Smallest id of every node's component by plain breadth-first search:
    nodes are visited in ascending order, so the first node that reaches a
    component is its smallest."""
    adj: list[list[int]] = [[] for _ in range(n)]
    for u, v in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        adj[u].append(v)
        adj[v].append(u)
    labels = [-1] * n
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s] = s
        queue = deque([s])
        while queue:
            u = queue.popleft()
            for w in adj[u]:
                if labels[w] < 0:
                    labels[w] = s
                    queue.append(w)
    return np.array(labels, dtype=np.int32)


def unified_80() -> UnifiedGraph:
    """80 nodes and 240 random edges (duplicates of one relationship collapse
    in add_edge), built like the centrality tests' graph; every third edge is
    a USES edge so that ``relationships`` has something to select."""
    rng = np.random.default_rng(80)
    g = UnifiedGraph()
    for i in range(80):
        g.add_node(UnifiedNode(id=f"u{i:02d}", entity_type=EntityType.PACKAGE, label=str(i)))
    for k in range(240):
        u, v = (int(x) for x in rng.integers(0, 80, 2))
        rel = RelationshipType.USES if k % 3 == 0 else RelationshipType.DEPENDS_ON
        e = UnifiedEdge(f"u{u:02d}", f"u{v:02d}", rel)
        e.bidirectional = k % 7 == 0
        e.traversable = k % 5 != 0
        g.add_edge(e)
    return g


def unified_bfs_components(g: UnifiedGraph, relationships=None) -> dict[str, str]:
    """Node id -> smallest id of its component, straight off the edge list."""
    ids = sorted(g.nodes)
    pos = {nid: i for i, nid in enumerate(ids)}
    edges = [e for e in g.edges if relationships is None or e.relationship in relationships]
    labels = bfs_labels([pos[e.source] for e in edges], [pos[e.target] for e in edges], len(ids))
    return {nid: ids[labels[i]] for i, nid in enumerate(ids)}
