"""Graph-analytics backend protocol: PageRank, betweenness centrality and
connected components.

Reference parity: src/agent_bom/graph_backend.py:25 — an optional analytics
backend behind a Protocol, NetworkX when installed, with the container's
built-in approximations otherwise.  MI355X build ships a NATIVE numpy
backend as the default (power-iteration PageRank, Brandes betweenness on a
bounded sample) so the analytics work in the air-gapped image where
networkx is absent; the NetworkX adapter remains for environments that
have it (``AGENT_BOM_GRAPH_BACKEND=networkx``).  ``hip`` runs the same
analytics as HIP kernels (ops/csrc/centrality.hip, ops/csrc/components.hip)
where a GPU and the built engine are present.
"""

from __future__ import annotations

import os
from typing import Protocol, runtime_checkable

import numpy as np


@runtime_checkable
class GraphBackendProtocol(Protocol):
    """What an analytics backend must provide over a UnifiedGraph."""

    name: str

    def pagerank(self, graph, damping: float = 0.85,
                 iterations: int = 50) -> dict[str, float]: ...

    def betweenness(self, graph, sample: int = 64) -> dict[str, float]: ...

    def components(self, graph, relationships=None) -> dict[str, str]: ...


class NativeBackend:
    """Numpy analytics over the in-RAM adjacency — no third-party deps."""

    name = "native"

    @staticmethod
    def _index(graph) -> tuple[list[str], dict[str, int]]:
        ids = sorted(graph.nodes)
        return ids, {nid: i for i, nid in enumerate(ids)}

    def pagerank(self, graph, damping: float = 0.85,
                 iterations: int = 50) -> dict[str, float]:
        ids, pos = self._index(graph)
        n = len(ids)
        if n == 0:
            return {}
        # column-stochastic sparse transition: follow traversable edges
        src_idx, dst_idx = [], []
        for e in graph.edges:
            if getattr(e, "traversable", True):
                src_idx.append(pos[e.source])
                dst_idx.append(pos[e.target])
                if getattr(e, "bidirectional", False):
                    src_idx.append(pos[e.target])
                    dst_idx.append(pos[e.source])
        src = np.asarray(src_idx, dtype=np.int64)
        dst = np.asarray(dst_idx, dtype=np.int64)
        out_deg = np.bincount(src, minlength=n).astype(np.float64)
        rank = np.full(n, 1.0 / n)
        teleport = (1.0 - damping) / n
        for _ in range(iterations):
            contrib = np.where(out_deg > 0, rank / np.maximum(out_deg, 1), 0.0)
            new = np.full(n, teleport)
            if len(src):
                np.add.at(new, dst, damping * contrib[src])
            # dangling mass redistributed uniformly
            new += damping * rank[out_deg == 0].sum() / n
            if np.abs(new - rank).sum() < 1e-10:
                rank = new
                break
            rank = new
        return {nid: float(rank[i]) for i, nid in enumerate(ids)}

    def betweenness(self, graph, sample: int = 64) -> dict[str, float]:
        """Brandes' algorithm from a deterministic source sample (exact when
        sample >= |V|), unweighted."""
        ids, pos = self._index(graph)
        n = len(ids)
        scores = dict.fromkeys(ids, 0.0)
        if n < 3:
            return scores
        adj: list[list[int]] = [[] for _ in range(n)]
        for e in graph.edges:
            if getattr(e, "traversable", True):
                adj[pos[e.source]].append(pos[e.target])
                if getattr(e, "bidirectional", False):
                    adj[pos[e.target]].append(pos[e.source])
        sources = range(n) if sample >= n else range(0, n, max(1, n // sample))
        for s in sources:
            # single-source shortest-path counts
            dist = [-1] * n
            sigma = [0.0] * n
            preds: list[list[int]] = [[] for _ in range(n)]
            dist[s], sigma[s] = 0, 1.0
            order: list[int] = []
            frontier = [s]
            while frontier:
                nxt = []
                for v in frontier:
                    order.append(v)
                    for w in adj[v]:
                        if dist[w] < 0:
                            dist[w] = dist[v] + 1
                            nxt.append(w)
                        if dist[w] == dist[v] + 1:
                            sigma[w] += sigma[v]
                            preds[w].append(v)
                frontier = nxt
            delta = [0.0] * n
            for w in reversed(order):
                for v in preds[w]:
                    delta[v] += sigma[v] / sigma[w] * (1.0 + delta[w])
                if w != s:
                    scores[ids[w]] += delta[w]
        norm = (n - 1) * (n - 2)
        if norm > 0:
            for k in scores:
                scores[k] /= norm
        return scores

    def components(self, graph, relationships=None) -> dict[str, str]:
        """Node id -> the lexicographically smallest id of its weakly
        connected component, over every edge (undirected) or only those of
        the given ``RelationshipType``s."""
        from agentbom_amd.ops import cpu_ref

        ids, src, dst = component_edges(graph, relationships)
        labels = cpu_ref.connected_components(src, dst, len(ids))
        return {nid: ids[labels[i]] for i, nid in enumerate(ids)}


class NetworkXBackend:
    """Adapter for environments that have networkx installed."""

    name = "networkx"

    def __init__(self) -> None:
        import networkx  # raises ImportError where absent — caller gates

        self._nx = networkx

    def _to_nx(self, graph):
        g = self._nx.DiGraph()
        g.add_nodes_from(graph.nodes)
        for e in graph.edges:
            if getattr(e, "traversable", True):
                g.add_edge(e.source, e.target)
                if getattr(e, "bidirectional", False):
                    g.add_edge(e.target, e.source)
        return g

    def pagerank(self, graph, damping: float = 0.85,
                 iterations: int = 50) -> dict[str, float]:
        return dict(self._nx.pagerank(self._to_nx(graph), alpha=damping,
                                      max_iter=iterations))

    def betweenness(self, graph, sample: int = 64) -> dict[str, float]:
        g = self._to_nx(graph)
        k = min(sample, g.number_of_nodes()) or None
        return dict(self._nx.betweenness_centrality(g, k=k, seed=7))

    def components(self, graph, relationships=None) -> dict[str, str]:
        ids, src, dst = component_edges(graph, relationships)
        g = self._nx.Graph()
        g.add_nodes_from(ids)
        g.add_edges_from((ids[u], ids[v]) for u, v in zip(src.tolist(), dst.tolist()))
        out = {}
        for members in self._nx.connected_components(g):
            out.update(dict.fromkeys(members, min(members)))
        return {nid: out[nid] for nid in ids}


def brandes_sources(n: int, sample: int) -> range:
    """NativeBackend's deterministic source sample: every node when
    ``sample >= n``, else every ``n // sample``-th (which can yield more than
    ``sample`` sources)."""
    return range(n) if sample >= n else range(0, n, max(1, n // sample))


def traversable_edges(graph) -> tuple[list[str], np.ndarray, np.ndarray]:
    """(ids, src, dst) exactly as NativeBackend walks a graph: nodes in
    sorted-id order, traversable edges only, a bidirectional edge in both
    directions, parallel edges kept, edge order as iterated."""
    ids, pos = NativeBackend._index(graph)
    src_idx, dst_idx = [], []
    for e in graph.edges:
        if getattr(e, "traversable", True):
            src_idx.append(pos[e.source])
            dst_idx.append(pos[e.target])
            if getattr(e, "bidirectional", False):
                src_idx.append(pos[e.target])
                dst_idx.append(pos[e.source])
    return (ids, np.asarray(src_idx, dtype=np.int64),
            np.asarray(dst_idx, dtype=np.int64))


def component_edges(graph, relationships=None) -> tuple[list[str], np.ndarray, np.ndarray]:
    """(ids, src, dst) for the component analytics: nodes in sorted-id order
    (so the smallest index of a component is its smallest id), every edge
    once whatever its direction or traversability, restricted to
    ``relationships`` when given; int32 index arrays."""
    ids, pos = NativeBackend._index(graph)
    keep = None if relationships is None else set(relationships)
    src_idx, dst_idx = [], []
    for e in graph.edges:
        if keep is None or e.relationship in keep:
            src_idx.append(pos[e.source])
            dst_idx.append(pos[e.target])
    return (ids, np.asarray(src_idx, dtype=np.int32),
            np.asarray(dst_idx, dtype=np.int32))


def csr_arrays(rows: np.ndarray, cols: np.ndarray, n: int) -> tuple[np.ndarray, np.ndarray]:
    """(row_off int64 [n+1], col int32 [E]) of the edges rows -> cols; the
    edges of one row keep their input order."""
    order = np.argsort(rows, kind="stable")
    row_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_off[1:])
    return row_off, cols[order].astype(np.int32)


class HipBackend:
    """The NativeBackend analytics on the GPU (ops/csrc/centrality.hip,
    ops/csrc/components.hip), with the same index, edge set and result
    contracts (traversable_edges, component_edges)."""

    name = "hip"

    @staticmethod
    def _csr(rows: np.ndarray, cols: np.ndarray, n: int) -> dict:
        import torch

        row_off, col = csr_arrays(rows, cols, n)
        dev = torch.device("cuda")
        return {"row_off": torch.from_numpy(row_off).to(dev),
                "col": torch.from_numpy(col).to(dev)}

    def pagerank(self, graph, damping: float = 0.85,
                 iterations: int = 50) -> dict[str, float]:
        import torch

        from agentbom_amd.ops import native

        ids, src, dst = traversable_edges(graph)
        n = len(ids)
        if n == 0:
            return {}
        rev = self._csr(dst, src, n)
        out_degree = torch.from_numpy(
            np.bincount(src, minlength=n).astype(np.int32)).to(rev["col"].device)
        rank = native.pagerank(rev["row_off"], rev["col"], out_degree, n,
                               damping=damping, iterations=iterations).cpu().numpy()
        return {nid: float(rank[i]) for i, nid in enumerate(ids)}

    def betweenness(self, graph, sample: int = 64) -> dict[str, float]:
        from agentbom_amd.ops import native

        ids, src, dst = traversable_edges(graph)
        n = len(ids)
        if n < 3:
            return dict.fromkeys(ids, 0.0)
        fwd = self._csr(src, dst, n)
        rev = self._csr(dst, src, n)
        bc = native.betweenness(fwd, rev, n, brandes_sources(n, sample)).cpu().numpy()
        bc = bc / ((n - 1) * (n - 2))
        return {nid: float(bc[i]) for i, nid in enumerate(ids)}

    def components(self, graph, relationships=None) -> dict[str, str]:
        import torch

        from agentbom_amd.ops import native

        ids, src, dst = component_edges(graph, relationships)
        if not ids:
            return {}
        dev = torch.device("cuda")
        labels = native.connected_components(
            torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev),
            len(ids)).cpu().numpy()
        return {nid: ids[labels[i]] for i, nid in enumerate(ids)}


def _hip_usable() -> bool:
    try:
        import torch

        from agentbom_amd.ops import native

        return bool(torch.cuda.is_available()) and native.available()
    except Exception:
        return False


def get_backend(name: str | None = None) -> GraphBackendProtocol:
    """Resolve the analytics backend: arg > $AGENT_BOM_GRAPH_BACKEND > native.

    Asking for networkx where it isn't installed, or for hip without a GPU
    and the built engine, falls back to native with the same results
    contract (never an ImportError at call time).
    """
    name = (name or os.environ.get("AGENT_BOM_GRAPH_BACKEND") or "native").lower()
    if name == "networkx":
        try:
            return NetworkXBackend()
        except ImportError:
            return NativeBackend()
    if name == "hip" and _hip_usable():
        return HipBackend()
    return NativeBackend()
