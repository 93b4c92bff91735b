"""Dependency-reach: which agents can structurally reach which packages.

Reference: src/agent_bom/graph/dependency_reach.py:109 compute_dependency_reach
(two passes: (1) BFS from every agent along USES/DEPENDS_ON/CONTAINS/
PROVIDES_TOOL recording min-hop per package; (2) join vulns to packages via
AFFECTS/VULNERABLE_TO -> per-vuln reachable_from + min hop) and
graph/blast_reach.py:48 apply_dependency_reachability_to_blast_radii.

The CPU path (``use_gpu=False``) is the reference implementation: one
``graph.bfs`` per agent.  The GPU path (``use_gpu=True``, or chosen
automatically for graphs of 5000 nodes and more when a GPU is present) lays
the graph out as the CSR that ``graph.bfs`` walks (:func:`reach_csr`) and runs
every agent in one bit-parallel multi-source BFS (``native.reach_hops``,
ops/csrc/reach_sets.hip), which returns the hop count per (package, agent);
there is no host BFS on that path.  Pass 2 is the same host join on both.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

from agentbom_amd.graph.container import UnifiedGraph
from agentbom_amd.graph.types import EntityType, RelationshipType

_REACH_RELS = {
    RelationshipType.USES,
    RelationshipType.DEPENDS_ON,
    RelationshipType.CONTAINS,
    RelationshipType.PROVIDES_TOOL,
}


@dataclass
class DependencyReach:
    # package node id -> {agent node id: min hops}
    package_reach: dict[str, dict[str, int]] = field(default_factory=dict)
    # vuln node id -> {"reachable_from": [agent ids], "min_hops": int}
    vuln_reach: dict[str, dict] = field(default_factory=dict)


def compute_dependency_reach(graph: UnifiedGraph,
                             use_gpu: Optional[bool] = None) -> DependencyReach:
    agents = [nid for nid, n in graph.nodes.items() if n.entity_type == EntityType.AGENT]
    reach = DependencyReach()

    if use_gpu is None:
        try:
            import torch

            use_gpu = torch.cuda.is_available() and graph.node_count >= 5000
        except Exception:
            use_gpu = False

    if use_gpu:
        _reach_gpu(graph, agents, reach)
    else:
        for a in agents:
            dist = graph.bfs(a, max_depth=16, allowed=_REACH_RELS)
            for nid, hops in dist.items():
                if graph.nodes[nid].entity_type == EntityType.PACKAGE:
                    cur = reach.package_reach.setdefault(nid, {})
                    if a not in cur or hops < cur[a]:
                        cur[a] = hops

    # pass 2: join vulns to packages
    for e in graph.edges:
        if e.relationship != RelationshipType.AFFECTS:
            continue
        v_id, p_id = e.source, e.target
        pr = reach.package_reach.get(p_id)
        if not pr:
            continue
        entry = reach.vuln_reach.setdefault(v_id, {"reachable_from": [], "min_hops": None})
        for a, hops in pr.items():
            if a not in entry["reachable_from"]:
                entry["reachable_from"].append(a)
            if entry["min_hops"] is None or hops < entry["min_hops"]:
                entry["min_hops"] = hops
        entry["reachable_from"].sort()
    return reach


def reach_csr(graph: UnifiedGraph, allowed: Optional[set] = None):
    """``(order, row_off, col, etype)``: the graph as ``graph.bfs(start,
    allowed=allowed)`` walks it.  Unlike ``to_csr()`` it leaves out the edges
    that walk skips (non-traversable ones, and relationships outside
    ``allowed`` when that is given); like it, a bidirectional edge appears in
    both directions, nodes are in sorted-id order and ``etype`` holds
    ``types.REL_CODE`` (capped at 255).  ``row_off`` is int64 [N+1], ``col``
    int32, ``etype`` uint8."""
    import numpy as np

    from agentbom_amd.graph.types import REL_CODE

    order = sorted(graph.nodes)
    index = {nid: i for i, nid in enumerate(order)}
    src, dst, et = [], [], []
    for e in graph.edges:
        if not e.traversable or (allowed is not None and e.relationship not in allowed):
            continue
        code = min(REL_CODE[e.relationship], 255)
        s, t = index[e.source], index[e.target]
        src.append(s), dst.append(t), et.append(code)
        if e.bidirectional:
            src.append(t), dst.append(s), et.append(code)
    n = len(order)
    src_a = np.asarray(src, dtype=np.int64)
    o = np.argsort(src_a, kind="stable")
    row_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src_a, minlength=n), out=row_off[1:])
    return (order, row_off, np.asarray(dst, dtype=np.int32)[o],
            np.asarray(et, dtype=np.uint8)[o])


# Bytes of the (package, agent) hop matrix held at once on the GPU path
_REACH_CHUNK_BYTES = 1 << 28


def _reach_gpu(graph: UnifiedGraph, agents: list[str], reach: "DependencyReach") -> None:
    """Hops per (package, agent) from one bit-parallel BFS over the device
    CSR: sources are the agents, targets the PACKAGE nodes, depth 16 as on the
    CPU path.  The matrix comes back in column pieces of bounded size."""
    import numpy as np
    import torch

    from agentbom_amd.graph.types import DEPENDENCY_REACH_MASK
    from agentbom_amd.ops import native

    order, row_off, col, etype = reach_csr(graph, _REACH_RELS)
    index = {nid: i for i, nid in enumerate(order)}
    pkgs = [i for i, nid in enumerate(order)
            if graph.nodes[nid].entity_type == EntityType.PACKAGE]
    if not agents or not pkgs:
        return
    dev = torch.device("cuda")
    sources = torch.tensor([index[a] for a in agents], dtype=torch.int32, device=dev)
    targets = torch.tensor(pkgs, dtype=torch.int32, device=dev)
    chunk = max(64, _REACH_CHUNK_BYTES // len(pkgs) // 64 * 64)
    for first, hops in native.reach_hops_chunks(
            torch.from_numpy(row_off).to(dev), torch.from_numpy(col).to(dev), sources, targets,
            len(order), etype=torch.from_numpy(etype).to(dev),
            allowed_mask=DEPENDENCY_REACH_MASK, max_depth=16, chunk_sources=chunk):
        h = hops.cpu().numpy()
        t_idx, s_idx = np.nonzero(h != native.REACH_UNREACHED)
        for t, s, d in zip(t_idx.tolist(), s_idx.tolist(), h[t_idx, s_idx].tolist()):
            reach.package_reach.setdefault(order[pkgs[t]], {})[agents[first + s]] = d


def apply_dependency_reachability_to_blast_radii(report, graph: UnifiedGraph,
                                                 reach: Optional[DependencyReach] = None) -> int:
    """Stamp dependency_* fields on every BlastRadius and rescore.

    Reference: graph/blast_reach.py:48 — structural closure proves topology,
    not exploitability; scores only shift via the reachability nudge."""
    from agentbom_amd.utils.canonical_ids import canonical_package_key

    if reach is None:
        reach = compute_dependency_reach(graph)
    updated = 0
    for br in report.blast_radii:
        p_id = "pkg:" + canonical_package_key(
            br.package.name, br.package.version, br.package.ecosystem, br.package.purl
        )
        pr = reach.package_reach.get(p_id)
        if pr:
            br.dependency_reachable = True
            br.dependency_min_hop_distance = min(pr.values())
            br.dependency_reachable_from_agents = sorted(
                a.removeprefix("agent:") for a in pr
            )
        else:
            br.dependency_reachable = False
            br.dependency_min_hop_distance = None
            br.dependency_reachable_from_agents = []
        br.calculate_risk_score()
        updated += 1
    report.blast_radii.sort(key=lambda b: -b.risk_score)
    return updated
