"""paths.hip with edge weights: bit-exact parity with cpu_ref.path_relax.

The path DP is the one kernel whose float result must equal the host
arithmetic bit for bit: reconstruction (graph/path_engine.py) accepts a
predecessor only when float32(pred_score + step) == stored_score, so a label
that is one ulp off silently drops its path.  The weight term
``edge_weight * 0.3f`` is where a fused multiply-add would round once where
the host rounds twice; a weight of exactly 1.0 hides that, so every graph
here carries other weights.  Inputs live in tests/path_relax_cases.py.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from path_relax_cases import (
    NO_EDGE,
    hand_cases,
    layered_dag,
    random_graph,
    tables,
)

pytestmark = pytest.mark.gpu

GRID_CAP_EDGES = 2048 * 256  # grid_for() caps the grid at 2048 blocks of 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _relax_gpu(dev, g, cur, use_node_gate=True, hops=1):
    """Chained native.path_relax hops; returns the u64 label level per hop."""
    from agentbom_amd.ops import native

    eb, tv, eg = tables()

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    src_t, dst_t, et_t, w_t = t(g["src"]), t(g["dst"]), t(g["et"]), t(g["w"])
    nb_t, eb_t, tv_t, eg_t = t(g["nb"]), t(eb), t(tv), t(eg)
    ng = g["ng"] if use_node_gate else None
    ng_t = t(ng) if ng is not None else None
    cur_t = t(cur.view(np.int64))
    levels = []
    for _ in range(hops):
        nxt_t = torch.zeros_like(cur_t)
        native.path_relax(src_t, dst_t, et_t, w_t, cur_t, nxt_t, nb_t, eb_t,
                          tv_t, eg_t, ng_t)
        levels.append(nxt_t.cpu().numpy().view(np.uint64))
        cur_t = nxt_t
    return levels


def _relax_ref(g, cur, use_node_gate=True, hops=1):
    from agentbom_amd.ops import cpu_ref

    eb, tv, eg = tables()
    ng = g["ng"] if use_node_gate else None
    levels = []
    for _ in range(hops):
        cur = cpu_ref.path_relax(g["src"], g["dst"], g["et"], g["w"], cur,
                                 g["nb"], eb, tv, eg, ng)
        levels.append(cur)
    return levels


def _hop1_labels(g, use_node_gate, fused):
    """Hop-1 labels from the seed level, computed directly (every seed has
    score 0 and no predecessor), with the weight term rounded twice as the
    host does it (fused=False) or once as an FMA does (fused=True)."""
    from agentbom_amd.ops import cpu_ref

    eb, tv, eg = tables()
    seeded = np.zeros(g["n"], dtype=bool)
    seeded[g["entries"]] = True
    e_idx = np.nonzero(tv[g["et"]].astype(bool) & seeded[g["src"]])[0]
    v = g["dst"][e_idx].astype(np.int64)
    step = eb[g["et"][e_idx]] + g["nb"][v]
    w = g["w"][e_idx]
    if fused:
        scaled64 = w.astype(np.float64) * np.float64(np.float32(0.3))
        step = (step.astype(np.float64) + scaled64).astype(np.float32)
    else:
        step = step + w * np.float32(0.3)
    assert step.dtype == np.float32
    gate = eg[g["et"][e_idx]].astype(bool)
    if use_node_gate:
        gate = gate | g["ng"][v].astype(bool)
    out = np.zeros(g["n"] * 2, dtype=np.uint64)
    np.maximum.at(out, v * 2 + gate, cpu_ref.path_pack(step, e_idx))
    return out


@pytest.fixture(scope="module")
def weighted_graph():
    return random_graph(3000, 40000, 64, seed=20240611)


@pytest.mark.parametrize("use_node_gate", [True, False],
                         ids=["node_gate", "no_node_gate"])
def test_weighted_parity(weighted_graph, dev, use_node_gate):
    """Four weighted hops on a random graph, bit for bit; node_gate=None with
    weights is the combination graph/attack_paths.py runs."""
    g = weighted_graph
    w = g["w"]
    assert (w >= 0).all() and (w == 1.0).sum() > len(w) // 5 and (w == 0.0).any()
    ref = _relax_ref(g, g["cur"], use_node_gate, hops=4)
    # the inputs must be able to tell one rounding from two
    two = _hop1_labels(g, use_node_gate, fused=False)
    one = _hop1_labels(g, use_node_gate, fused=True)
    assert np.array_equal(two, ref[0])
    n_tell = int((one != two).sum())
    print(f"hop-1 labels that a fused weight term would change: {n_tell}")
    assert n_tell >= 1

    got = _relax_gpu(dev, g, g["cur"], use_node_gate, hops=4)
    for d in range(4):
        diff = int((got[d] != ref[d]).sum())
        print(f"hop {d + 1}: {diff} of {int((ref[d] != 0).sum())} labels differ")
    for d in range(4):
        assert np.array_equal(got[d], ref[d]), f"hop {d + 1} labels diverge"


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_built(dev, name):
    """One-hop semantics with weights present: expected labels written by
    hand, checked against the oracle and the kernel."""
    c = hand_cases()[name]
    ref = _relax_ref(c, c["cur"])[0]
    assert np.array_equal(ref, c["expect"])
    got = _relax_gpu(dev, c, c["cur"])[0]
    assert np.array_equal(got, c["expect"])
    if name == "tie_larger_edge_wins":
        assert int(got[2 * 2 + 0]) & NO_EDGE == 1


@pytest.mark.parametrize("num_edges", [1, 255, 256, 257])
def test_launch_shape_small(dev, num_edges):
    """Edge counts around one block of 256 threads.  The last edge is
    traversable, leaves a seeded node and carries a weight that makes it win
    its slot, so a kernel that dropped it (or never ran) cannot pass; that
    weight is also one at which a fused weight term rounds differently."""
    g = random_graph(48, num_edges, 48, seed=1000 + num_edges)
    eb, _tv, _eg = tables()
    last = num_edges - 1
    g["et"][last] = 1
    base = eb[1] + g["nb"][g["dst"][last]]
    # >= 20 adds >= 6 to the step; every other step is below 1.5 + 2 + 0.6
    rng = np.random.default_rng(num_edges)
    heavy = (20.0 + 20.0 * rng.random(256)).astype(np.float32)
    two = base + heavy * np.float32(0.3)
    one = (np.float64(base)
           + heavy.astype(np.float64) * np.float64(np.float32(0.3))).astype(np.float32)
    assert (two != one).any()
    g["w"][last] = heavy[np.nonzero(two != one)[0][0]]
    ref = _relax_ref(g, g["cur"], hops=2)
    assert ref[0].any()
    if num_edges > 1:  # one edge cannot carry a label two hops
        assert ref[1].any()
    winners = (ref[0][ref[0] != 0] & np.uint64(NO_EDGE)).astype(np.int64)
    assert last in winners  # the thread at the end of the range must count
    got = _relax_gpu(dev, g, g["cur"], hops=2)
    for d in range(2):
        assert np.array_equal(got[d], ref[d]), f"hop {d + 1} labels diverge"


def test_launch_shape_grid_stride(dev):
    """E = 2048*256 + 300: the smallest edge count that enters the
    grid-stride loop.  The 300 edges past the capped grid leave entry nodes
    with a weight large enough that they must win their slots."""
    num_edges = GRID_CAP_EDGES + 300
    g = random_graph(4096, num_edges, 64, seed=77)
    rng = np.random.default_rng(78)
    g["src"][-300:] = rng.choice(g["entries"], size=300).astype(np.int32)
    g["et"][-300:] = rng.integers(0, 4, size=300).astype(np.uint8)
    g["w"][-300:] = (40.0 + rng.random(300)).astype(np.float32)
    ref = _relax_ref(g, g["cur"], hops=2)
    winners = (ref[0][ref[0] != 0] & np.uint64(NO_EDGE)).astype(np.int64)
    assert (winners >= GRID_CAP_EDGES).sum() >= 100  # tail edges do win
    got = _relax_gpu(dev, g, g["cur"], hops=2)
    for d in range(2):
        assert np.array_equal(got[d], ref[d]), f"hop {d + 1} labels diverge"


@pytest.fixture(scope="module")
def dag():
    return layered_dag(8, 250, 20000, seed=4242)


@pytest.mark.parametrize("use_node_gate", [False, True],
                         ids=["no_node_gate", "node_gate"])
def test_run_path_dp_weighted_gpu_matches_cpu(dag, dev, use_node_gate):
    """DP plus reconstruction with weights: the device run must return the
    paths the host run returns — a label one ulp off loses its path.  k is
    above the number of targets, so every hit is compared."""
    from agentbom_amd.graph.path_engine import run_path_dp

    eb, tv, eg = tables()
    ng = dag["ng"] if use_node_gate else None

    def run(device):
        return run_path_dp(dag["src"], dag["dst"], dag["et"], dag["w"],
                           dag["n"], dag["entries"], dag["nb"], eb, tv, eg,
                           ng, dag["tm"], max_depth=6, k=1000, device=device)

    hits_c = run(None)
    assert len(hits_c) == int(dag["tm"].sum()) == 750  # every target, not a top-k cut
    hits_g = run(dev)
    print(f"hits: host {len(hits_c)}, device {len(hits_g)}")
    assert len(hits_g) == len(hits_c)
    for a, b in zip(hits_g, hits_c):
        assert a.nodes == b.nodes
        assert a.etypes == b.etypes
        assert a.score == b.score


def _weighted_unified_graph():
    """~50 nodes: agents -> servers -> packages/creds/tools, lateral server
    links, vulnerabilities; every edge weight differs from the 1.0 default."""
    from agentbom_amd.graph.container import UnifiedEdge, UnifiedGraph, UnifiedNode
    from agentbom_amd.graph.types import EntityType as E
    from agentbom_amd.graph.types import NodeStatus
    from agentbom_amd.graph.types import RelationshipType as R

    rng = np.random.default_rng(42)
    g = UnifiedGraph()

    def add(kind, prefix, count, **props):
        ids = [f"{prefix}{i:02d}" for i in range(count)]
        for i, nid in enumerate(ids):
            sev = props.get("severity")
            g.add_node(UnifiedNode(
                id=nid, entity_type=kind, label=nid,
                status=NodeStatus.VULNERABLE if props.get("vuln") and i % 2 else NodeStatus.ACTIVE,
                properties={"severity": sev[i % len(sev)]} if sev else {}))
        return ids

    agents = add(E.AGENT, "agent", 4)
    servers = add(E.SERVER, "server", 10, vuln=True)
    pkgs = add(E.PACKAGE, "pkg", 16, vuln=True)
    vulns = add(E.VULNERABILITY, "vuln", 8, severity=["critical", "high", "medium"])
    creds = add(E.CREDENTIAL, "cred", 6)
    tools = add(E.TOOL, "tool", 6)

    def link(a, b, rel, bidirectional=False):
        weight = round(float(rng.uniform(0.05, 1.95)), 2)
        if weight == 1.0:
            weight = 0.7
        g.add_edge(UnifiedEdge(a, b, rel, weight=weight, bidirectional=bidirectional))

    for a in agents:
        for s in rng.choice(servers, size=4, replace=False):
            link(a, str(s), R.USES)
    for i, s in enumerate(servers):
        for p in rng.choice(pkgs, size=3, replace=False):
            link(s, str(p), R.DEPENDS_ON)
        link(s, creds[i % len(creds)], R.EXPOSES_CRED)
        link(s, tools[i % len(tools)], R.PROVIDES_TOOL)
        link(s, servers[(i + 3) % len(servers)], R.SHARES_SERVER, bidirectional=True)
    for i, p in enumerate(pkgs):
        link(p, vulns[i % len(vulns)], R.VULNERABLE_TO)
    for i, v in enumerate(vulns):
        link(v, tools[i % len(tools)], R.EXPLOITABLE_VIA)
    return g


def _hops_that_tell_roundings_apart(graph, paths) -> int:
    """Hops on the host's paths whose step rounds differently when the
    weight term is fused — a condition on the graph, checked on the CPU."""
    from agentbom_amd.graph.attack_paths import _EDGE_BOOST, _node_boost
    from agentbom_amd.graph.types import RelationshipType

    weight = {}
    for e in graph.edges:
        weight[(e.source, e.target, e.relationship.value)] = e.weight
        if e.bidirectional:
            weight[(e.target, e.source, e.relationship.value)] = e.weight
    count = 0
    for p in paths:
        for u, v, rel in zip(p.nodes, p.nodes[1:], p.relationships):
            base = (np.float32(_EDGE_BOOST.get(RelationshipType(rel), 0.3))
                    + np.float32(_node_boost(graph, v)))
            w = np.float32(weight[(u, v, rel)])
            two = base + w * np.float32(0.3)
            one = np.float32(np.float64(base)
                             + np.float64(w) * np.float64(np.float32(0.3)))
            count += int(two != one)
    return count


def test_graph_route_weighted_gpu_matches_cpu(dev):
    """compute_attack_paths_dp passes a per-edge weight array and
    node_gate=None; call it directly so the node-count threshold is moot."""
    from agentbom_amd.graph.attack_paths import compute_attack_paths_dp

    graph = _weighted_unified_graph()
    assert 40 <= len(graph.nodes) <= 60
    assert all(e.weight != 1.0 for e in graph.edges)
    host = compute_attack_paths_dp(graph, max_paths=50, device=None)
    assert len(host) >= 10
    assert any(len(p.nodes) >= 4 for p in host)
    assert _hops_that_tell_roundings_apart(graph, host) >= 1
    got = compute_attack_paths_dp(graph, max_paths=50, device=dev)
    assert [p.id for p in got] == [p.id for p in host]
    assert [p.score for p in got] == [p.score for p in host]
    assert [p.nodes for p in got] == [p.nodes for p in host]
