"""The per-source reach kernels (ops/csrc/reach_sets.hip) against the
``cpu_ref.reach_hops`` oracle: hand-built graphs and source counts through
``native.reach_hops``, the graph layer's GPU path against its CPU path, and
``EstateEngine.agent_reach`` on a small estate against the CPU engine.  Every
comparison is exact integer equality.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from reach_sets_graphs import (
    DEPTHS, ESTATE_ARGS, GRAPHS, NO, SOURCE_COUNTS, STAGE_STAR_LEAVES, edited_demo_graph,
    estate_agents, random_graph, random_sources, stage_star, star,
)

from agentbom_amd.graph.builder import build_unified_graph_from_report
from agentbom_amd.graph.container import UnifiedEdge, UnifiedGraph, UnifiedNode
from agentbom_amd.graph.dependency_reach import compute_dependency_reach
from agentbom_amd.graph.gpu_engine import EstateEngine
from agentbom_amd.graph.types import EntityType, RelationshipType
from agentbom_amd.ops import cpu_ref, native
from agentbom_amd.scan.orchestrator import run_demo_scan
from agentbom_amd.scan.synth import generate_estate

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to("cuda")


def _run(csr, sources, targets, n, mask, depth, ws=None):
    row_off, col, etype = csr
    return native.reach_hops(
        _dev(row_off), _dev(col), _dev(np.asarray(sources, dtype=np.int32)),
        _dev(np.asarray(targets, dtype=np.int32)), n, etype=_dev(etype), allowed_mask=mask,
        max_depth=depth, workspace=ws)


def _check(got, want):
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    print("mismatches:", int((got != want).sum()), "of", want.size)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("make", GRAPHS, ids=lambda f: f.__name__)
def test_kernel_equals_oracle_on_hand_built_graphs(make, depth):
    g = make()
    csr = g.csr()
    ws: dict = {}
    got = _run(csr, g.sources, g.targets, g.num_nodes, g.mask, depth, ws)
    want = cpu_ref.reach_hops(*csr[:2], g.sources, g.targets, g.num_nodes, etype=csr[2],
                              allowed_mask=g.mask, max_depth=depth)
    assert np.array_equal(want, g.expected(depth))
    _check(got, want)
    assert isinstance(ws["levels"], int) and isinstance(ws["passes"], int)
    assert ws["passes"] == 1 and 0 <= ws["levels"] <= depth


@pytest.mark.parametrize("leaves", STAGE_STAR_LEAVES)
def test_one_block_stages_a_row_around_its_queue_capacity(leaves):
    g = stage_star(leaves)
    csr = g.csr()
    want = cpu_ref.reach_hops(*csr[:2], g.sources, g.targets, g.num_nodes, etype=csr[2],
                              allowed_mask=g.mask, max_depth=1)
    assert np.array_equal(want, g.expected(1)) and (want == 1).all()
    _check(_run(csr, g.sources, g.targets, g.num_nodes, g.mask, 1), want)


@pytest.fixture(scope="module")
def rand():
    n, row_off, col, etype, mask = random_graph()
    return n, (row_off, col, etype), mask, np.arange(n, dtype=np.int32)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("count", SOURCE_COUNTS)
def test_kernel_equals_oracle_at_every_source_count(rand, count, depth):
    n, csr, mask, targets = rand
    sources = random_sources(count, n)
    ws: dict = {}
    got = _run(csr, sources, targets, n, mask, depth, ws)
    _check(got, cpu_ref.reach_hops(*csr[:2], sources, targets, n, etype=csr[2],
                                   allowed_mask=mask, max_depth=depth))
    per_pass = native.REACH_WORD_SOURCES * native.REACH_MAX_WORDS
    assert ws["passes"] == (count + per_pass - 1) // per_pass


def test_workspace_is_clean_for_the_next_call(rand):
    n, csr, mask, targets = rand
    ws: dict = {}
    # depth 3 stops with a live frontier, depth 16 runs it dry; then fewer words
    for count, depth in ((130, 3), (257, 16), (65, 1), (1, 16)):
        sources = random_sources(count, n, seed=count + depth)
        _check(_run(csr, sources, targets, n, mask, depth, ws),
               cpu_ref.reach_hops(*csr[:2], sources, targets, n, etype=csr[2],
                                  allowed_mask=mask, max_depth=depth))
    g = star()
    _check(_run(g.csr(), g.sources, g.targets, g.num_nodes, g.mask, 16, ws), g.expected(16))
    for key in ("reach_cur", "reach_nxt"):
        assert int(ws[key].count_nonzero()) == 0, key


def test_chunks_are_the_columns_of_the_whole(rand):
    n, csr, mask, targets = rand
    sources = random_sources(130, n)
    want = cpu_ref.reach_hops(*csr[:2], sources, targets, n, etype=csr[2], allowed_mask=mask,
                              max_depth=16)
    args = (_dev(csr[0]), _dev(csr[1]), _dev(sources), _dev(targets), n)
    pieces = list(native.reach_hops_chunks(*args, etype=_dev(csr[2]), allowed_mask=mask,
                                           max_depth=16, chunk_sources=50))
    assert [first for first, _ in pieces] == [0, 50, 100]
    assert [h.shape[1] for _, h in pieces] == [50, 50, 30]
    _check(torch.cat([h for _, h in pieces], dim=1), want)


def test_empty_sources_or_targets_launch_nothing(rand):
    n, csr, mask, targets = rand
    none = np.zeros(0, dtype=np.int32)
    ws: dict = {}
    got = _run(csr, none, targets, n, mask, 16, ws)
    assert tuple(got.shape) == (n, 0) and got.dtype == torch.uint8
    got = _run(csr, targets, none, n, mask, 16, ws)
    assert tuple(got.shape) == (0, n) and got.dtype == torch.uint8
    # nothing was launched: no state buffer was ever allocated
    assert ws == {"levels": 0, "passes": 0}


def test_arguments_are_checked(rand):
    n, csr, mask, targets = rand
    row_off, col = _dev(csr[0]), _dev(csr[1])
    with pytest.raises(TypeError):
        native.reach_hops(row_off, col, _dev(targets, torch.int64), _dev(targets), n)
    with pytest.raises(ValueError):
        native.reach_hops(row_off, col, torch.from_numpy(targets), _dev(targets), n)


# ── graph layer: compute_dependency_reach(use_gpu=True) ────────────────────


@pytest.fixture(scope="module")
def demo_graph():
    return build_unified_graph_from_report(run_demo_scan())


def _assert_same_reach(graph):
    want = compute_dependency_reach(graph, use_gpu=False)
    got = compute_dependency_reach(graph, use_gpu=True)
    assert want.package_reach, "the CPU path reached nothing: the test shows nothing"
    assert got.package_reach == want.package_reach
    assert got.vuln_reach == want.vuln_reach
    return want


def test_graph_gpu_path_equals_cpu_path_on_the_demo_graph(demo_graph):
    want = _assert_same_reach(demo_graph)
    assert want.vuln_reach


def test_graph_gpu_path_skips_a_non_traversable_edge(demo_graph):
    edited = edited_demo_graph(demo_graph)
    want = _assert_same_reach(edited)
    # the blocked edge matters: with it the agent reached more
    assert want.package_reach != compute_dependency_reach(demo_graph, use_gpu=False).package_reach


def _chain_graph(hops: int = 20) -> UnifiedGraph:
    """agent -USES-> server -DEPENDS_ON-> p1 -> ... : ``hops`` edges in all."""
    g = UnifiedGraph()
    g.add_node(UnifiedNode(id="agent:a", entity_type=EntityType.AGENT, label="a"))
    g.add_node(UnifiedNode(id="server:s", entity_type=EntityType.SERVER, label="s"))
    g.add_edge(UnifiedEdge("agent:a", "server:s", RelationshipType.USES))
    prev = "server:s"
    for i in range(2, hops + 1):
        nid = f"pkg:p{i:02d}"
        g.add_node(UnifiedNode(id=nid, entity_type=EntityType.PACKAGE, label=nid))
        g.add_edge(UnifiedEdge(prev, nid, RelationshipType.DEPENDS_ON))
        prev = nid
    g.add_node(UnifiedNode(id="vuln:v", entity_type=EntityType.VULNERABILITY, label="v"))
    g.add_edge(UnifiedEdge("vuln:v", "pkg:p16", RelationshipType.AFFECTS))
    g.add_edge(UnifiedEdge("vuln:v", "pkg:p17", RelationshipType.AFFECTS))
    return g


def test_graph_gpu_path_stops_at_depth_16():
    g = _chain_graph()
    want = _assert_same_reach(g)
    assert want.package_reach["pkg:p16"] == {"agent:a": 16}
    assert "pkg:p17" not in want.package_reach
    assert want.vuln_reach["vuln:v"] == {"reachable_from": ["agent:a"], "min_hops": 16}


def test_graph_gpu_path_runs_no_host_bfs(demo_graph, monkeypatch):
    want = compute_dependency_reach(demo_graph, use_gpu=False)

    def no_bfs(self, *args, **kwargs):
        raise AssertionError("graph.bfs called on the GPU path")

    monkeypatch.setattr(UnifiedGraph, "bfs", no_bfs)
    got = compute_dependency_reach(demo_graph, use_gpu=True)
    assert got.package_reach == want.package_reach
    assert not any("*" in agents for agents in got.package_reach.values())


# ── estate engine: agent_reach ─────────────────────────────────────────────


@pytest.fixture(scope="module")
def engines():
    est = generate_estate(**ESTATE_ARGS)
    return EstateEngine(est, device="cuda"), EstateEngine(est, device="cpu")


def _assert_same_result(got, want):
    for key in ("hops", "agents", "targets", "n_reaching", "min_hop"):
        assert got[key].is_cuda and got[key].dtype == want[key].dtype, key
        print(key, "mismatches:", int((got[key].cpu() != want[key]).sum()))
        assert torch.equal(got[key].cpu(), want[key]), key


def test_engine_agent_reach_equals_cpu_engine_on_all_packages(engines):
    gpu, cpu = engines
    agents = estate_agents(gpu.estate)
    want = cpu.agent_reach(agents)
    assert set(torch.unique(want["hops"]).tolist()) == {2, NO}
    _assert_same_result(gpu.agent_reach(agents), want)
    _assert_same_result(gpu.agent_reach(agents, max_depth=1), cpu.agent_reach(agents, max_depth=1))


def test_engine_agent_reach_on_matched_packages_counts_the_blast_agents(engines):
    gpu, cpu = engines
    est = gpu.estate
    res = gpu.step()
    pkg_idx = res["pkg_idx"].cpu().numpy()
    uniq, first = np.unique(pkg_idx, return_index=True)
    assert len(uniq) > 0
    targets = torch.from_numpy(uniq + est.pkg_base)
    n_agents = res["n_agents"].cpu().numpy()[first]
    agents = estate_agents(est)
    got = gpu.agent_reach(agents, targets=targets)
    _assert_same_result(got, cpu.agent_reach(agents, targets=targets))
    assert (got["n_reaching"].cpu().numpy() <= n_agents).all()
    # every agent a source: a package sits exactly two hops below each agent
    # that uses one of its servers, which is what the blast count counts
    everyone = np.arange(est.n_agents, dtype=np.int32) + est.agent_base
    full = gpu.agent_reach(everyone, targets=targets)
    assert np.array_equal(full["n_reaching"].cpu().numpy(), n_agents)
    assert set(full["min_hop"].cpu().tolist()) <= {2, NO}
