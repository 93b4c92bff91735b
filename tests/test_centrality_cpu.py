"""Centrality oracles and plumbing that need no GPU.

``cpu_ref.pagerank`` / ``cpu_ref.betweenness`` are the oracle of the HIP
kernels (tests/test_centrality_gpu.py); here they are held against
``NativeBackend``, the behaviour the hip backend has to reproduce.

Tolerance (derived, not measured): every term of both algorithms is
non-negative, so nothing cancels; an fp64 sum of m non-negative terms is off
by at most (m-1) * 2^-53 relative, compounding over at most `depth` levels or
`iterations` passes.  These graphs have m <= 200 and depth * m < 1e4, far
below the 1e-9 the comparison allows.  Values that are exactly 0.0 on one
side (chain endpoints, sources, unreached nodes) must be exactly 0.0 on the
other.  Both PageRank loops stop on the same rule (first pass with an L1
change below 1e-10); should rounding make them stop one pass apart, both
changes are below 1e-10 by construction, which ``atol`` absorbs.
"""

from __future__ import annotations

import random
import re
from pathlib import Path

import numpy as np
import pytest

from agentbom_amd.graph.backend import (
    NativeBackend,
    brandes_sources,
    csr_arrays,
    get_backend,
    traversable_edges,
)
from agentbom_amd.graph.container import UnifiedEdge, UnifiedGraph, UnifiedNode
from agentbom_amd.graph.types import EntityType, RelationshipType
from agentbom_amd.ops import cpu_ref, native

RTOL, ATOL = 1e-9, 1e-12


def _graph(n: int, edges, bidirectional=(), blocked=()) -> UnifiedGraph:
    """n nodes v000.. and the (u, v) edges in order; edge indices listed in
    ``bidirectional`` / ``blocked`` get that flag."""
    g = UnifiedGraph()
    for i in range(n):
        g.add_node(UnifiedNode(id=f"v{i:03d}", entity_type=EntityType.PACKAGE,
                               label=f"v{i:03d}"))
    for k, (u, v) in enumerate(edges):
        e = UnifiedEdge(f"v{u:03d}", f"v{v:03d}", RelationshipType.DEPENDS_ON)
        e.bidirectional = k in bidirectional
        e.traversable = k not in blocked
        g.add_edge(e)
    return g


def _random_digraph():
    rng = random.Random(7)
    edges = [(rng.randrange(60), rng.randrange(60)) for _ in range(196)]
    edges += [edges[0], edges[0], edges[5], (9, 9)]  # parallel edges, a self-loop
    return _graph(60, edges)


CASES = {
    "star_in": lambda: _graph(6, [(i, 0) for i in range(1, 6)]),
    "star_out": lambda: _graph(6, [(0, i) for i in range(1, 6)]),
    "chain7": lambda: _graph(7, [(i, i + 1) for i in range(6)]),
    "diamond": lambda: _graph(5, [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)]),
    "random60": _random_digraph,
    # 3 and 4 dangle, 5 is isolated
    "dangling_isolated": lambda: _graph(6, [(0, 1), (1, 2), (2, 0), (2, 3), (1, 4)]),
    "bidirectional": lambda: _graph(5, [(0, 1), (1, 2), (2, 3), (3, 4)], bidirectional={1}),
    "non_traversable": lambda: _graph(5, [(0, 1), (1, 2), (2, 3), (0, 3), (3, 4)], blocked={3}),
}


def _assert_close(got: np.ndarray, want: np.ndarray) -> None:
    zero = want == 0.0
    assert np.array_equal(got[zero], want[zero]), "exact zeros differ"
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("case", sorted(CASES))
def test_cpu_ref_pagerank_matches_native_backend(case):
    g = CASES[case]()
    want = NativeBackend().pagerank(g)
    ids, src, dst = traversable_edges(g)
    n = len(ids)
    rev_off, rev_col = csr_arrays(dst, src, n)
    got = cpu_ref.pagerank(rev_off, rev_col, np.bincount(src, minlength=n), n)
    assert list(want) == ids
    _assert_close(got, np.array([want[i] for i in ids]))
    assert abs(got.sum() - 1.0) < 1e-9


@pytest.mark.parametrize("sample", [3, 100])
@pytest.mark.parametrize("case", sorted(CASES))
def test_cpu_ref_betweenness_matches_native_backend(case, sample):
    g = CASES[case]()
    want = NativeBackend().betweenness(g, sample=sample)
    ids, src, dst = traversable_edges(g)
    n = len(ids)
    fwd_off, fwd_col = csr_arrays(src, dst, n)
    got = cpu_ref.betweenness(fwd_off, fwd_col, n, brandes_sources(n, sample))
    _assert_close(got / ((n - 1) * (n - 2)), np.array([want[i] for i in ids]))


def test_cpu_ref_betweenness_edge_type_mask():
    """Masking an edge type out equals deleting those edges."""
    edges = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 4)]
    etype = np.array([0, 0, 0, 1, 0], dtype=np.uint8)
    src, dst = (np.array(c, dtype=np.int64) for c in zip(*edges))
    off, col = csr_arrays(src, dst, 5)
    et = etype[np.argsort(src, kind="stable")]
    masked = cpu_ref.betweenness(off, col, 5, range(5), etype=et, allowed_mask=0b01)
    keep = etype == 0
    off2, col2 = csr_arrays(src[keep], dst[keep], 5)
    assert np.array_equal(masked, cpu_ref.betweenness(off2, col2, 5, range(5)))
    assert not np.array_equal(masked, cpu_ref.betweenness(off, col, 5, range(5)))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_betweenness_tiny_graphs_are_zero(n):
    g = _graph(n, [(0, 1)] if n == 2 else [])
    assert set(NativeBackend().betweenness(g).values()) <= {0.0}
    off, col = csr_arrays(*traversable_edges(g)[1:], n)
    assert not cpu_ref.betweenness(off, col, n, range(n)).any()
    assert cpu_ref.pagerank(off, col, np.zeros(n, dtype=np.int64), n).shape == (n,)


@pytest.mark.parametrize("sample", [3, 64, 100])
def test_source_sampling_matches_native_backend(sample):
    """A 100-node chain has betweenness contributions only from the chosen
    sources: node i is credited by source s exactly when s < i < 99, so the
    sources NativeBackend used can be read off its result."""
    n = 100
    sources = list(brandes_sources(n, sample))
    g = _graph(n, [(i, i + 1) for i in range(n - 1)])
    want = NativeBackend().betweenness(g, sample=sample)
    expect = np.zeros(n)
    for s in sources:
        for i in range(s + 1, n - 1):
            expect[i] += n - 1 - i
    got = np.array([want[f"v{i:03d}"] for i in range(n)]) * ((n - 1) * (n - 2))
    np.testing.assert_allclose(got, expect, rtol=RTOL, atol=ATOL)
    if sample == 64:
        assert len(sources) == 100  # n // sample == 1: more sources than asked for
    if sample == 3:
        assert sources == list(range(0, 100, 33))


def test_get_backend_hip_resolution(monkeypatch):
    """hip needs a visible GPU and the built engine; anywhere else the request
    falls back to native instead of raising.  The default stays native."""
    import torch

    expected = "hip" if torch.cuda.is_available() and native.available() else "native"
    assert get_backend("hip").name == expected
    monkeypatch.setenv("AGENT_BOM_GRAPH_BACKEND", "hip")
    assert get_backend().name == expected
    monkeypatch.delenv("AGENT_BOM_GRAPH_BACKEND")
    assert get_backend().name == "native"


def test_batch_size_respects_workspace_budget(monkeypatch):
    from agentbom_amd.utils import config as cfg

    monkeypatch.setattr(cfg, "CENTRALITY_WS_MB", 4096)
    assert native.brandes_batch_size(7, 1031) == 7
    assert native.brandes_batch_size(500, 1031) == 64
    # 4 GiB / (20 B * 100M nodes) = 2 sources at a time
    assert native.brandes_batch_size(64, 100_000_000) == 2
    assert native.brandes_batch_size(64, 1_000_000_000) == 1


def test_heavy_degree_constant_mirrors_kernel():
    text = (Path(native.__file__).resolve().parent / "csrc" / "centrality.hip").read_text()
    m = re.search(r"constexpr uint64_t CENTRALITY_HEAVY_DEGREE = (\d+);", text)
    assert m and int(m.group(1)) == native.CENTRALITY_HEAVY_DEGREE


# ── REST ────────────────────────────────────────────────────────────────────


@pytest.fixture(scope="module")
def client_and_graph():
    from fastapi.testclient import TestClient

    from agentbom_amd.api.server import create_app

    app = create_app()
    c = TestClient(app)
    r = c.post("/v1/scan", json={"demo": True})
    assert r.status_code == 201
    return c, app.state.abom.graphs[r.json()["job_id"]]


def _top(scores: dict, k: int) -> list[str]:
    return [nid for nid, _ in sorted(scores.items(), key=lambda kv: (-kv[1], kv[0]))[:k]]


def test_rest_centrality_metrics(client_and_graph):
    client, g = client_and_graph
    pr = client.get("/v1/graph/centrality?metric=pagerank&top_n=7").json()
    assert [row["id"] for row in pr["centrality"]] == _top(g.pagerank(), 7)
    bc = client.get("/v1/graph/centrality?metric=betweenness&top_n=7&backend=native").json()
    assert [row["id"] for row in bc["centrality"]] == _top(g.betweenness(), 7)
    assert bc["centrality"][0]["score"] == max(g.betweenness().values())
    assert client.get("/v1/graph/centrality?metric=eigenvector").status_code == 422


def test_rest_bottlenecks_methods(client_and_graph):
    client, g = client_and_graph
    br = client.get("/v1/graph/bottlenecks?method=brandes&top_n=5").json()
    assert [row["id"] for row in br["bottlenecks"]] == _top(g.betweenness(), 5)
    assert client.get("/v1/graph/bottlenecks?method=exact").status_code == 422


def test_rest_defaults_unchanged(client_and_graph):
    client, g = client_and_graph
    cent = client.get("/v1/graph/centrality?top_n=5").json()
    assert cent == {"centrality": [{"id": nid, "degree": deg}
                                   for nid, deg in g.degree_centrality(5)]}
    assert cent == client.get("/v1/graph/centrality?top_n=5&metric=degree").json()
    bn = client.get("/v1/graph/bottlenecks?top_n=3").json()
    assert bn == {"bottlenecks": [{"id": nid, "score": round(score, 4)}
                                  for nid, score in g.bottlenecks(top_n=3, sample=64)]}
    assert bn == client.get("/v1/graph/bottlenecks?top_n=3&method=approx").json()
