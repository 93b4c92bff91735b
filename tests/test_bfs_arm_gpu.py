"""The reach BFS arm: staged frontier appends, the early stop of the
bottom-up level loop, the begin/run split with its 16-byte fill, and the
step that uses them.  Every comparison is exact equality with cpu_ref.bfs.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UNVISITED = 0xFFFFFFFF
STAGE = 4096          # BFS_STAGE, csrc/bfs.hip: entries of a block's LDS claim queue
GRID_THREADS = 2048 * 256  # the largest grid of bfs_expand_kernel: one grid-stride round


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _csr(src, dst, et, n):
    """CSR by stable sort on source (as EstateEngine._build_csr)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    et = np.asarray(et, dtype=np.uint8)
    order = np.argsort(src, kind="stable")
    row_off = np.zeros(n + 1, dtype=np.int64)
    row_off[1:] = np.cumsum(np.bincount(src, minlength=n))
    return {"row_off": row_off, "col": dst[order].astype(np.int32),
            "etype": et[order], "src": src[order].astype(np.int32)}


def _to_dev(csr, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in csr.items()}


def _graph(edges, n, dev):
    """{fwd, rev (device CSRs), np (host forward CSR), n} of an edge list of
    (src, dst) or (src, dst, type) rows."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 3 if edges and len(edges[0]) == 3 else 2)
    src, dst = e[:, 0], e[:, 1]
    et = e[:, 2] if e.shape[1] == 3 else np.zeros(len(e), dtype=np.int64)
    fwd = _csr(src, dst, et, n)
    return {"np": fwd, "fwd": _to_dev(fwd, dev), "rev": _to_dev(_csr(dst, src, et, n), dev),
            "n": n}


def _ref(g, sources=(0,), mask=0xFFFFFFFF, max_levels=64):
    from agentbom_amd.ops import cpu_ref

    c = g["np"]
    return cpu_ref.bfs(c["row_off"], c["col"], np.asarray(sources), g["n"],
                       etype=c["etype"], allowed_mask=mask, max_levels=max_levels)


def _bfs(g, dev, mode="sparse", sources=(0,), mask=0xFFFFFFFF, **kw):
    from agentbom_amd.ops import native

    fwd = g["fwd"]
    dist = native.bfs(
        fwd["row_off"], fwd["col"],
        torch.tensor(list(sources), dtype=torch.int32, device=dev), g["n"],
        etype=fwd["etype"], allowed_mask=mask,
        edge_src=None if mode == "sparse" else fwd["src"],
        rev=g["rev"] if mode == "bottom_up" else None, **kw)
    return dist.cpu().numpy().view(np.uint32)


# ── staged append ───────────────────────────────────────────────────────────
#
# fan(F, d): 0 -> F vertices -> d distinct leaves each.  Level 2 expands a
# frontier of F vertices of out-degree d; `short` gives vertex 1 d + short
# leaves instead.

def _fan_edges(frontier, degree, short=0):
    src = [np.zeros(frontier, dtype=np.int64)]
    dst = [np.arange(1, frontier + 1, dtype=np.int64)]
    deg = np.full(frontier, degree, dtype=np.int64)
    deg[0] += short
    src.append(np.repeat(np.arange(1, frontier + 1, dtype=np.int64), deg))
    dst.append(frontier + 1 + np.arange(deg.sum(), dtype=np.int64))
    n = 1 + frontier + int(deg.sum())
    return np.stack([np.concatenate(src), np.concatenate(dst)], axis=1), n


def _fan(frontier, degree, dev, short=0):
    edges, n = _fan_edges(frontier, degree, short)
    fwd = _csr(edges[:, 0], edges[:, 1], np.zeros(len(edges)), n)
    return {"np": fwd, "fwd": _to_dev(fwd, dev), "n": n, "rev": None, "frontier": frontier}


FAN_CASES = [(f, d, 0) for f in (1, 255, 256, 257) for d in (0, 1, 63, 64)]
# one block (256 frontier vertices) claiming 4095, 4096 and 4097 vertices
FAN_CASES += [(256, STAGE // 256, s) for s in (-1, 0, 1)]


@pytest.fixture(scope="module")
def fans(dev):
    out = {}
    for f, d, s in FAN_CASES:
        g = _fan(f, d, dev, short=s)
        g["ref"] = _ref(g)
        out[(f, d, s)] = g
    return out


@pytest.fixture(scope="module")
def second_round(dev):
    """A frontier one longer than the largest grid: the last vertex is
    expanded in a second grid-stride round."""
    g = _fan(GRID_THREADS + 1, 1, dev)
    g["ref"] = _ref(g)
    return g


@pytest.fixture(scope="module")
def shared_targets(dev):
    """10k frontier vertices that all point at the same 3 targets."""
    f = 10_000
    edges = [(0, v) for v in range(1, f + 1)]
    edges += [(v, f + 1 + t) for v in range(1, f + 1) for t in range(3)]
    g = _graph(edges, f + 4, dev)
    g["frontier"] = f
    g["ref"] = _ref(g)
    return g


@pytest.mark.parametrize("case", FAN_CASES, ids=lambda c: "F%d-d%d%+d" % c)
def test_staged_append_fans(fans, dev, case):
    g = fans[case]
    assert case[2] == 0 or int((g["ref"] == 2).sum()) == STAGE + case[2]
    assert np.array_equal(_bfs(g, dev), g["ref"])


def test_staged_append_second_round(second_round, dev):
    g = second_round
    assert g["n"] == 2 * (GRID_THREADS + 1) + 1
    ws: dict = {}
    assert np.array_equal(_bfs(g, dev, workspace=ws), g["ref"])
    assert ws["levels"] == 3  # the level after the leaves finds nothing


def test_staged_append_shared_targets(shared_targets, dev):
    g = shared_targets
    dist = _bfs(g, dev)
    assert np.array_equal(dist, g["ref"])
    assert int((dist == 2).sum()) == 3


def _level_two(g, dev):
    """bfs_level from the level-1 frontier of a fan-shaped graph."""
    from agentbom_amd.ops import native

    f = g["frontier"]
    dist = np.full(g["n"], UNVISITED, dtype=np.uint32)
    dist[0], dist[1:f + 1] = 0, 1
    dist_t = torch.from_numpy(dist.view(np.int32)).to(dev)
    frontier = torch.arange(1, f + 1, dtype=torch.int32, device=dev)
    fwd = g["fwd"]
    nxt = native.bfs_level(fwd["row_off"], fwd["col"], frontier, dist_t, 2,
                           etype=fwd["etype"])
    return nxt.cpu().numpy(), dist_t.cpu().numpy().view(np.uint32)


def _check_level_two(g, dev):
    nxt, dist = _level_two(g, dev)
    assert len(np.unique(nxt)) == len(nxt)
    assert np.array_equal(np.sort(nxt), np.flatnonzero(g["ref"] == 2))
    assert np.array_equal(dist, g["ref"])


@pytest.mark.parametrize("case", FAN_CASES, ids=lambda c: "F%d-d%d%+d" % c)
def test_bfs_level_fans(fans, dev, case):
    _check_level_two(fans[case], dev)


def test_bfs_level_second_round(second_round, dev):
    _check_level_two(second_round, dev)


def test_bfs_level_shared_targets(shared_targets, dev):
    _check_level_two(shared_targets, dev)


@pytest.mark.parametrize("case,capacity", [((256, 16, 0), 1000), ((256, 63, 0), 5000),
                                           ((256, 64, 0), 100)],
                         ids=["staged", "staged+direct", "heavy"])
def test_capacity_guard_drops_writes(fans, dev, case, capacity):
    """More claims than ``capacity``: the count is exact, the first
    ``capacity`` slots hold distinct claimed vertices and nothing is written
    past them.  (bfs_level sizes the list by dist, which cannot be shorter
    than the claims it holds, so this calls the two launches directly.)"""
    from agentbom_amd.ops import native

    g = fans[case]
    lib = native.load()
    f, fwd = g["frontier"], g["fwd"]
    claims = int((g["ref"] == 2).sum())
    assert claims > capacity
    dist = np.full(g["n"], UNVISITED, dtype=np.uint32)
    dist[0], dist[1:f + 1] = 0, 1
    dist_t = torch.from_numpy(dist.view(np.int32)).to(dev)
    frontier = torch.arange(1, f + 1, dtype=torch.int32, device=dev)
    nxt = torch.full((capacity + 4096,), -7, dtype=torch.int32, device=dev)
    hq = torch.empty(f, dtype=torch.int32, device=dev)
    ctr = torch.zeros(4, dtype=torch.int32, device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.abom_bfs_expand(p(fwd["row_off"]), p(fwd["col"]), p(fwd["etype"]), 0xFFFFFFFF,
                             p(frontier), f, p(dist_t), 2, p(nxt), p(ctr), p(hq), p(ctr, 4),
                             p(ctr, 8), capacity, stream)
    assert rc == 0
    rc = lib.abom_bfs_expand_heavy(p(fwd["row_off"]), p(fwd["col"]), p(fwd["etype"]),
                                   0xFFFFFFFF, p(hq), p(ctr, 4), p(dist_t), 2, p(nxt), p(ctr),
                                   p(ctr, 8), capacity, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(ctr[0]) == claims
    got = nxt.cpu().numpy()
    assert (got[capacity:] == -7).all()
    kept = got[:capacity]
    assert len(np.unique(kept)) == capacity
    assert (g["ref"][kept] == 2).all()
    assert np.array_equal(dist_t.cpu().numpy().view(np.uint32), g["ref"])


# ── early stop of the bottom-up loop ────────────────────────────────────────
#
# 4 agents -> 8 servers each -> 20 leaves each: E = 672, the agents' 32 edges
# stay under E/8 (level 1 sparse), the servers' 640 are over it (level 2
# bottom-up).  Node ids: agents 0-3, servers 4-35, leaves 36-675, then extras.

_AGENTS, _SERVERS, _LEAVES = 4, 32, 640
_ESTATE_N = _AGENTS + _SERVERS + _LEAVES
_SOURCES = tuple(range(_AGENTS))


def _estate_edges():
    edges = [(a, _AGENTS + 8 * a + k, 0) for a in range(_AGENTS) for k in range(8)]
    edges += [(_AGENTS + s, _AGENTS + _SERVERS + 20 * s + k, 0)
              for s in range(_SERVERS) for k in range(20)]
    return edges


def _levels(g, dev, mask=0x1, **kw):
    ws: dict = {}
    dist = _bfs(g, dev, mode="bottom_up", sources=_SOURCES, mask=mask, workspace=ws, **kw)
    return dist, ws["levels"]


def test_early_stop_estate_shape(dev):
    g = _graph(_estate_edges(), _ESTATE_N, dev)
    dist, levels = _levels(g, dev)
    assert np.array_equal(dist, _ref(g, _SOURCES, 0x1))
    assert dist.max() == 2
    assert levels == 2


def test_no_early_stop_with_unreached_parent(dev):
    """X has an allowed in-edge from a parent nothing reaches: the level-2
    pass cannot rule X out, so a third pass runs (and claims nothing)."""
    parent, x = _ESTATE_N, _ESTATE_N + 1
    g = _graph(_estate_edges() + [(parent, x, 0)], _ESTATE_N + 2, dev)
    dist, levels = _levels(g, dev)
    assert np.array_equal(dist, _ref(g, _SOURCES, 0x1))
    assert dist[x] == UNVISITED and dist[parent] == UNVISITED
    assert levels == 3


@pytest.mark.parametrize("parent", [_AGENTS, _ESTATE_N], ids=["reached", "unreached"])
def test_masked_in_edge_does_not_keep_loop_alive(dev, parent):
    """X's only in-edge has a masked type, from a server or from a vertex
    nothing reaches."""
    x = _ESTATE_N + 1
    g = _graph(_estate_edges() + [(parent, x, 5)], _ESTATE_N + 2, dev)
    dist, levels = _levels(g, dev)
    assert np.array_equal(dist, _ref(g, _SOURCES, 0x1))
    assert dist[x] == UNVISITED
    assert levels == 2
    # with every type allowed the edge counts again
    dist, levels = _levels(g, dev, mask=0xFFFFFFFF)
    assert np.array_equal(dist, _ref(g, _SOURCES))
    assert levels == (2 if parent == _AGENTS else 3)


def test_max_levels_still_truncates(dev):
    g = _graph(_estate_edges(), _ESTATE_N, dev)
    dist, levels = _levels(g, dev, max_levels=1)
    assert np.array_equal(dist, _ref(g, _SOURCES, 0x1, max_levels=1))
    assert dist.max() == UNVISITED and dist[dist != UNVISITED].max() == 1
    assert levels == 1


# ── begin/run split, the 16-byte fill ───────────────────────────────────────

def _star_chain(n):
    """0 -> 1..n-42, then 1 -> a chain through the last 41 vertices; for a
    small n a plain chain 0 -> 1 -> ... -> n-1."""
    if n < 300:
        return [(v, v + 1) for v in range(n - 1)]
    star = n - 42
    edges = [(0, v) for v in range(1, star + 1)]
    edges.append((1, star + 1))
    edges += [(v, v + 1) for v in range(star + 1, n - 1)]
    return edges


def _split_bfs(g, dev, ws, mode="sparse", sources=(0,), **kw):
    from agentbom_amd.ops import native

    src = torch.tensor(list(sources), dtype=torch.int32, device=dev)
    native.bfs_begin(g["fwd"]["row_off"], src, g["n"], ws)
    return _bfs(g, dev, mode=mode, sources=sources, workspace=ws, begun=True, **kw)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8202])
@pytest.mark.parametrize("offset", [0, 1, 3], ids=lambda o: "head%d" % ((4 - o) % 4))
def test_begin_then_run_equals_one_shot(dev, n, offset):
    """The split call, on a ``dist`` that starts 0, 3 or 1 words before a
    16-byte boundary and is longer than the graph: the words past N are
    left alone."""
    g = _graph(_star_chain(n), n, dev)
    ref = _ref(g)
    assert np.array_equal(_bfs(g, dev), ref)
    backing = torch.full((n + 16,), 123, dtype=torch.int32, device=dev)
    assert backing.data_ptr() % 16 == 0
    ws = {"dist": backing[offset:offset + n + 7]}
    for _ in range(2):
        assert np.array_equal(_split_bfs(g, dev, ws), ref)
        assert ws["dist"].data_ptr() == backing.data_ptr() + 4 * offset
        assert (backing[:offset] == 123).all() and (backing[offset + n:] == 123).all()
    for mode in ("bottom_up", "edge_dense"):
        assert np.array_equal(_split_bfs(g, dev, ws, mode=mode), ref)
    assert (backing[:offset] == 123).all() and (backing[offset + n:] == 123).all()


def test_workspace_of_a_larger_graph(dev):
    big = _graph(_star_chain(8202), 8202, dev)
    small = _graph(_star_chain(5), 5, dev)
    ws: dict = {}
    assert np.array_equal(_bfs(big, dev, workspace=ws), _ref(big))
    assert np.array_equal(_split_bfs(small, dev, ws), _ref(small))
    assert np.array_equal(_bfs(small, dev, workspace=ws), _ref(small))
    assert ws["dist"].numel() == 8202
    assert np.array_equal(_split_bfs(big, dev, ws, mode="bottom_up"), _ref(big))


def test_begun_needs_the_workspace(dev):
    g = _graph(_star_chain(5), 5, dev)
    with pytest.raises(ValueError):
        _bfs(g, dev, begun=True)
    with pytest.raises(ValueError):
        _bfs(g, dev, begun=True, workspace={})


@pytest.mark.parametrize("mode", ["sparse", "bottom_up", "edge_dense"])
@pytest.mark.parametrize("sources", [(0,), (0, 0), (0, 1, 5)])
def test_sources_degree_given_or_read(dev, mode, sources):
    g = _graph(_star_chain(8202), 8202, dev)
    ref = _ref(g, sources)
    row_off = g["np"]["row_off"]
    degree = int(sum(row_off[s + 1] - row_off[s] for s in sources))
    read = _bfs(g, dev, mode=mode, sources=sources)
    given = _bfs(g, dev, mode=mode, sources=sources, sources_degree=degree)
    split = _split_bfs(g, dev, {}, mode=mode, sources=sources, sources_degree=degree)
    assert np.array_equal(read, ref)
    assert np.array_equal(given, ref)
    assert np.array_equal(split, ref)


# ── the step ────────────────────────────────────────────────────────────────

def test_step_equals_step_on_cpu_reach(dev):
    """EstateEngine.step() twice on one engine (fill and seed ahead of the
    match, early stop, known source degree) against a step fed the CPU
    engine's dependency_reach()."""
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=400, n_servers=2000, n_packages=120_000,
                          name_catalog=20_000, seed=99, arena_windows=40_000)
    eng = EstateEngine(est, device=dev)
    cpu_dist = EstateEngine(est, device="cpu").dependency_reach()
    want = eng.step(reach_dist=cpu_dist.to(dev))
    assert want["n_findings"] > 0
    for _ in range(2):
        got = eng.step()
        assert got["n_findings"] == want["n_findings"]
        for key, value in want.items():
            if isinstance(value, torch.Tensor):
                assert got[key].dtype == value.dtype, key
                assert torch.equal(got[key], value), key
    assert eng._bfs_ws["levels"] == 2
