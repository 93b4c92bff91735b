"""Finding emit and blast counts sized from device memory
(``native.assemble_findings_begin_ahead``, ``abom_findings_ahead``,
``abom_blast_counts_indexed_sized``) and the step that runs them under the
reach BFS.  Every comparison is ``torch.equal`` against
``native.assemble_findings`` + ``native.blast_counts_indexed`` on a match of
the same case."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from match_by_window_cases import (
    HAND_ROWS,
    HAND_WINDOWS,
    I,
    row,
    sized_case,
    tensors,
    window,
)

from agentbom_amd.ops.cpu_ref import WF_CPU_FALLBACK
from agentbom_amd.scan.synth import ET_CONTAINS, generate_estate

pytestmark = pytest.mark.gpu

ROOMY = 1 << 17  # a pair capacity no case here can fill
ASSEMBLED = ("pkg_idx", "win_idx", "pkg_nodes", "pos", "uniq_pkgs", "uniq_pkgs32")
BLAST = ("blast_counts", "blast_overflow")
SRV_CAP = 64  # csrc/blast.hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


@pytest.fixture(autouse=True)
def toggles(monkeypatch):
    for name in ("AGENT_BOM_FINDINGS_AHEAD", "AGENT_BOM_MATCH_TILED",
                 "AGENT_BOM_BLAST_INDEX", "AGENT_BOM_FINDINGS_NATIVE"):
        monkeypatch.delenv(name, raising=False)


class Graph:
    """The graph side of the arm: the estate of tests/test_blast_index_gpu.py
    (3000 packages; single-server, multi-server and a few packages past the
    server cap).  The match cases use its first packages."""

    def __init__(self, dev):
        from agentbom_amd.graph.gpu_engine import EstateEngine

        self.est = generate_estate(n_agents=50, n_servers=200, n_packages=3000,
                                   name_catalog=500, extra_pkg_share=2.0, seed=7)
        self.eng = EstateEngine(self.est, device=dev)
        self.pkg_base = self.est.pkg_base
        self.index = self.eng.reach_index

    def inputs(self, ws, index=None):
        from agentbom_amd.ops import native

        e = self.eng
        return native.blast_inputs(e.rev, index or self.index, ET_CONTAINS,
                                   e.node_is_db_cred, e.node_is_db_tool, ws)

    def counts(self, pkgs32, index=None):
        from agentbom_amd.ops import native

        e = self.eng
        return native.blast_counts_indexed(
            pkgs32, e.rev, index or self.index, ET_CONTAINS,
            e.node_is_db_cred, e.node_is_db_tool, {})


@pytest.fixture(scope="module")
def graph(dev):
    return Graph(dev)


def _match(case, capacity=ROOMY):
    from agentbom_amd.ops import native

    arena, _layout, table = case
    return native.match_by_window_launch(arena["windows"], table, capacity=capacity)


def _want(case, graph):
    """The host-sized path on a fresh workspace, plus its blast counts."""
    from agentbom_amd.ops import native

    out = native.assemble_findings(_match(case), case[1], graph.pkg_base, {})
    counts, overflow, n_overflow = graph.counts(out["uniq_pkgs32"])
    out.update(blast_counts=counts, blast_overflow=overflow, blast_n_overflow=n_overflow)
    return out


def _ahead(case, graph, ws, bws, side=None, capacity=ROOMY):
    """Match and the begin part (on ``side`` when given), then the finish."""
    from agentbom_amd.ops import native

    def begin():
        return native.assemble_findings_begin_ahead(
            _match(case, capacity), case[1], ws, graph.pkg_base, graph.inputs(bws))

    if side is None:
        state = begin()
    else:
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            state = begin()
        main.wait_stream(side)
    return native.assemble_findings_finish(state, graph.pkg_base)


def _assert_equal(got, want):
    for key in ASSEMBLED + BLAST:
        assert got[key].dtype == want[key].dtype, key
        assert got[key].shape == want[key].shape, key
        assert torch.equal(got[key], want[key]), key
        assert got[key].is_contiguous(), key
    assert got["blast_n_overflow"] == want["blast_n_overflow"]


def _assert_clean(ws):
    assert ws["fa_dirty"] is False
    for key in ("fa_bitmap", "fa_row_cnt", "fa_row_tail"):
        assert not bool(ws[key].any()), key


def _sizes(want):
    return want["pkg_idx"].numel(), want["uniq_pkgs"].numel()


# ── first call, hits, forced misses ────────────────────────────────────────

@pytest.fixture(scope="module")
def cases(dev, graph):
    """Match cases by name, each with its expected result."""
    made = {"hand": tensors(HAND_ROWS, HAND_WINDOWS, dev)}
    for n in (1, 255, 256, 257, 513):
        made[n] = tensors(*sized_case(n), dev)
    return {name: (case, _want(case, graph)) for name, case in made.items()}


@pytest.mark.parametrize("name", ["hand", 1, 255, 256, 257, 513])
def test_first_call_then_hits(cases, graph, name):
    from agentbom_amd.ops import native

    case, want = cases[name]
    F, NU = _sizes(want)
    assert F > 0 and NU > 0
    ws, bws = {}, {}
    for call, hit in enumerate((False, True, True)):
        got = _ahead(case, graph, ws, bws)
        assert ws["fa_ahead_hit"] is hit, call
        _assert_equal(got, want)
        _assert_clean(ws)
        assert ws["fa_ahead_cap"] == (native.findings_ahead_capacity(F),
                                      native.findings_ahead_capacity(NU))


def test_forced_misses_fall_back_and_the_next_call_hits(cases, graph):
    case, want = cases[513]
    F, NU = _sizes(want)
    assert F > 1 and NU > 1 and want["blast_n_overflow"] >= 0
    ws, bws = {}, {}
    _ahead(case, graph, ws, bws)
    for caps, hit in (((F - 1, NU), False), ((F, NU - 1), False), ((0, 0), False),
                      ((F, NU), True), ((F + 1000, NU + 1000), True)):
        ws["fa_ahead_cap"] = caps
        got = _ahead(case, graph, ws, bws)
        assert ws["fa_ahead_hit"] is hit, caps
        _assert_equal(got, want)
        _assert_clean(ws)
        again = _ahead(case, graph, ws, bws)
        assert ws["fa_ahead_hit"] is True, caps
        _assert_equal(again, want)
        _assert_clean(ws)


def test_changing_estate_misses_growing_and_fits_shrinking(cases, graph):
    """Two cases alternate on one workspace.  The larger after the smaller
    does not fit; the smaller after the larger fits unless the capacities
    are forced down to what the smaller one before it needed."""
    from agentbom_amd.ops import native

    small, want_small = cases[255]
    big, want_big = cases[513]
    assert _sizes(want_big)[0] > native.findings_ahead_capacity(_sizes(want_small)[0])
    ws, bws = {}, {}
    _assert_equal(_ahead(small, graph, ws, bws), want_small)
    for _ in range(2):
        _assert_equal(_ahead(big, graph, ws, bws), want_big)
        assert ws["fa_ahead_hit"] is False  # grew past the prediction
        _assert_clean(ws)
        _assert_equal(_ahead(small, graph, ws, bws), want_small)
        assert ws["fa_ahead_hit"] is True   # shrank: a shorter view of the outputs
        _assert_clean(ws)
    # shrinking below a prediction that is wrong in the other quantity
    ws["fa_ahead_cap"] = (_sizes(want_big)[0], _sizes(want_small)[1] - 1)
    _assert_equal(_ahead(small, graph, ws, bws), want_small)
    assert ws["fa_ahead_hit"] is False
    _assert_clean(ws)


def _empty_cases(dev):
    rows = [row(10, 1, 3 * i + 1) for i in range(9)]
    nothing = [window(10, I, intro=(9, 0)) for _ in range(300)]       # above every row
    fallback = [window(10, I | WF_CPU_FALLBACK, intro=(1, 1)) for _ in range(300)]
    return tensors(rows, nothing, dev), tensors(rows, fallback, dev)


def test_no_findings(dev, graph):
    for case in _empty_cases(dev):
        want = _want(case, graph)
        assert _sizes(want) == (0, 0)
        ws, bws = {}, {}
        for hit in (False, True, True):
            got = _ahead(case, graph, ws, bws)
            assert ws["fa_ahead_hit"] is hit
            _assert_equal(got, want)
            assert got["blast_counts"].shape == (0, 6)
            _assert_clean(ws)


def test_findings_after_none_and_none_after_findings(dev, cases, graph):
    nothing, _ = _empty_cases(dev)
    want_nothing = _want(nothing, graph)
    some, want_some = cases[257]
    ws, bws = {}, {}
    _ahead(nothing, graph, ws, bws)
    for case, want in ((some, want_some), (nothing, want_nothing), (some, want_some)):
        _assert_equal(_ahead(case, graph, ws, bws), want)
        _assert_clean(ws)


def test_pair_buffer_overflow_with_a_prediction(cases, graph):
    """capacity=8: the device condition fails on the match count, the match is
    relaunched and the host-sized path runs."""
    case, want = cases[257]
    F, NU = _sizes(want)
    assert F > 8
    ws, bws = {}, {}
    _ahead(case, graph, ws, bws)
    assert ws["fa_ahead_cap"][0] >= F
    got = _ahead(case, graph, ws, bws, capacity=8)
    assert ws["fa_ahead_hit"] is False
    _assert_equal(got, want)
    _assert_clean(ws)
    _assert_equal(_ahead(case, graph, ws, bws), want)
    assert ws["fa_ahead_hit"] is True


def test_begin_on_a_side_stream(cases, graph, dev):
    case, want = cases[513]
    side = torch.cuda.Stream(device=dev)
    ws, bws = {}, {}
    for hit in (False, True, True):
        got = _ahead(case, graph, ws, bws, side=side)
        assert ws["fa_ahead_hit"] is hit
        _assert_equal(got, want)
        _assert_clean(ws)
    one_ws, one_bws = {}, {}
    for _ in range(2):
        same = _ahead(case, graph, one_ws, one_bws)
    for key in ASSEMBLED + BLAST:
        assert torch.equal(got[key], same[key]), key


def test_results_of_two_calls_share_no_storage(cases, graph):
    case, want = cases[513]
    ws, bws = {}, {}
    _ahead(case, graph, ws, bws)
    first = _ahead(case, graph, ws, bws)
    kept = {k: first[k].clone() for k in ASSEMBLED + BLAST}
    second = _ahead(case, graph, ws, bws)
    assert ws["fa_ahead_hit"] is True
    for key in ASSEMBLED + BLAST:
        assert first[key].data_ptr() != second[key].data_ptr(), key
        second[key].zero_()
        assert torch.equal(first[key], kept[key]), key


# ── blast counts sized from the device ─────────────────────────────────────

@pytest.fixture(scope="module")
def package_order(graph):
    """All packages, ordered so that the shortest prefixes already hold a
    multi-server package, a single-server one and one past the server cap."""
    est = graph.est
    m = est.edge_type == ET_CONTAINS
    pairs = np.unique(np.stack([est.edge_dst[m] - est.pkg_base, est.edge_src[m]], 1), axis=0)
    per_pkg = np.bincount(pairs[:, 0], minlength=est.n_packages)
    multi = int(np.nonzero((per_pkg > 1) & (per_pkg <= SRV_CAP))[0][0])
    single = int(np.nonzero(per_pkg == 1)[0][0])
    over = int(np.nonzero(per_pkg > SRV_CAP)[0][0])
    head = [multi, single, over]
    rest = [p for p in range(est.n_packages) if p not in head]
    order = np.array(head + rest, dtype=np.int64) + est.pkg_base
    return torch.from_numpy(order).to(torch.int32).to(graph.eng.device)


@pytest.mark.parametrize("slack", [0, 100])
@pytest.mark.parametrize("n", [0, 1, 3, 63, 64, 65, 1000])
def test_blast_counts_sized_from_the_device(graph, package_order, n, slack):
    from agentbom_amd.ops import native

    e = graph.eng
    pkgs = package_order[:n + slack].contiguous()
    n_dev = torch.tensor([n], dtype=torch.int64, device=pkgs.device)
    counts, overflow, queued, n_overflow = native.blast_counts_indexed_sized(
        pkgs, n_dev, e.rev, graph.index, ET_CONTAINS, e.node_is_db_cred,
        e.node_is_db_tool, {})
    ws = {}
    want_counts, want_overflow, want_n = native.blast_counts_indexed(
        pkgs[:n].contiguous(), e.rev, graph.index, ET_CONTAINS, e.node_is_db_cred,
        e.node_is_db_tool, ws)
    assert counts.numel() == 6 * (n + slack) and overflow.numel() == n + slack
    assert torch.equal(counts[:6 * n].view(n, 6), want_counts)
    assert torch.equal(overflow[:n], want_overflow)
    assert n_overflow == want_n
    assert queued == int(ws["counters"][0].item())
    if n >= 3:
        assert n_overflow >= 1 and queued >= 2  # the overflow word came through the pinned copy
        assert int(overflow[2]) == 1


def test_blast_counts_sized_with_packages_outside_the_index(graph, package_order):
    """An index over a slice of the servers: packages of the others are
    flagged, by the thread pass and by the wave pass."""
    from agentbom_amd.ops import native

    e = graph.eng
    full = graph.index
    part = dict(full, row_base=full["row_base"] + 20,
                reach_off=full["reach_off"][20:120].contiguous(),
                reach_db=full["reach_db"][20:120].contiguous())
    n = 1000
    pkgs = package_order[:n + 50].contiguous()
    n_dev = torch.tensor([n], dtype=torch.int64, device=pkgs.device)
    counts, overflow, _queued, n_overflow = native.blast_counts_indexed_sized(
        pkgs, n_dev, e.rev, part, ET_CONTAINS, e.node_is_db_cred, e.node_is_db_tool, {})
    want_counts, want_overflow, want_n = graph.counts(pkgs[:n].contiguous(), index=part)
    assert want_n > 100 and n_overflow == want_n
    assert torch.equal(counts[:6 * n].view(n, 6), want_counts)
    assert torch.equal(overflow[:n], want_overflow)


def test_overflowed_rows_reach_the_join_through_the_arm(dev, graph):
    """Every package of the graph gets a finding, so the arm's blast counts
    include the packages past the server cap; the step's resolve turns the
    flagged rows into the join's counts."""
    from agentbom_amd.ops import native

    n = graph.est.n_packages
    rows = [row(10, 1, i + 1) for i in range(n // 2)]  # tensors() doubles them
    case = tensors(rows, [window(10, 0)], dev)
    want = _want(case, graph)
    assert _sizes(want) == (n, n) and want["blast_n_overflow"] >= 1
    ws, bws = {}, {}
    _ahead(case, graph, ws, bws)
    got = _ahead(case, graph, ws, bws)
    assert ws["fa_ahead_hit"] is True
    _assert_equal(got, want)
    resolved = graph.eng._blast_counts_resolve(
        got["uniq_pkgs"], got["blast_counts"], got["blast_overflow"], got["blast_n_overflow"])
    exact = graph.eng._blast_counts_join(got["uniq_pkgs"])
    for k, key in enumerate(("n_servers", "n_agents", "n_creds_all", "n_creds_db",
                             "n_tools_all", "n_tools_db")):
        assert torch.equal(resolved[key], exact[key]), key
        assert torch.equal(resolved["counts2d"][:, k], exact[key]), key
    assert native.findings_ahead_capacity(n) >= n


# ── the step ───────────────────────────────────────────────────────────────

@pytest.fixture(scope="module")
def estate():
    return generate_estate(n_agents=400, n_servers=2000, n_packages=120_000,
                           name_catalog=20_000, seed=99, arena_windows=40_000)


def test_step_three_times_then_toggle_off(dev, estate, monkeypatch):
    from agentbom_amd.graph.gpu_engine import EstateEngine, findings_ahead_enabled

    eng = EstateEngine(estate, device=dev)
    assert eng.match_dedup is not None and eng.reach_index is not None
    assert findings_ahead_enabled()
    first = eng.step()
    assert eng._findings_ws["fa_ahead_hit"] is False
    kept = {k: v.clone() for k, v in first.items() if isinstance(v, torch.Tensor)}
    second = eng.step()
    assert eng._findings_ws["fa_ahead_hit"] is True
    for key, value in kept.items():
        assert torch.equal(first[key], value), key  # step 2 left step 1's tensors alone
    third = eng.step()
    assert eng._findings_ws["fa_ahead_hit"] is True
    monkeypatch.setenv("AGENT_BOM_FINDINGS_AHEAD", "0")
    assert not findings_ahead_enabled()
    eng._findings_ws["fa_ahead_hit"] = None
    off = eng.step()
    assert eng._findings_ws["fa_ahead_hit"] is None  # the arm did not run
    assert first["n_findings"] > 0
    for other in (second, third, off):
        assert other.keys() == first.keys()
        assert other["n_findings"] == first["n_findings"]
        for key, value in first.items():
            if isinstance(value, torch.Tensor):
                assert other[key].dtype == value.dtype, key
                assert other[key].shape == value.shape, key
                assert torch.equal(other[key], value), key


def test_step_with_given_reach_distances(dev, estate):
    """``step(reach_dist=...)``, the distributed engine's call, takes the arm too."""
    from agentbom_amd.graph.gpu_engine import EstateEngine

    eng = EstateEngine(estate, device=dev)
    assert eng.match_dedup is not None and eng.reach_index is not None
    base = eng.step()
    dist = base["reach_dist"].clone()
    for hit in (True, True):
        got = eng.step(reach_dist=dist)
        assert eng._findings_ws["fa_ahead_hit"] is hit
        for key, value in base.items():
            if isinstance(value, torch.Tensor):
                assert torch.equal(got[key], value), key
