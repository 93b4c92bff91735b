"""What the ahead arm (``abom_findings_ahead``) leaves for the next call on
the same workspace: bitmap, row counts and row tails all-zero after a hit
and after a forced miss, and blast counters that start at zero whatever was
in them, on one stream, from a side stream and with the two taking turns.
Everything goes through ``native.assemble_findings_begin_ahead`` and
``assemble_findings_finish``; every comparison is ``torch.equal``."""

from __future__ import annotations

import pytest
import torch

from match_by_window_cases import sized_case, tensors

from agentbom_amd.scan.synth import ET_CONTAINS, generate_estate

pytestmark = pytest.mark.gpu

ROOMY = 1 << 17
SIZES = (1, 255, 256, 257)
KEYS = ("pkg_idx", "win_idx", "pkg_nodes", "pos", "uniq_pkgs", "uniq_pkgs32",
        "blast_counts", "blast_overflow")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


@pytest.fixture(autouse=True)
def toggles(monkeypatch):
    for name in ("AGENT_BOM_FINDINGS_AHEAD", "AGENT_BOM_MATCH_TILED", "AGENT_BOM_BLAST_INDEX",
                 "AGENT_BOM_FINDINGS_NATIVE"):
        monkeypatch.delenv(name, raising=False)


class Graph:
    def __init__(self, dev):
        from agentbom_amd.graph.gpu_engine import EstateEngine

        self.est = generate_estate(n_agents=50, n_servers=200, n_packages=3000,
                                   name_catalog=500, extra_pkg_share=2.0, seed=7)
        self.eng = EstateEngine(self.est, device=dev)
        self.pkg_base = self.est.pkg_base

    def inputs(self, ws):
        from agentbom_amd.ops import native

        e = self.eng
        return native.blast_inputs(e.rev, e.reach_index, ET_CONTAINS,
                                   e.node_is_db_cred, e.node_is_db_tool, ws)


@pytest.fixture(scope="module")
def graph(dev):
    return Graph(dev)


def _match(case):
    from agentbom_amd.ops import native

    return native.match_by_window_launch(case[0]["windows"], case[2], capacity=ROOMY)


@pytest.fixture(scope="module")
def cases(dev, graph):
    """Per size: the match case and the host-sized result on fresh workspaces."""
    from agentbom_amd.ops import native

    e = graph.eng
    made = {}
    for n in SIZES:
        case = tensors(*sized_case(n), dev)
        want = native.assemble_findings(_match(case), case[1], graph.pkg_base, {})
        counts, overflow, n_overflow = native.blast_counts_indexed(
            want["uniq_pkgs32"], e.rev, e.reach_index, ET_CONTAINS,
            e.node_is_db_cred, e.node_is_db_tool, {})
        want.update(blast_counts=counts, blast_overflow=overflow, blast_n_overflow=n_overflow)
        assert want["pkg_idx"].numel() > 0
        made[n] = (case, want)
    return made


def _call(case, graph, ws, bws, side=None):
    """Begin (on ``side`` when given, the caller's stream then waiting for
    it, as the step does) and finish."""
    from agentbom_amd.ops import native

    def begin():
        return native.assemble_findings_begin_ahead(
            _match(case), case[1], ws, graph.pkg_base, graph.inputs(bws))

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
    for key in KEYS:
        assert got[key].shape == want[key].shape, key
        assert torch.equal(got[key], want[key]), key
    assert got["blast_n_overflow"] == want["blast_n_overflow"]


def _assert_workspace_as_the_next_call_sees_it(ws, bws, side=None):
    """What a next begin on that stream would find, with the stream order
    alone between the arm's reset and these reads."""
    stream = side or torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        dirty = [bool(ws[key].any()) for key in ("fa_bitmap", "fa_row_cnt", "fa_row_tail")]
    assert dirty == [False, False, False]
    assert ws["fa_dirty"] is False


@pytest.mark.parametrize("n", SIZES)
def test_workspace_is_zero_after_a_hit_and_counters_start_at_zero(cases, graph, n):
    case, want = cases[n]
    ws, bws = {}, {}
    _call(case, graph, ws, bws)                      # no prediction yet
    for _ in range(2):
        # whatever the last call left in the counters must not be counted
        bws["counters"].fill_(12345)
        got = _call(case, graph, ws, bws)
        assert ws["fa_ahead_hit"] is True
        _assert_equal(got, want)
        _assert_workspace_as_the_next_call_sees_it(ws, bws)
        queued, overflowed = bws["counters"].tolist()
        assert overflowed == want["blast_n_overflow"] == got["blast_n_overflow"]
        assert 0 <= queued <= want["uniq_pkgs"].numel()


@pytest.mark.parametrize("n", SIZES)
def test_workspace_is_zero_after_a_forced_miss(cases, graph, n):
    case, want = cases[n]
    F, NU = want["pkg_idx"].numel(), want["uniq_pkgs"].numel()
    ws, bws = {}, {}
    _call(case, graph, ws, bws)
    ws["fa_ahead_cap"] = (F - 1, NU)
    got = _call(case, graph, ws, bws)
    assert ws["fa_ahead_hit"] is False
    _assert_equal(got, want)
    _assert_workspace_as_the_next_call_sees_it(ws, bws)
    again = _call(case, graph, ws, bws)
    assert ws["fa_ahead_hit"] is True
    _assert_equal(again, want)
    _assert_workspace_as_the_next_call_sees_it(ws, bws)


@pytest.mark.parametrize("n", SIZES)
def test_hit_and_miss_from_a_side_stream(cases, graph, n):
    case, want = cases[n]
    F, NU = want["pkg_idx"].numel(), want["uniq_pkgs"].numel()
    side = torch.cuda.Stream()
    ws, bws = {}, {}
    _call(case, graph, ws, bws, side)
    for caps, hit in (((F, NU), True), ((F - 1, NU), False), ((F, NU), True)):
        ws["fa_ahead_cap"] = caps
        got = _call(case, graph, ws, bws, side)
        assert ws["fa_ahead_hit"] is hit
        _assert_equal(got, want)
    _assert_workspace_as_the_next_call_sees_it(ws, bws, side)
    # the next call may also come on another stream than the last one ran on
    got = _call(case, graph, ws, bws)
    assert ws["fa_ahead_hit"] is True
    _assert_equal(got, want)
    _assert_workspace_as_the_next_call_sees_it(ws, bws)


def test_two_cases_alternate_on_one_workspace(cases, graph):
    side = torch.cuda.Stream()
    ws, bws = {}, {}
    order = (255, 257, 1, 256, 257, 255, 1, 256)
    hits = 0
    for i, n in enumerate(order):
        case, want = cases[n]
        got = _call(case, graph, ws, bws, side if i % 2 else None)
        hits += ws["fa_ahead_hit"] is True
        _assert_equal(got, want)
    assert 0 < hits < len(order)     # the first call has no prediction to hit
    torch.cuda.synchronize()
    for key in ("fa_bitmap", "fa_row_cnt", "fa_row_tail"):
        assert not bool(ws[key].any()), key


def test_step_three_times_equal_and_equal_to_the_arm_off(dev, monkeypatch):
    from agentbom_amd.graph.gpu_engine import EstateEngine

    est = generate_estate(n_agents=400, n_servers=2000, n_packages=120_000,
                          name_catalog=20_000, seed=99, arena_windows=40_000)
    eng = EstateEngine(est, device=dev)
    first = eng.step()
    kept = {k: v.clone() for k, v in first.items() if isinstance(v, torch.Tensor)}
    second = eng.step()
    for key, value in kept.items():
        assert torch.equal(first[key], value), key   # step 2 left step 1's tensors alone
    third = eng.step()
    assert eng._findings_ws["fa_ahead_hit"] is True
    monkeypatch.setenv("AGENT_BOM_FINDINGS_AHEAD", "0")
    off = eng.step()
    assert first["n_findings"] > 0
    for other in (second, third, off):
        assert other["n_findings"] == first["n_findings"]
        for key, value in first.items():
            if isinstance(value, torch.Tensor):
                assert other[key].shape == value.shape, key
                assert torch.equal(other[key], value), key
    torch.cuda.synchronize()
    for key in ("fa_bitmap", "fa_row_cnt", "fa_row_tail"):
        assert not bool(eng._findings_ws[key].any()), key
