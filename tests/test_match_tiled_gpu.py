"""The block-tiled window match (ops/csrc/match.hip,
``match_by_window_tiled_kernel``), the split finding assembly
(``native.assemble_findings_begin`` / ``assemble_findings_finish``) and the
step that uses both.  Every comparison is exact: pairs as sorted sets against
the row kernel and ``cpu_ref.match``, assembled tensors with ``torch.equal``."""

from __future__ import annotations

import pytest
import torch

from match_by_window_cases import (
    HAND_ROWS,
    HAND_WINDOWS,
    F,
    I,
    L,
    reference_pairs,
    row,
    sized_case,
    tensors,
    window,
)

from agentbom_amd.ops.cpu_ref import WF_CPU_FALLBACK

pytestmark = pytest.mark.gpu

TILE = 256   # MT_TILE, csrc/match.hip
CAP = 1024   # MT_CAP
PKG_BASE = 1_000_003
ROOMY = 1 << 17  # a pair capacity no case here can fill
ASSEMBLED = ("pkg_idx", "win_idx", "pkg_nodes", "pos", "uniq_pkgs", "uniq_pkgs32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


@pytest.fixture(autouse=True)
def tiled(monkeypatch):
    from agentbom_amd.ops import native

    monkeypatch.delenv("AGENT_BOM_MATCH_TILED", raising=False)
    assert native.match_tiled_enabled()


def _row_launch(arena, layout, capacity=ROOMY):
    from agentbom_amd.ops import native

    return native.match_launch(
        layout["u_gk"], layout["u_hi"], layout["u_lo"], layout["u_flags"],
        arena["group_keys"], arena["group_off"], arena["windows"],
        pkg_win_range=layout["u_ranges"], order=layout["heavy_order"], capacity=capacity)


def _sorted_pairs(pending):
    from agentbom_amd.ops import native

    rows, wins = native.match_finalize(pending, sort=True)
    return (rows << 32) | wins


def _as_set(pairs):
    return {(int(p) >> 32, int(p) & 0xFFFFFFFF) for p in pairs.tolist()}


def _check(arena, layout, table):
    """Tiled kernel == row kernel == cpu_ref.match; returns the sorted pairs."""
    from agentbom_amd.ops import native

    got = _sorted_pairs(native.match_by_window_launch(arena["windows"], table, capacity=ROOMY))
    assert torch.equal(got, _sorted_pairs(_row_launch(arena, layout)))
    assert _as_set(got) == reference_pairs(arena, layout)
    return got


def _key(i):
    return 1, 3 * i + 1


# ── tiles and their row slices ─────────────────────────────────────────────

def test_every_window_form(dev):
    got = _check(*tensors(HAND_ROWS, HAND_WINDOWS, dev))
    assert got.numel() > 60


@pytest.mark.parametrize("n_windows", [1, 255, 256, 257, 513])
def test_partial_tiles_and_groups_across_tiles(dev, n_windows):
    """The last tile partly filled; with 257 and 513 windows the five groups
    of sized_case straddle tile boundaries.  One window emits 300 rows."""
    arena, layout, table = tensors(*sized_case(n_windows), dev)
    assert arena["windows"]["flags"].numel() == n_windows
    got = _check(arena, layout, table)
    spans = torch.bincount(got & 0xFFFFFFFF, minlength=n_windows)
    assert int(spans.max()) == 300
    if n_windows > TILE:
        off = arena["group_off"].cpu().tolist()
        assert any(a < TILE < b for a, b in zip(off, off[1:]))


def _edge_case(total_rows: int, first: int = 600):
    """One tile whose slice is ``total_rows`` rows: a group of ``first`` rows
    and one of the rest, with windows whose bounds sit on the rows around the
    staged edge (row CAP - 1 is the last staged one)."""
    sizes = {21: first, 22: total_rows - first}
    rows = [row(g, *_key(i)) for g, n in sizes.items() for i in range(n)]
    windows = []
    for g, n in sizes.items():
        windows += [window(g, 0), window(g, I, intro=_key(n - 1)), window(g, F, fixed=_key(0))]
    n = sizes[22]
    at = sorted({max(0, min(n - 1, CAP - first + d)) for d in (-2, -1, 0, 1)} | {0, n - 1})
    for i in at:
        hi, lo = _key(i)
        windows += [
            window(22, I, intro=(hi, lo)), window(22, I, intro=(hi, lo + 1)),
            window(22, F, fixed=(hi, lo)), window(22, L, last=(hi, lo)),
            window(22, I | F, intro=_key(max(i - 1, 0)), fixed=_key(min(i + 2, n - 1))),
            window(22, I | L, intro=(hi, lo), last=(hi, lo)),
            window(22, I | F | L, intro=_key(0), fixed=_key(n - 1), last=(hi, lo - 1)),
        ]
    assert len(windows) <= TILE
    return rows, windows


@pytest.mark.parametrize("total_rows", [CAP - 1, CAP, CAP + 1, 4 * CAP + 5])
def test_slice_around_the_staged_cap(dev, total_rows):
    """Rows past the first CAP of a tile's slice are probed in global memory;
    runs end on either side of that edge and one spans it."""
    arena, layout, table = tensors(*_edge_case(total_rows), dev)
    assert int(table["w_rend"].max()) - int(table["w_rbeg"].min()) == total_rows
    got = _check(arena, layout, table)
    spans = torch.bincount(got & 0xFFFFFFFF)
    assert int(spans.max()) == max(600, total_rows - 600)  # a window without bounds


def test_empty_runs_first_and_last_in_a_tile(dev):
    """Windows of groups without an estate row at both ends of two tiles."""
    rows = [row(g, *_key(i)) for g in (10, 30) for i in range(7)]
    some = []
    for g, before, after in ((10, 5, 20), (30, 25, 40)):
        some += [window(before, 0)]
        some += [window(g, (0, I, F, I | F)[w % 4], intro=_key(w % 7), fixed=_key(6))
                 for w in range(TILE - 2)]
        some += [window(after, I, intro=_key(0))]
    arena, layout, table = tensors(rows, some, dev)
    empty = (table["w_rbeg"] == table["w_rend"]).cpu()
    assert empty.numel() == 2 * TILE
    assert empty[[0, TILE - 1, TILE, 2 * TILE - 1]].all() and int(empty.sum()) == 4
    assert _check(arena, layout, table).numel() > 2 * TILE


def test_tile_of_cpu_fallback_windows(dev):
    """No lane of the first tile searches: its slice is empty, nothing is
    staged, and the second tile is not disturbed."""
    rows = [row(g, *_key(i)) for g in (10, 30) for i in range(9)]
    windows = [window(10, I | WF_CPU_FALLBACK, intro=_key(0)) for _ in range(TILE)]
    windows += [window(30, 0), window(30, I, intro=_key(4))]
    arena, layout, table = tensors(rows, windows, dev)
    got = _check(arena, layout, table)
    assert got.numel() == 9 + 5
    assert int((got & 0xFFFFFFFF).min()) == TILE


def test_waves_with_one_lane_or_all_lanes_emitting(dev):
    """Wave 0: only lane 0 emits; wave 1: only lane 63; wave 2: all 64;
    wave 3: none.  The block reserves once, from the totals of its waves."""
    rows = [row(10, *_key(i)) for i in range(5)]
    hit, miss = window(10, 0), window(10, I, intro=(9, 0))
    windows = [hit] + [miss] * 63 + [miss] * 63 + [hit] + [hit] * 64 + [miss] * 64
    arena, layout, table = tensors(rows, windows, dev)
    got = _check(arena, layout, table)
    emitting = torch.unique(got & 0xFFFFFFFF).tolist()
    assert emitting == [0, 127] + list(range(128, 192))
    assert got.numel() == 5 * 66


# ── capacity and the toggle ────────────────────────────────────────────────

@pytest.fixture(scope="module")
def overflowing(dev):
    arena, layout, table = tensors(*sized_case(257), dev)
    want = _sorted_pairs(_row_launch(arena, layout))
    assert 8 < want.numel() < ROOMY
    return arena, layout, table, want


def test_count_runs_past_capacity_and_finalize_relaunches(overflowing):
    from agentbom_amd.ops import native

    arena, _layout, table, want = overflowing
    pending = native.match_by_window_launch(arena["windows"], table, capacity=8)
    assert int(pending["out_count"].item()) == want.numel()
    assert pending["out_pairs"].numel() == 8
    assert torch.equal(_sorted_pairs(pending), want)


def test_assembly_relaunches_on_overflow(overflowing):
    from agentbom_amd.ops import native

    arena, layout, table, _want = overflowing
    full = native.assemble_findings(
        native.match_by_window_launch(arena["windows"], table, capacity=ROOMY),
        layout, PKG_BASE, {})
    grown = native.assemble_findings(
        native.match_by_window_launch(arena["windows"], table, capacity=8),
        layout, PKG_BASE, {})
    assert full["pkg_idx"].numel() > 8
    for key in ASSEMBLED:
        assert torch.equal(grown[key], full[key]), key


def test_toggle_gives_the_same_pairs(overflowing, monkeypatch):
    from agentbom_amd.ops import native

    arena, _layout, table, want = overflowing
    on = _sorted_pairs(native.match_by_window_launch(arena["windows"], table))
    monkeypatch.setenv("AGENT_BOM_MATCH_TILED", "0")
    assert not native.match_tiled_enabled()
    off = _sorted_pairs(native.match_by_window_launch(arena["windows"], table))
    assert torch.equal(on, off) and torch.equal(on, want)


# ── the split assembly ─────────────────────────────────────────────────────

def _split(arena, table, layout, ws, side, capacity=ROOMY):
    """Match and count phase on ``side``, the rest on the current stream."""
    from agentbom_amd.ops import native

    main = torch.cuda.current_stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        pending = native.match_by_window_launch(arena["windows"], table, capacity=capacity)
        state = native.assemble_findings_begin(pending, layout, ws)
    main.wait_stream(side)
    return native.assemble_findings_finish(state, PKG_BASE)


def test_split_assembly_equals_the_single_call(overflowing, dev):
    from agentbom_amd.ops import native

    arena, layout, table, _want = overflowing
    want = native.assemble_findings(
        native.match_by_window_launch(arena["windows"], table), layout, PKG_BASE, {})
    side = torch.cuda.Stream(device=dev)
    ws = {}
    first = _split(arena, table, layout, ws, side)
    assert not ws["fa_dirty"]
    second = _split(arena, table, layout, ws, side)  # the same workspace again
    third = native.assemble_findings(  # and from the single call, on the main stream
        native.match_by_window_launch(arena["windows"], table), layout, PKG_BASE, ws)
    assert want["pkg_idx"].numel() > 8
    for key in ASSEMBLED:
        for got in (first, second, third):
            assert torch.equal(got[key], want[key]), key


def test_split_assembly_overflow(overflowing, dev):
    from agentbom_amd.ops import native

    arena, layout, table, _want = overflowing
    want = native.assemble_findings(
        native.match_by_window_launch(arena["windows"], table), layout, PKG_BASE, {})
    side = torch.cuda.Stream(device=dev)
    ws = {}
    grown = _split(arena, table, layout, ws, side, capacity=8)
    assert not ws["fa_dirty"]
    again = _split(arena, table, layout, ws, side)
    for key in ASSEMBLED:
        assert torch.equal(grown[key], want[key]), key
        assert torch.equal(again[key], want[key]), key


# ── the step ───────────────────────────────────────────────────────────────

def test_step_twice_and_toggles(dev, monkeypatch):
    """EstateEngine.step() twice on one engine with the tiled kernel, then
    with the thread-per-window kernel and with the row kernel."""
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=400, n_servers=2000, n_packages=120_000,
                          name_catalog=20_000, seed=99, arena_windows=40_000)
    eng = EstateEngine(est, device=dev)
    assert eng.match_dedup is not None and eng.match_table is not None
    first, second = eng.step(), eng.step()
    monkeypatch.setenv("AGENT_BOM_MATCH_TILED", "0")
    untiled = eng.step()
    monkeypatch.delenv("AGENT_BOM_MATCH_TILED")
    monkeypatch.setenv("AGENT_BOM_MATCH_BY_WINDOW", "0")
    by_row = eng.step()
    assert first["n_findings"] > 0
    for other in (second, untiled, by_row):
        assert other["n_findings"] == first["n_findings"]
        for key, value in first.items():
            if isinstance(value, torch.Tensor):
                assert other[key].dtype == value.dtype, key
                assert torch.equal(other[key], value), key
