"""The window-per-thread match kernel (ops/csrc/match.hip,
``match_by_window_kernel``) against the row kernel: on the same distinct
rows both must give the same (row, window) pairs, as sorted sets."""

from __future__ import annotations

import pytest
import torch

from match_by_window_cases import (
    HAND_ROWS,
    HAND_WINDOWS,
    reference_pairs,
    sized_case,
    tensors,
)

pytestmark = pytest.mark.gpu

PKG_BASE = 1_000_003
ROOMY = 1 << 17  # a pair capacity no case here can fill: 257 windows x 300 rows < 2^17
ASSEMBLED = ("pkg_idx", "win_idx", "pkg_nodes", "pos", "uniq_pkgs", "uniq_pkgs32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


def _row_launch(arena, layout, capacity=None):
    from agentbom_amd.ops import native

    return native.match_launch(
        layout["u_gk"], layout["u_hi"], layout["u_lo"], layout["u_flags"],
        arena["group_keys"], arena["group_off"], arena["windows"],
        pkg_win_range=layout["u_ranges"], order=layout["heavy_order"], capacity=capacity)


def _sorted_pairs(pending):
    from agentbom_amd.ops import native

    rows, wins = native.match_finalize(pending, sort=True)
    return (rows << 32) | wins


def _assert_same_pairs(arena, layout, table):
    from agentbom_amd.ops import native

    got = _sorted_pairs(native.match_by_window_launch(arena["windows"], table))
    want = _sorted_pairs(_row_launch(arena, layout))
    assert torch.equal(got, want)
    return got


def test_every_window_form(dev):
    """The hand-built arena: each window form, rows on each bound, rows that
    differ only in lo, keys with bit 63 set, a row that is not encodable
    inside a window, groups without rows and rows without a group."""
    arena, layout, table = tensors(HAND_ROWS, HAND_WINDOWS, dev)
    got = _assert_same_pairs(arena, layout, table)
    want = reference_pairs(arena, layout)
    assert {(int(p) >> 32, int(p) & 0xFFFFFFFF) for p in got.tolist()} == want


@pytest.mark.parametrize("n_windows", [1, 255, 256, 257])
def test_group_sizes_and_grid_edge(dev, n_windows):
    """Groups of 1, 63, 64, 65 and 300 rows; window 0 emits all 300 rows of
    its group; the window count sits on either side of one block."""
    arena, layout, table = tensors(*sized_case(n_windows), dev)
    assert arena["windows"]["flags"].numel() == n_windows
    got = _assert_same_pairs(arena, layout, table)
    assert got.numel() >= 300
    spans = torch.bincount(got & 0xFFFFFFFF, minlength=n_windows)
    assert int(spans.max()) == 300


@pytest.fixture(scope="module")
def overflowing(dev):
    arena, layout, table = tensors(*sized_case(257), dev)
    want = _sorted_pairs(_row_launch(arena, layout, capacity=ROOMY))
    assert 8 < want.numel() < ROOMY
    return arena, layout, table, want


@pytest.fixture
def by_window_only(monkeypatch):
    """Counts the by-window launches and forbids the row kernel."""
    from agentbom_amd.ops import native

    launches = []
    real = native.match_by_window_launch

    def counted(*args, **kw):
        launches.append(kw.get("capacity"))
        return real(*args, **kw)

    def forbidden(*_args, **_kw):
        raise AssertionError("the row kernel was launched")

    monkeypatch.setattr(native, "match_by_window_launch", counted)
    monkeypatch.setattr(native, "match_launch", forbidden)
    return launches


def test_overflow_relaunches_through_finalize(overflowing, by_window_only):
    from agentbom_amd.ops import native

    arena, _layout, table, want = overflowing
    pending = native.match_by_window_launch(arena["windows"], table, capacity=8)
    assert int(pending["out_count"].item()) == want.numel()  # counted past the capacity
    assert torch.equal(_sorted_pairs(pending), want)
    assert len(by_window_only) == 2 and by_window_only[1] > want.numel()


def test_overflow_relaunches_through_assembly(overflowing, by_window_only):
    from agentbom_amd.ops import native

    arena, layout, table, _want = overflowing
    full = native.assemble_findings(
        native.match_by_window_launch(arena["windows"], table, capacity=ROOMY),
        layout, PKG_BASE, {})
    assert by_window_only == [ROOMY]
    grown = native.assemble_findings(
        native.match_by_window_launch(arena["windows"], table, capacity=8),
        layout, PKG_BASE, {})
    assert by_window_only[:2] == [ROOMY, 8] and len(by_window_only) == 3
    assert by_window_only[2] > 8
    assert full["pkg_idx"].numel() > 8
    for key in ASSEMBLED:
        assert torch.equal(grown[key], full[key]), key


def test_assembly_equals_row_kernel(overflowing):
    from agentbom_amd.ops import native

    arena, layout, table, _want = overflowing
    got = native.assemble_findings(
        native.match_by_window_launch(arena["windows"], table), layout, PKG_BASE, {})
    want = native.assemble_findings(_row_launch(arena, layout), layout, PKG_BASE, {})
    for key in ASSEMBLED:
        assert torch.equal(got[key], want[key]), key


def test_step_toggle(dev, monkeypatch):
    """EstateEngine.step() with the window kernel and with the row kernel:
    every output tensor equal, the same number of findings."""
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.ops import native
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=400, n_servers=2000, n_packages=120_000,
                          name_catalog=20_000, seed=99, arena_windows=40_000)
    eng = EstateEngine(est, device=dev)
    assert eng.match_dedup is not None and eng.match_table is not None
    launches = {"window": 0, "row": 0}
    for name, attr in (("window", "match_by_window_launch"), ("row", "match_launch")):
        def counted(*args, _real=getattr(native, attr), _name=name, **kw):
            launches[_name] += 1
            return _real(*args, **kw)
        monkeypatch.setattr(native, attr, counted)

    monkeypatch.setenv("AGENT_BOM_MATCH_BY_WINDOW", "1")
    on = eng.step()
    assert launches == {"window": 1, "row": 0}
    monkeypatch.delenv("AGENT_BOM_MATCH_BY_WINDOW")
    default = eng.step()
    assert launches == {"window": 2, "row": 0}
    monkeypatch.setenv("AGENT_BOM_MATCH_BY_WINDOW", "0")
    off = eng.step()
    assert launches == {"window": 2, "row": 1}

    assert on["n_findings"] == default["n_findings"] == off["n_findings"] > 0
    for key, value in off.items():
        if isinstance(value, torch.Tensor):
            assert on[key].dtype == value.dtype, key
            assert torch.equal(on[key], value), key
            assert torch.equal(default[key], value), key
