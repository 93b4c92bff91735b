"""Native finding assembly (ops/csrc/findings.hip) vs the torch op chain.

The oracle is ``expand_dedup_matches`` on the same inputs plus
``unique_consecutive`` / ``searchsorted`` for the unique packages and the
per-finding positions; every output array must be exactly equal, dtype
included.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PKG_BASE = 1_000_003
KEYS = ("pkg_idx", "win_idx", "pkg_nodes", "pos", "uniq_pkgs", "uniq_pkgs32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layout_from_rows(row_of_pkg, U, dev):
    """Layout (run_off, perm2, row_of) of packages assigned to rows."""
    from agentbom_amd.graph.gpu_engine import row_of_from_runs

    row_of_pkg = torch.as_tensor(row_of_pkg, dtype=torch.int64)
    perm2 = torch.argsort(row_of_pkg, stable=True)
    counts = torch.bincount(row_of_pkg, minlength=U)
    run_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    layout = {"run_off": run_off.to(dev), "perm2": perm2.to(dev)}
    layout["row_of"] = row_of_from_runs(torch, layout["run_off"], layout["perm2"])
    return layout


def _random_layout(rng, P, U, dev):
    return _layout_from_rows(rng.integers(0, U, P), U, dev)


def _distinct_pairs(rows, wins):
    """int64 (row << 32 | win), duplicates dropped, in ascending order."""
    rows = torch.as_tensor(np.asarray(rows), dtype=torch.int64)
    wins = torch.as_tensor(np.asarray(wins), dtype=torch.int64)
    return torch.unique((rows << 32) | wins)


def _pending(pairs, dev, spare: int = 0):
    """What native.match_launch hands over: pair buffer, device count, capacity."""
    m = pairs.numel()
    buf = torch.full((m + spare,), -1, dtype=torch.int64)
    buf[:m] = pairs
    return {"out_pairs": buf.to(dev),
            "out_count": torch.tensor([m], dtype=torch.int32, device=dev),
            "cap": m + spare}


def _oracle(layout, pairs, dev):
    from agentbom_amd.graph.gpu_engine import expand_dedup_matches

    p = pairs.to(dev)
    pkg, win = expand_dedup_matches(torch, layout, p >> 32, p & 0xFFFFFFFF)
    nodes = pkg + PKG_BASE
    uniq = torch.unique_consecutive(nodes)
    return {"pkg_idx": pkg, "win_idx": win, "pkg_nodes": nodes,
            "pos": torch.searchsorted(uniq, nodes),
            "uniq_pkgs": uniq, "uniq_pkgs32": uniq.to(torch.int32)}


def _assemble(layout, pairs, dev, ws=None, spare: int = 0):
    from agentbom_amd.ops import native

    return native.assemble_findings(_pending(pairs, dev, spare), layout, PKG_BASE,
                                    {} if ws is None else ws)


def _assert_same(got, want):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype, key
        assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_layouts(dev, seed):
    rng = np.random.default_rng(seed)
    layout = _random_layout(rng, 500, 60, dev)
    pairs = _distinct_pairs(rng.integers(0, 60, 80), rng.integers(0, 1000, 80))
    _assert_same(_assemble(layout, pairs, dev), _oracle(layout, pairs, dev))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000, 40_000])
def test_word_edges(dev, P):
    """Matched packages at bit 0 and bit 63 of a bitmap word and at index
    P-1; 40,000 packages span three blocks of bitmap words."""
    rng = np.random.default_rng(P)
    U = max(1, P // 3)
    rows = rng.integers(0, U, P)
    layout = _layout_from_rows(rows, U, dev)
    edge_pkgs = {0, P - 1, min(63, P - 1), min(64, P - 1), (P - 1) // 64 * 64}
    edge_rows = [int(rows[p]) for p in sorted(edge_pkgs)]
    extra = rng.integers(0, U, max(4, P // 12))
    match_rows = np.concatenate([edge_rows, edge_rows, extra])
    pairs = _distinct_pairs(match_rows, rng.integers(0, 50, match_rows.size))
    got = _assemble(layout, pairs, dev)
    _assert_same(got, _oracle(layout, pairs, dev))
    found = set(got["pkg_idx"].tolist())
    assert edge_pkgs <= found


@pytest.mark.parametrize("spare", [0, 16])
def test_no_matches(dev, spare):
    layout = _random_layout(np.random.default_rng(0), 100, 10, dev)
    got = _assemble(layout, torch.empty(0, dtype=torch.int64), dev, spare=spare)
    for key in KEYS:
        assert got[key].numel() == 0
        assert got[key].dtype == (torch.int32 if key == "uniq_pkgs32" else torch.int64)
        assert got[key].device.type == "cuda"


def test_empty_runs_contribute_nothing(dev):
    layout = {"run_off": torch.tensor([0, 2, 2, 5], device=dev),
              "perm2": torch.tensor([4, 1, 0, 3, 2], device=dev)}
    from agentbom_amd.graph.gpu_engine import row_of_from_runs

    layout["row_of"] = row_of_from_runs(torch, layout["run_off"], layout["perm2"])
    pairs = _distinct_pairs([0, 1, 2, 2], [7, 9, 3, 8])
    got = _assemble(layout, pairs, dev)
    _assert_same(got, _oracle(layout, pairs, dev))
    assert 9 not in got["win_idx"].tolist()
    assert got["pkg_idx"].numel() == 2 * 1 + 3 * 2
    # only an empty row matched: nothing at all
    only_empty = _distinct_pairs([1], [9])
    assert _assemble(layout, only_empty, dev)["pkg_idx"].numel() == 0


def test_seventy_matches_and_a_run_of_5000(dev):
    """More matches on a row than a wave has lanes, and a run far longer than
    one lane should walk: row 0 holds 5,000 of the 5,200 packages (every
    index not divisible by 26) and matches 70 windows; row 1 (3 packages)
    matches 70 others."""
    P, U = 5200, 40
    rng = np.random.default_rng(7)
    rows = np.zeros(P, dtype=np.int64)
    rest = np.arange(0, P, 26)
    rows[rest] = rng.integers(2, U, rest.size)
    rows[rest[:3]] = 1
    layout = _layout_from_rows(rows, U, dev)
    assert int(layout["run_off"][1] - layout["run_off"][0]) == 5000
    wins = rng.permutation(400)
    match_rows = np.concatenate([np.zeros(70), np.ones(70), rng.integers(2, U, 30)])
    pairs = _distinct_pairs(match_rows.astype(np.int64), wins[:170])
    pairs = pairs[torch.from_numpy(rng.permutation(pairs.numel()))]
    got = _assemble(layout, pairs, dev)
    assert got["pkg_idx"].numel() >= 70 * 5000
    _assert_same(got, _oracle(layout, pairs, dev))


def test_arrival_order_does_not_leak(dev):
    rng = np.random.default_rng(11)
    layout = _random_layout(rng, 3000, 200, dev)
    pairs = _distinct_pairs(rng.integers(0, 200, 600), rng.integers(0, 40, 600))
    base = _assemble(layout, pairs, dev)
    _assert_same(base, _oracle(layout, pairs, dev))
    for _ in range(3):
        shuffled = pairs[torch.from_numpy(rng.permutation(pairs.numel()))]
        _assert_same(_assemble(layout, shuffled, dev), base)


def test_workspace_reuse(dev):
    """A second call with other matches on the same workspace equals its own
    oracle: no stale bitmap bit, count or tail survives a call."""
    rng = np.random.default_rng(5)
    layout = _random_layout(rng, 2000, 150, dev)
    ws: dict = {}
    for m in (300, 20, 0, 500):
        pairs = _distinct_pairs(rng.integers(0, 150, m), rng.integers(0, 30, m))
        _assert_same(_assemble(layout, pairs, dev, ws=ws, spare=8),
                     _oracle(layout, pairs, dev))
        assert not ws["fa_dirty"]
        for key in ("fa_bitmap", "fa_row_cnt", "fa_row_tail"):
            assert not bool(ws[key].any()), key


def test_dirty_workspace_is_cleared(dev):
    """A call that died between count and emit leaves the workspace flagged;
    the next call must not trust its contents."""
    rng = np.random.default_rng(9)
    layout = _random_layout(rng, 2000, 150, dev)
    ws: dict = {}
    pairs = _distinct_pairs(rng.integers(0, 150, 200), rng.integers(0, 30, 200))
    _assemble(layout, pairs, dev, ws=ws)
    ws["fa_bitmap"].fill_(-1)
    ws["fa_row_cnt"].fill_(3)
    ws["fa_row_tail"].fill_(1)
    ws["fa_dirty"] = True
    _assert_same(_assemble(layout, pairs, dev, ws=ws), _oracle(layout, pairs, dev))


# ── engine level ───────────────────────────────────────────────────────────

STEP_KEYS = ("pkg_idx", "win_idx", "scores", "order", "n_agents", "n_creds", "n_tools")


@pytest.fixture(scope="module")
def engine(dev):
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=400, n_servers=2000, n_packages=120_000,
                          name_catalog=20_000, seed=99, arena_windows=40_000)
    eng = EstateEngine(est, device=str(dev))
    assert eng.match_dedup is not None
    return eng


def test_step_native_equals_torch_chain(engine, monkeypatch):
    monkeypatch.setenv("AGENT_BOM_FINDINGS_NATIVE", "1")
    native_res = engine.step()
    again = engine.step()  # steady state: the workspace has been used once
    monkeypatch.setenv("AGENT_BOM_FINDINGS_NATIVE", "0")
    chain_res = engine.step()
    assert native_res["n_findings"] == chain_res["n_findings"] > 0
    for key in STEP_KEYS:
        assert native_res[key].dtype == chain_res[key].dtype, key
        assert torch.equal(native_res[key], chain_res[key]), key
        assert torch.equal(again[key], chain_res[key]), key


def test_capacity_overflow_relaunches(engine):
    """A pair buffer too small for the matches: the assembly relaunches the
    match with a grown buffer, like match_finalize."""
    from agentbom_amd.graph.gpu_engine import expand_dedup_matches
    from agentbom_amd.ops import native

    dd = engine.match_dedup

    def launch(capacity):
        return native.match_launch(
            dd["u_gk"], dd["u_hi"], dd["u_lo"], dd["u_flags"],
            engine.arena["group_keys"], engine.arena["group_off"],
            engine.arena["windows"], pkg_win_range=dd["u_ranges"],
            order=dd["heavy_order"], capacity=capacity)

    sp, sw = native.match_finalize(launch(None), sort=False)
    assert sp.numel() > 64
    pkg, win = expand_dedup_matches(torch, dd, sp, sw)
    got = native.assemble_findings(launch(64), dd, engine.estate.pkg_base, {})
    assert torch.equal(got["pkg_idx"], pkg)
    assert torch.equal(got["win_idx"], win)
