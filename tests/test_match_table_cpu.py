"""The row search table of the window-per-thread match
(``build_match_search_table``), built on CPU tensors and compared with brute
force, and the window search itself emulated in numpy against
``cpu_ref.match`` -- the algorithm pinned before any kernel runs."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from match_by_window_cases import (
    B63,
    G_EMPTY,
    G_FIRST,
    G_LAST,
    G_ONE,
    HAND_ROWS,
    HAND_WINDOWS,
    NO_GROUP,
    emulate_window_search,
    expected_runs,
    np_u64,
    reference_pairs,
    sized_case,
    tensors,
)

from agentbom_amd.ops.cpu_ref import PF_ENCODABLE


def _check_table(arena, layout, table):
    """Every window's run is exactly the encodable rows of its group, in
    ascending unsigned (hi, lo) order, and s_row points back at them."""
    W = arena["windows"]["flags"].numel()
    s_key, s_row = np_u64(table["s_key"]), table["s_row"].numpy()
    assert table["s_key"].dtype == torch.int64 and table["s_key"].shape == (s_row.size, 2)
    assert table["s_key"].is_contiguous()
    assert table["s_row"].dtype == torch.int32
    rbeg, rend = table["w_rbeg"].numpy(), table["w_rend"].numpy()
    assert rbeg.shape == rend.shape == (W,)
    runs = expected_runs(arena, layout)
    group_off = arena["group_off"].numpy().view(np.uint32)
    u_hi, u_lo = np_u64(layout["u_hi"]), np_u64(layout["u_lo"])
    covered = 0
    for g, want in enumerate(runs):
        for w in range(int(group_off[g]), int(group_off[g + 1])):
            assert s_row[rbeg[w]:rend[w]].tolist() == want, (g, w)
        if not want:
            continue
        b, e = int(rbeg[group_off[g]]), int(rend[group_off[g]])
        covered += e - b
        keys = [(int(h), int(l)) for h, l in s_key[b:e]]
        assert keys == sorted(keys)
        assert keys == [(int(u_hi[r]), int(u_lo[r])) for r in want]
    # nothing but those runs: no row without a group, none that is not encodable
    assert covered == s_row.size
    flags = layout["u_flags"].numpy()
    assert all(flags[r] & PF_ENCODABLE for r in s_row)
    return runs


@pytest.fixture(scope="module")
def hand():
    return tensors(HAND_ROWS, HAND_WINDOWS)


def _group_index(arena, key):
    return np_u64(arena["group_keys"]).tolist().index(key)


def test_hand_built_table(hand):
    arena, layout, table = hand
    runs = _check_table(arena, layout, table)
    G = arena["group_keys"].numel()
    assert _group_index(arena, G_FIRST) == 0 and _group_index(arena, G_LAST) == G - 1
    assert len(runs[0]) == 16 and len(runs[G - 1]) == 2       # first and last arena group
    assert runs[_group_index(arena, G_EMPTY)] == []           # a group with no estate row
    assert len(runs[_group_index(arena, G_ONE)]) == 1         # one row
    # an estate name with no group, and the row that is not encodable: absent
    gk, flags = np_u64(layout["u_gk"]), layout["u_flags"].numpy()
    present = set(table["s_row"].tolist())
    absent = set(range(gk.size)) - present
    assert {int(r) for r in np.nonzero(gk == NO_GROUP)[0]} <= absent
    assert sum(1 for r in absent if gk[r] == G_FIRST and flags[r] == 0) == 1
    # two rows with equal key and different flags sit side by side
    hi, lo = np_u64(layout["u_hi"]), np_u64(layout["u_lo"])
    twins = [r for r in runs[0] if (hi[r], lo[r]) == (1, 20)]
    assert len(twins) == 2 and flags[twins[0]] != flags[twins[1]]
    at = runs[0].index(twins[0])
    assert runs[0][at:at + 2] == twins


def test_bit_63_orders_as_unsigned(hand):
    """Keys with bit 63 set in lo, or in hi, come after those with it clear;
    torch's signed order, which the layout itself uses, puts them first."""
    arena, layout, table = hand
    b, e = int(table["w_rbeg"][0]), int(table["w_rend"][0])
    keys = [(int(h), int(l)) for h, l in np_u64(table["s_key"])[b:e]]
    assert keys.index((1, 50)) < keys.index((1, B63)) < keys.index((1, B63 | 5))
    assert keys.index((2, 11)) < keys.index((B63 - 1, 3)) < keys.index((B63, 0))
    in_group = np_u64(layout["u_gk"]) == G_FIRST
    layout_order = [(int(h), int(l)) for h, l in zip(np_u64(layout["u_hi"])[in_group],
                                                     np_u64(layout["u_lo"])[in_group])]
    assert layout_order != sorted(layout_order)


def test_hand_built_search_equals_cpu_ref(hand):
    arena, layout, table = hand
    want = reference_pairs(arena, layout)
    assert len(want) > 60
    assert emulate_window_search(arena, table) == want


@pytest.mark.parametrize("n_windows", [1, 257])
def test_sized_groups(n_windows):
    arena, layout, table = tensors(*sized_case(n_windows))
    _check_table(arena, layout, table)
    want = reference_pairs(arena, layout)
    assert len(want) >= 300
    assert emulate_window_search(arena, table) == want


@pytest.fixture(scope="module")
def seeded():
    """The estate of tests/test_finding_layout.py."""
    from agentbom_amd.graph.gpu_engine import build_dedup_match_layout, build_match_search_table
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=50, n_servers=200, n_packages=5000,
                          name_catalog=800, seed=3, arena_windows=1600)
    arena = est.arena.to_torch(torch.device("cpu"))
    cols = [torch.from_numpy(a.view(np.int64)) for a in
            (est.pkg_name_id, est.pkg_key_hi, est.pkg_key_lo)]
    layout = build_dedup_match_layout(torch, arena, *cols, torch.from_numpy(est.pkg_flags))
    assert layout is not None
    return arena, layout, build_match_search_table(torch, arena, layout)


def test_seeded_estate_table(seeded):
    arena, layout, table = seeded
    runs = _check_table(arena, layout, table)
    assert sum(1 for r in runs if r) > 10 and any(not r for r in runs)


def test_seeded_estate_search_equals_cpu_ref(seeded):
    arena, layout, table = seeded
    want = reference_pairs(arena, layout)
    assert want  # the comparison is not vacuous
    assert emulate_window_search(arena, table) == want


def test_layout_is_left_as_it_was(seeded):
    """The table is built beside the layout, not into it."""
    _arena, layout, _table = seeded
    assert set(layout) == {"u_gk", "u_hi", "u_lo", "u_flags", "run_off", "perm2", "row_of",
                           "u_ranges", "heavy_order"}
