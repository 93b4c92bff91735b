"""What the block-tiled window match (ops/csrc/match.hip,
``match_by_window_tiled_kernel``) takes from the search table, and its tile
logic emulated in numpy: the row slice of a tile, staged versus fallback
probes and the per-block reservation, against ``cpu_ref.match`` -- every
branch of the kernel without a GPU."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from match_by_window_cases import (
    HAND_ROWS,
    HAND_WINDOWS,
    np_u64,
    reference_pairs,
    sized_case,
    tensors,
    windows_np,
)

from agentbom_amd.ops.cpu_ref import (
    WF_CPU_FALLBACK,
    WF_HAS_FIXED,
    WF_HAS_INTRO,
    WF_HAS_LAST,
    WF_UNFIXED_SUPPRESSED,
)


@pytest.fixture(scope="module")
def hand():
    return tensors(HAND_ROWS, HAND_WINDOWS)


@pytest.fixture(scope="module")
def sized():
    return tensors(*sized_case(257))


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


CASES = ("hand", "sized", "seeded")


@pytest.mark.parametrize("case", CASES)
def test_runs_ascend_with_the_window_index(case, request):
    """Windows are stored group by group and the runs follow the groups, so
    the rows a tile of consecutive windows searches are one contiguous slice.
    The kernel's speed rests on this, its results do not."""
    _arena, _layout, table = request.getfixturevalue(case)
    rbeg = table["w_rbeg"].numpy().astype(np.int64)
    rend = table["w_rend"].numpy().astype(np.int64)
    assert rbeg.size > 0
    assert (np.diff(rbeg) >= 0).all()
    assert (np.diff(rend) >= 0).all()
    assert (rbeg <= rend).all()
    assert rend.max() <= table["s_row"].numel()


def emulate_tiled(arena, table, tile: int, cap: int, wave: int = 2, capacity=None):
    """The tiled kernel step by step: per tile the row slice of the lanes
    that search, ``cap`` rows of it staged, probes inside the staged rows read
    the copy and the others the table, prefix sums per wave of ``wave`` lanes
    and one reservation per tile from the waves' totals.  Returns (pairs as a
    set, final count, staged probes, fallback probes, out buffer)."""
    win = windows_np(arena)
    key = np_u64(table["s_key"]).reshape(-1, 2)
    keys = [(int(h) << 64) | int(l) for h, l in key]
    s_row = table["s_row"].numpy()
    rbeg, rend = table["w_rbeg"].numpy(), table["w_rend"].numpy()
    W = rbeg.size
    probes = {"staged": 0, "fallback": 0}
    count = 0
    out = {}

    for w0 in range(0, W, tile):
        lanes = range(w0, min(w0 + tile, W))
        searches = {w: not (win["flags"][w] & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED))
                    and rbeg[w] < rend[w] for w in lanes}
        slo = min([int(rbeg[w]) for w in lanes if searches[w]], default=0xFFFFFFFF)
        shi = max([int(rend[w]) for w in lanes if searches[w]], default=0)
        nst = min(shi - slo, cap) if slo < shi else 0
        staged = keys[slo:slo + nst]  # the block's copy

        def bound(lo, hi, b, after):
            while lo < hi:
                mid = lo + (hi - lo) // 2
                at = (mid - slo) & 0xFFFFFFFF
                if at < nst:
                    k = staged[at]
                    probes["staged"] += 1
                else:
                    k = keys[mid]
                    probes["fallback"] += 1
                if (k <= b) if after else (k < b):
                    lo = mid + 1
                else:
                    hi = mid
            return lo

        runs = []
        for w in lanes:
            n, begin = 0, int(rbeg[w])
            if searches[w]:
                f, end = int(win["flags"][w]), int(rend[w])
                if f & WF_HAS_INTRO:
                    begin = bound(begin, end,
                                  (int(win["intro_hi"][w]) << 64) | int(win["intro_lo"][w]), False)
                if f & WF_HAS_FIXED:
                    end = bound(begin, end,
                                (int(win["fixed_hi"][w]) << 64) | int(win["fixed_lo"][w]), False)
                if f & WF_HAS_LAST:
                    end = bound(begin, end,
                                (int(win["last_hi"][w]) << 64) | int(win["last_lo"][w]), True)
                n = max(end - begin, 0)
            runs.append((w, begin, n))
        # lanes past the last window of a partial tile hold n = 0
        runs += [(None, 0, 0)] * (tile - len(runs))
        wave_n = [sum(n for _w, _b, n in runs[v0:v0 + wave]) for v0 in range(0, tile, wave)]
        if sum(wave_n) == 0:
            continue
        block_base, count = count, count + sum(wave_n)  # the one atomic
        for v, v0 in enumerate(range(0, tile, wave)):
            lanes_v = runs[v0:v0 + wave]
            incl = np.cumsum([n for _w, _b, n in lanes_v])
            for (w, begin, n), upto in zip(lanes_v, incl):
                base = block_base + sum(wave_n[:v]) + int(upto) - n
                for j in range(n):
                    if capacity is None or base + j < capacity:
                        assert base + j not in out
                        out[base + j] = (int(s_row[begin + j]), w)
    return set(out.values()), count, probes["staged"], probes["fallback"], out


@pytest.mark.parametrize("tile", [4, 256])
@pytest.mark.parametrize("case", CASES)
def test_tile_logic_equals_cpu_ref(case, tile, request):
    arena, layout, table = request.getfixturevalue(case)
    want = reference_pairs(arena, layout)
    assert want
    pairs, count, staged, fallback, out = emulate_tiled(arena, table, tile=tile, cap=3)
    assert pairs == want
    assert count == len(want) == len(out)
    assert sorted(out) == list(range(count))  # the reservations tile the buffer
    # a cap of 3 rows leaves most of a slice outside: both probe paths run
    assert staged > 0 and fallback > 0


def test_whole_slice_staged_needs_no_fallback(hand):
    arena, layout, table = hand
    pairs, _count, staged, fallback, _out = emulate_tiled(arena, table, tile=256, cap=1024)
    assert pairs == reference_pairs(arena, layout)
    assert staged > 0 and fallback == 0


def test_count_runs_past_the_capacity(sized):
    arena, layout, table = sized
    want = reference_pairs(arena, layout)
    pairs, count, _s, _f, out = emulate_tiled(arena, table, tile=256, cap=3, capacity=8)
    assert count == len(want) > 8
    assert sorted(out) == list(range(8)) and pairs <= want
