"""Shared inputs and oracles of the window-per-thread match tests
(tests/test_match_table_cpu.py, tests/test_match_by_window_gpu.py).

A case is an advisory arena plus package rows, both written as plain Python
integers (u64 values, so bit 63 can be set); ``tensors`` turns a case into
what the engine holds: the arena dict, the dedup layout of the rows and the
row search table.  The oracles are brute force over the layout's columns.
"""

from __future__ import annotations

import numpy as np
import torch

from agentbom_amd.db.arena import build_arena_from_columns
from agentbom_amd.graph.gpu_engine import build_dedup_match_layout, build_match_search_table
from agentbom_amd.ops import cpu_ref
from agentbom_amd.ops.cpu_ref import (
    PF_ENCODABLE,
    WF_CPU_FALLBACK,
    WF_HAS_FIXED,
    WF_HAS_INTRO,
    WF_HAS_LAST,
    WF_UNFIXED_SUPPRESSED,
)

B63 = 1 << 63
TOP = (1 << 64) - 1
I, F, L = WF_HAS_INTRO, WF_HAS_FIXED, WF_HAS_LAST
Z = (0, 0)


def window(group, flags, intro=Z, fixed=Z, last=Z):
    return (group, flags, intro, fixed, last)


def row(group, hi, lo, flags=PF_ENCODABLE):
    return (group, hi, lo, flags)


# ── the hand-built case ────────────────────────────────────────────────────

G_FIRST, G_EMPTY, G_ONE, G_HIGH, G_LAST = 5, 100, 0x7000_0000_0000_0001, B63 | 9, TOP - 15
NO_GROUP = 77  # an estate name the arena does not know

HAND_ROWS = [
    # G_FIRST: the rows every window form is tried on
    row(G_FIRST, 1, 10), row(G_FIRST, 1, 20), row(G_FIRST, 1, 20, PF_ENCODABLE | 2),
    row(G_FIRST, 1, 21), row(G_FIRST, 1, 30), row(G_FIRST, 1, 40), row(G_FIRST, 1, 50),
    row(G_FIRST, 1, 25, 0),          # not encodable, inside most windows
    row(G_FIRST, 1, 7), row(G_FIRST, 1, B63), row(G_FIRST, 1, B63 | 5),   # bit 63 of lo
    row(G_FIRST, 1, TOP),
    row(G_FIRST, 2, 10), row(G_FIRST, 2, 11),                             # differ in lo only
    row(G_FIRST, B63 - 1, 3), row(G_FIRST, B63, 0), row(G_FIRST, B63 | 1, 3),  # bit 63 of hi
    row(G_ONE, 4, 4),
    row(G_HIGH, 3, 1), row(G_HIGH, 3, B63 | 1),
    row(G_LAST, 9, 9), row(G_LAST, 9, 10),
    row(NO_GROUP, 1, 20), row(NO_GROUP, 1, 30),
]

HAND_WINDOWS = [
    window(G_FIRST, 0),                                        # no bound at all
    window(G_FIRST, F, fixed=(1, 30)),                         # no intro
    window(G_FIRST, I, intro=(1, 20)),                         # intro only, on a row
    window(G_FIRST, I | F, intro=(1, 20), fixed=(1, 40)),      # rows on both bounds
    window(G_FIRST, I | L, intro=(1, 20), last=(1, 40)),
    window(G_FIRST, I | F | L, intro=(1, 10), fixed=(1, 30), last=(1, 50)),  # fixed tighter
    window(G_FIRST, F | L, fixed=(1, 50), last=(1, 30)),       # last tighter
    window(G_FIRST, F | L, fixed=(1, 30), last=(1, 30)),       # same key: fixed excludes it
    window(G_FIRST, I | F | WF_CPU_FALLBACK, intro=(1, 10), fixed=(1, 50)),
    window(G_FIRST, I | F | WF_UNFIXED_SUPPRESSED, intro=(1, 10), fixed=(1, 50)),
    window(G_FIRST, I | F, intro=(1, 40), fixed=(1, 20)),      # inverted: nothing
    window(G_FIRST, I, intro=(B63 | 2, 0)),                    # above every row
    window(G_FIRST, F, fixed=(0, 5)),                          # below every row
    window(G_FIRST, I | F, intro=(1, 22), fixed=(1, 29)),      # only the unencodable row
    window(G_FIRST, I, intro=(1, B63)),                        # bit 63 of lo
    window(G_FIRST, F, fixed=(1, B63)),
    window(G_FIRST, I | L, intro=(1, 8), last=(1, B63)),
    window(G_FIRST, I | L, intro=(2, 11), last=(2, 11)),       # rows differing in lo
    window(G_FIRST, I, intro=(B63, 0)),                        # bit 63 of hi
    window(G_FIRST, L, last=(B63 - 1, TOP)),
    window(G_FIRST, I | F, intro=(B63 - 1, 3), fixed=(B63 | 1, 3)),
    window(G_EMPTY, 0), window(G_EMPTY, I, intro=(1, 1)),      # group without estate row
    window(G_ONE, 0), window(G_ONE, I | F, intro=(4, 4), fixed=(4, 5)),
    window(G_ONE, F, fixed=(4, 4)), window(G_ONE, L, last=(4, 4)),
    window(G_HIGH, I, intro=(3, 2)), window(G_HIGH, F, fixed=(3, 2)),
    window(G_LAST, L, last=(9, 9)), window(G_LAST, I, intro=(9, 10)),
]


# ── groups of 1, 63, 64, 65 and 300 rows, any number of windows ────────────

SIZED_GROUPS = {11: 1, 12: 63, 13: 64, 14: 65, 15: 300}
BIG_GROUP = 15


def _sized_key(i):
    """Key of row i of a sized group, distinct per i: every seventh row has
    bit 63 of lo set, rows from 40 on a hi word with bit 63 set."""
    hi = 1 if i < 40 else B63 | 1
    lo = 3 * i + 1 + (B63 if i % 7 == 0 else 0)
    return hi, lo


def sized_case(n_windows: int, seed: int = 0):
    """(rows, windows): window 0 spans the whole 300-row group; the others
    take every form in turn, with bounds on and between the rows' keys."""
    rng = np.random.default_rng([seed, n_windows])
    rows = [row(g, *_sized_key(i)) for g, n in SIZED_GROUPS.items() for i in range(n)]
    by_group = {g: sorted(_sized_key(i) for i in range(n)) for g, n in SIZED_GROUPS.items()}
    forms = [0, I, F, L, I | F, I | L, F | L, I | F | L,
             I | F | WF_CPU_FALLBACK, F | WF_UNFIXED_SUPPRESSED]
    windows = [window(BIG_GROUP, 0)]
    groups = list(SIZED_GROUPS)
    for w in range(1, n_windows):
        g = groups[int(rng.integers(len(groups)))]
        keys = by_group[g]

        def bound():
            hi, lo = keys[int(rng.integers(len(keys)))]
            return hi, lo + int(rng.integers(-1, 2))  # on a row or right beside it

        a, b = sorted((bound(), bound()))
        windows.append(window(g, forms[w % len(forms)], intro=a, fixed=b, last=bound()))
    return rows, windows


# ── case -> tensors ────────────────────────────────────────────────────────

def _u64(values):
    return np.array(values, dtype=np.uint64)


def tensors(rows, windows, dev="cpu"):
    """(arena dict, layout, table) on ``dev``.  Every row is listed twice so
    the dedup layout exists (it is dropped above 90 % distinct rows)."""
    W = len(windows)
    arena = build_arena_from_columns(
        _u64([w[0] for w in windows]),
        _u64([w[2][0] for w in windows]), _u64([w[2][1] for w in windows]),
        _u64([w[3][0] for w in windows]), _u64([w[3][1] for w in windows]),
        _u64([w[4][0] for w in windows]), _u64([w[4][1] for w in windows]),
        np.array([w[1] for w in windows], dtype=np.uint8),
        np.ones(W, dtype=np.uint8), np.zeros(W, dtype=np.float32),
        np.zeros(W, dtype=np.float32), np.zeros(W, dtype=np.uint8),
    ).to_torch(torch.device(dev))
    doubled = list(rows) + list(rows)
    cols = [torch.from_numpy(_u64([r[c] for r in doubled]).view(np.int64)).to(dev)
            for c in range(3)]
    flags = torch.tensor([r[3] for r in doubled], dtype=torch.uint8, device=dev)
    layout = build_dedup_match_layout(torch, arena, *cols, flags)
    assert layout is not None
    return arena, layout, build_match_search_table(torch, arena, layout)


# ── oracles ────────────────────────────────────────────────────────────────

def np_u64(t):
    return t.cpu().numpy().view(np.uint64)


def windows_np(arena):
    return {k: (np_u64(v) if v.dtype == torch.int64 else v.cpu().numpy())
            for k, v in arena["windows"].items() if k != "packed"}


def expected_runs(arena, layout):
    """Per arena group: the layout rows a window of the group may match, as
    row ids in ascending unsigned (hi, lo, row id) order."""
    gk, hi, lo = (np_u64(layout[k]) for k in ("u_gk", "u_hi", "u_lo"))
    enc = (layout["u_flags"].cpu().numpy() & PF_ENCODABLE) != 0
    runs = []
    for key in np_u64(arena["group_keys"]):
        ids = [int(r) for r in np.nonzero((gk == key) & enc)[0]]
        runs.append(sorted(ids, key=lambda r: (int(hi[r]), int(lo[r]), r)))
    return runs


def reference_pairs(arena, layout):
    """Set of (row, window): cpu_ref.match over the layout's distinct rows."""
    rows, wins = cpu_ref.match(
        np_u64(layout["u_gk"]), np_u64(layout["u_hi"]), np_u64(layout["u_lo"]),
        layout["u_flags"].cpu().numpy(), np_u64(arena["group_keys"]),
        arena["group_off"].cpu().numpy().view(np.uint32), windows_np(arena))
    return set(zip(rows.tolist(), wins.tolist()))


def emulate_window_search(arena, table):
    """The kernel's algorithm in numpy and Python integers: per window, lower
    bounds over the run of its group, then one pair per row in between."""
    win = windows_np(arena)
    key = np_u64(table["s_key"])
    keys = [(int(h) << 64) | int(l) for h, l in key.reshape(-1, 2)]
    s_row = table["s_row"].cpu().numpy()
    rbeg, rend = table["w_rbeg"].cpu().numpy(), table["w_rend"].cpu().numpy()

    def bound(lo, hi, b, after):
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if (keys[mid] <= b) if after else (keys[mid] < b):
                lo = mid + 1
            else:
                hi = mid
        return lo

    pairs = set()
    for w, f in enumerate(win["flags"].tolist()):
        if f & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED) or rbeg[w] >= rend[w]:
            continue
        begin, end = int(rbeg[w]), int(rend[w])
        if f & WF_HAS_INTRO:
            begin = bound(begin, end, (int(win["intro_hi"][w]) << 64) | int(win["intro_lo"][w]),
                          False)
        if f & WF_HAS_FIXED:
            end = bound(begin, end, (int(win["fixed_hi"][w]) << 64) | int(win["fixed_lo"][w]),
                        False)
        if f & WF_HAS_LAST:
            end = bound(begin, end, (int(win["last_hi"][w]) << 64) | int(win["last_lo"][w]),
                        True)
        pairs.update((int(s_row[r]), w) for r in range(begin, end))
    return pairs
