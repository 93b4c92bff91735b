"""GPU estate engine: CSR residency in HBM + the blast-radius pipeline.

The estate graph (agents, servers, creds, tools, packages) is built as
forward and reverse CSR on-device (torch sort/bincount/cumsum — GPU CSR
construction) and stays resident in HBM3E.  On top of it:

- ``match()``            bulk advisory matching (ops/csrc/match.hip), one
                         thread per package row walking the windows of its
                         group (``match_kernel``).  ``step()`` matches the
                         DISTINCT rows of the dedup layout instead, with one
                         thread per advisory window binary-searching the
                         group's rows in a search table built once
                         (``build_match_search_table``,
                         ``match_by_window_tiled_kernel``, which stages the
                         rows of 256 consecutive windows in LDS;
                         AGENT_BOM_MATCH_TILED=0 probes global memory
                         instead); AGENT_BOM_MATCH_BY_WINDOW=0, or an estate
                         without a dedup layout, keeps the row kernel there
- ``dependency_reach()`` multi-source BFS from all agents (ops/csrc/bfs.hip).
                         Its dense level is a bottom-up pass over a parent
                         index (``native.bfs_parent_index``: per vertex the
                         first allowed in-edge of its reverse row, built once
                         with the CSR for the mask of the reach walk);
                         AGENT_BOM_BFS_PARENT_INDEX=0 walks the reverse rows
                         instead
- ``agent_reach()``      hop count per (target, agent) for a set of agents:
                         bit-parallel multi-source BFS, 64 agents per 64-bit
                         word (ops/csrc/reach_sets.hip)
- ``blast_counts()``     segmented joins: per-finding distinct agent/cred/
                         tool reach with CWE-impact filtering.  On the GPU
                         the matched packages are joined against a
                         per-server reach index (``build_reach_index``: each
                         server's distinct agents, creds and tools, laid out
                         once with the CSR) by the two kernels of
                         ops/csrc/blast.hip; AGENT_BOM_BLAST_INDEX=0 walks
                         the CSR rows per package instead
- ``score()``            GPU risk scoring (reference formula)
- ``step()``             full findings pipeline: match -> reach -> join ->
                         score -> rank (the bench.py timed region).  Match,
                         finding assembly and blast counts run on a side
                         stream under the reach BFS, their outputs sized
                         from the step before and checked on the device
                         (AGENT_BOM_FINDINGS_AHEAD=0 emits and counts after
                         the BFS, sized by a host read)
- ``transitive_blast()`` / ``step(blast_depth=k)`` multi-hop delegation
                         expansion over agent<->server sharing: per matched
                         package the agents first reached at hop 2..5, the
                         deepest hop and the transitive credentials, from the
                         reach index and a per-agent server index
                         (``build_agent_index``) by the two kernels of
                         ops/csrc/blast_hops.hip; packages that overflow an
                         LDS cap are recomputed by an exact join
- ``remediation_plan()`` the fix-first plan: findings grouped per (name,
                         version) item with their counts, worst severity, KEV,
                         largest fixed version and the distinct servers,
                         agents, creds and tools over every install, ranked;
                         folded and unioned by the kernels of
                         ops/csrc/remediation.hip (LDS sets per wave, a
                         bitmap pool for the zipf heads;
                         AGENT_BOM_REMEDIATION_NATIVE=0 runs an exact torch
                         join instead)
- ``toxic_combinations()`` the pattern layer: per finding the risks that
                         are critical together (creds, KEV, execute or
                         retrieval tools, a shared server, an advisory across
                         three agents) with their score, per advisory its
                         findings, packages, servers and agents, and the
                         shared servers with a write and a read tool; a
                         per-server capability table, a fold per finding and
                         the set unions of ops/csrc/toxic.hip
- ``blast_radius_query()`` batched bounded BFS for p50 query latency /
                         the /v1/graph read path
- ``pagerank()`` / ``betweenness()`` / ``choke_points()`` centrality on
                         the resident CSR (ops/csrc/centrality.hip)
- ``components()`` / ``lateral_domains()`` connected components and the
                         per-domain findings roll-up (ops/csrc/components.hip)

Replaces the reference's scan_packages hot loop + graph dict walks
(reference: src/agent_bom/scanners/package_scan.py:1307-2028,
src/agent_bom/graph/{container,dependency_reach}.py) — see SURVEY.md §2.11.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from agentbom_amd.models.blast import HOP_RISK_FACTORS
from agentbom_amd.models.cwe_impact import (
    IMPACT_CODE,
    IMPACT_CREDENTIAL_ACCESS,
    IMPACT_CODE_EXECUTION,
    IMPACT_DATA_LEAK,
    IMPACT_FILE_ACCESS,
    IMPACT_INJECTION,
    IMPACT_SSRF,
)
from agentbom_amd.scan.synth import ET_CONTAINS, ET_HAS_CRED, ET_PROVIDES_TOOL, ET_USES, SyntheticEstate

# Impact-code lookup tables (u8 code -> filter class), device-ready.
_FULL_CRED = {IMPACT_CODE[c] for c in (IMPACT_CODE_EXECUTION, IMPACT_CREDENTIAL_ACCESS,
                                       IMPACT_DATA_LEAK, IMPACT_FILE_ACCESS, IMPACT_SSRF)}
_DB_CRED = {IMPACT_CODE[IMPACT_INJECTION]}
_FULL_TOOL = _FULL_CRED
_DB_TOOL = {IMPACT_CODE[IMPACT_INJECTION]}


def _impact_lut(full: set, db: set):
    """9-entry u8 LUT: 2 = full reach, 1 = db-only, 0 = none."""
    lut = np.zeros(9, dtype=np.uint8)
    for c in full:
        lut[c] = 2
    for c in db:
        lut[c] = 1
    return lut


_SIGN64 = -0x8000000000000000  # xor flips int64 order into u64 order


def _precompute_win_ranges(torch, arena: dict, pkg_group_key_sorted):
    """(wbeg u32[P], wend u32[P]) advisory window range per package row.

    Keys are u64 hashes stored as int64 bit patterns; xor with the sign bit
    makes torch.searchsorted order match the kernel's unsigned compare."""
    gk = arena["group_keys"]
    G = gk.numel()
    P = pkg_group_key_sorted.numel()
    dev = pkg_group_key_sorted.device
    if G == 0:
        z = torch.zeros(P, dtype=torch.int32, device=dev)
        return z, z.clone()
    g = torch.searchsorted(gk ^ _SIGN64, pkg_group_key_sorted ^ _SIGN64)
    gc = g.clamp(max=G - 1)
    valid = (g < G) & (gk[gc] == pkg_group_key_sorted)
    off = arena["group_off"].to(torch.int32)
    zero = torch.zeros(P, dtype=torch.int32, device=dev)
    wbeg = torch.where(valid, off[gc], zero)
    wend = torch.where(valid, off[gc + 1], zero)
    return wbeg.contiguous(), wend.contiguous()


def row_of_from_runs(torch, run_off, perm2):
    """int32 [P]: package index -> the run (unique row) that holds it, i.e.
    ``row_of[perm2[k]] == r`` for every k in ``run_off[r]:run_off[r+1]``."""
    U = run_off.numel() - 1
    rows = torch.repeat_interleave(
        torch.arange(U, dtype=torch.int32, device=perm2.device),
        run_off[1:] - run_off[:-1])
    row_of = torch.empty(perm2.numel(), dtype=torch.int32, device=perm2.device)
    row_of[perm2] = rows
    return row_of


def build_dedup_match_layout(torch, arena: dict, gk, hi, lo, flags):
    """Dedup (group, version, flags) rows for the resident-estate match.

    Real estates install the same (name, version) on many servers; the
    reference dedups before matching (package_scan.py:1794-1816).  The
    engine mirrors that: match runs once per DISTINCT row, results fan back
    out to package rows.  Returns None when dedup would not pay
    (>90% distinct).  Layout:
      u_*       unique row columns (lexicographically sorted)
      run_off   int64 [U+1]: unique row -> its span in ``perm2``
      perm2     int64 [P]: sorted-row -> original package index
      u_ranges  precomputed window ranges for the unique rows
      row_of    int32 [P]: original package index -> its unique row (the
                inverse of perm2/run_off; read by ops/csrc/findings.hip)
    """
    P = gk.numel()
    # lexicographic stable sort by (gk, hi, lo, flags)
    idx = torch.argsort(flags.to(torch.int64), stable=True)
    for keycol in (lo, hi, gk):
        idx = idx[torch.argsort(keycol[idx], stable=True)]
    g2, h2, l2, f2 = gk[idx], hi[idx], lo[idx], flags[idx]
    neq = (g2[1:] != g2[:-1]) | (h2[1:] != h2[:-1]) | (l2[1:] != l2[:-1]) \
        | (f2[1:] != f2[:-1])
    starts = torch.cat([
        torch.zeros(1, dtype=torch.int64, device=gk.device),
        torch.nonzero(neq).flatten() + 1,
    ])
    U = starts.numel()
    if U > int(P * 0.9):
        return None
    run_off = torch.cat([starts, torch.tensor([P], dtype=torch.int64, device=gk.device)])
    layout = {
        "u_gk": g2[starts].contiguous(),
        "u_hi": h2[starts].contiguous(),
        "u_lo": l2[starts].contiguous(),
        "u_flags": f2[starts].contiguous(),
        "run_off": run_off,
        "perm2": idx,
        "row_of": row_of_from_runs(torch, run_off, idx),
    }
    layout["u_ranges"] = _precompute_win_ranges(torch, arena, layout["u_gk"])
    # Match schedule experiments (AGENT_BOM_MATCH_SCHEDULE).  They order the
    # rows of the row kernel (match_kernel) only: the window-per-thread
    # kernel visits windows, not rows, and ignores ``heavy_order``.
    #   row   — rows in window-count-descending order.  Measured SLOWER
    #           (2.44 vs 2.27 ms/step): equal-wcnt rows from DIFFERENT
    #           groups interleave, so wave lanes stop sharing a window
    #           range and the cooperative walk (64x traffic saving on
    #           zipf heads) stops firing.
    #   group — GROUPS ordered by descending total work (rows x windows),
    #           rows within a group stay adjacent and in original order:
    #           cooperative walk intact, heavy groups launch first.
    #   off   — natural lexicographic order (default).
    import os

    mode = os.environ.get("AGENT_BOM_MATCH_SCHEDULE", "off")
    if mode in ("1", "row"):
        wcnt = (layout["u_ranges"][1] - layout["u_ranges"][0]).to(torch.int64)
        layout["heavy_order"] = torch.argsort(
            -wcnt, stable=True).to(torch.int32).contiguous()
    elif mode == "group":
        wbeg, wend = layout["u_ranges"]
        wcnt = (wend - wbeg).to(torch.int64)
        # group id = first row index of the run of equal wbeg (rows are
        # lexicographically sorted, so equal-group rows are adjacent)
        wb = wbeg.to(torch.int64)
        new_grp = torch.cat([torch.ones(1, dtype=torch.bool, device=wb.device),
                             wb[1:] != wb[:-1]])
        grp = torch.cumsum(new_grp.to(torch.int64), 0) - 1
        n_grp = int(grp[-1].item()) + 1 if grp.numel() else 0
        rows_per = torch.bincount(grp, minlength=n_grp)
        gw = torch.zeros(n_grp, dtype=torch.int64, device=wb.device)
        gw.scatter_add_(0, grp, wcnt)  # total windows walked per group
        # stable argsort by descending group work -> group visit order
        grp_rank = torch.empty(n_grp, dtype=torch.int64, device=wb.device)
        grp_rank[torch.argsort(-gw, stable=True)] = torch.arange(
            n_grp, device=wb.device)
        # row key = (group rank, original row index) — one stable sort
        U = wb.numel()
        bits = max(1, (U - 1).bit_length())
        key = (grp_rank[grp] << bits) | torch.arange(U, device=wb.device)
        layout["heavy_order"] = torch.argsort(key).to(torch.int32).contiguous()
    else:
        layout["heavy_order"] = None
    return layout


def build_match_search_table(torch, arena: dict, layout: dict) -> dict:
    """Row search table of the window-per-thread match (ops/csrc/match.hip,
    ``match_by_window_kernel``): the layout's distinct rows regrouped by
    advisory group and sorted by version key, so that the rows a window
    matches are one contiguous run and two or three binary searches find it.

    Like ``pkg_win_range`` this joins estate rows to arena groups by name and
    nothing else: no version key is compared with a window bound here, every
    such test runs in the kernel in every step.  Holds the rows with
    PF_ENCODABLE set and a non-empty window range, ordered by (arena group,
    key hi, key lo, row id) with the key as unsigned 128 bits -- the layout's
    own order compares signed int64, which misplaces a key with bit 63 set in
    either word, so the order is rebuilt here with the sign bit flipped.
      s_key    int64 [R,2]: (hi, lo) bit patterns, one 16-byte probe per row
      s_row    int32 [R]: the row's index in the layout's ``u_*`` columns
      w_rbeg   int32 [W]: for every arena window the run of its group in
      w_rend   int32 [W]  ``s_*``; empty when no estate row has the name
    """
    from agentbom_amd.ops.cpu_ref import PF_ENCODABLE

    gk = arena["group_keys"]
    group_off = arena["group_off"].to(torch.int64) & 0xFFFFFFFF
    G = gk.numel()
    dev = gk.device
    W = arena["windows"]["flags"].numel()
    wbeg, wend = layout["u_ranges"]
    keep = ((layout["u_flags"] & PF_ENCODABLE) != 0) & (wend != wbeg)
    rows = torch.nonzero(keep).flatten()  # ascending row id
    if rows.numel() >= 2 ** 31 or W >= 2 ** 31:
        raise ValueError("match search table exceeds int32 offsets")
    # a kept row has windows, so its name is one of the arena's group keys
    grp = torch.searchsorted(gk ^ _SIGN64, layout["u_gk"][rows] ^ _SIGN64)
    hi, lo = layout["u_hi"][rows], layout["u_lo"][rows]
    # stable sorts from the least significant column up; ties keep row order
    order = torch.argsort(lo ^ _SIGN64, stable=True)
    order = order[torch.argsort((hi ^ _SIGN64)[order], stable=True)]
    order = order[torch.argsort(grp[order], stable=True)]
    run_off = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(grp, minlength=G), 0, out=run_off[1:])
    win_grp = torch.repeat_interleave(
        torch.arange(G, device=dev), group_off[1:] - group_off[:-1])
    return {
        "s_key": torch.stack([hi[order], lo[order]], dim=1).contiguous(),
        "s_row": rows[order].to(torch.int32).contiguous(),
        "w_rbeg": run_off[win_grp].to(torch.int32).contiguous(),
        "w_rend": run_off[win_grp + 1].to(torch.int32).contiguous(),
    }


def build_reach_index(torch, src, dst, et, server_base: int, n_servers: int,
                      node_is_db_cred, node_is_db_tool) -> dict:
    """Per-server reach index for the blast counts (ops/csrc/blast.hip).

    A server's agents, creds and tools depend on the graph alone, so they
    are filtered, deduplicated and laid out once, next to the CSR, instead of
    once per visit of the server in every step.  Rows cover the server id
    range, widened to every source of a CONTAINS edge, so a package's
    containing server always has a row.  Layout:
      row_base   node id of row 0
      reach_col  int32 [T]: per row three consecutive segments -- distinct
                 agents (reverse USES), distinct creds (forward HAS_CRED),
                 distinct tools (forward PROVIDES_TOOL) -- each strictly
                 ascending by node id
      reach_off  int32 [S,4]: (agents begin, creds begin, tools begin, end);
                 a row's end is the next row's agents begin
      reach_db   int32 [S,2]: distinct creds with node_is_db_cred set,
                 distinct tools with node_is_db_tool set
    """
    dev = src.device
    lo, hi = int(server_base), int(server_base) + int(n_servers)
    holders = src[et == ET_CONTAINS]
    if holders.numel():
        lo = min(lo, int(holders.min().item()))
        hi = max(hi, int(holders.max().item()) + 1)
    S = hi - lo

    # one key per (row, segment, neighbour); unique() sorts and deduplicates
    keys = []
    for seg, (etype, row_node, nbr) in enumerate((
            (ET_USES, dst, src), (ET_HAS_CRED, src, dst), (ET_PROVIDES_TOOL, src, dst))):
        m = (et == etype) & (row_node >= lo) & (row_node < hi)
        row = row_node[m].to(torch.int64) - lo
        keys.append(((row * 3 + seg) << 32) | nbr[m].to(torch.int64))
    key = torch.unique(torch.cat(keys))
    slot = key >> 32  # row * 3 + segment
    nbr = key & 0xFFFFFFFF
    if key.numel() >= 2 ** 31:
        raise ValueError("reach index exceeds int32 offsets")

    bounds = torch.zeros(3 * S + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(slot, minlength=3 * S), 0, out=bounds[1:])
    pick = 3 * torch.arange(S, device=dev).unsqueeze(1) + torch.arange(4, device=dev)
    reach_off = bounds[pick].to(torch.int32).contiguous()

    reach_db = torch.zeros(S, 2, dtype=torch.int64, device=dev)
    row = slot // 3
    seg = slot - 3 * row
    for column, (which, flag) in enumerate(((1, node_is_db_cred), (2, node_is_db_tool))):
        m = seg == which
        reach_db[:, column].index_add_(0, row[m], flag[nbr[m]].to(torch.int64))
    return {
        "row_base": lo,
        "reach_col": nbr.to(torch.int32).contiguous(),
        "reach_off": reach_off,
        "reach_db": reach_db.to(torch.int32).contiguous(),
    }


def build_agent_index(torch, src, dst, et, n_agents: int, reach_index: dict) -> dict:
    """Per-agent server index for the multi-hop expansion
    (ops/csrc/blast_hops.hip), the forward counterpart of the agents segment
    of the reach index and built once with it.  Agents are the node ids
    ``0..n_agents-1``.  Layout:
      agent_off  int32 [n_agents+1]: agent -> its span in ``agent_srv``
      agent_srv  int32 [T]: each agent's distinct servers (USES targets),
                 strictly ascending by node id
    The expansion looks servers up in the reach index and agents up here, so
    every USES edge must run from an agent id to a server with a reach row.
    """
    dev = src.device
    uses = et == ET_USES
    a, s = src[uses].to(torch.int64), dst[uses].to(torch.int64)
    lo = int(reach_index["row_base"])
    hi = lo + int(reach_index["reach_off"].shape[0])
    if a.numel() and (int(a.max().item()) >= n_agents or int(s.min().item()) < lo
                      or int(s.max().item()) >= hi):
        raise ValueError("agent index: a USES edge leaves the agent or server id range")
    # one key per (agent, server); unique() sorts and deduplicates
    key = torch.unique((a << 32) | s)
    if key.numel() >= 2 ** 31:
        raise ValueError("agent index exceeds int32 offsets")
    agent_off = torch.zeros(n_agents + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(key >> 32, minlength=n_agents), 0, out=agent_off[1:])
    return {
        "agent_off": agent_off.to(torch.int32).contiguous(),
        "agent_srv": (key & 0xFFFFFFFF).to(torch.int32).contiguous(),
    }


def blast_index_enabled() -> bool:
    """A/B toggle: AGENT_BOM_BLAST_INDEX=0 makes ``_blast_counts_fused`` walk
    the CSR rows per package (``native.blast_counts``) instead of joining
    the packages against the per-server reach index."""
    import os

    return os.environ.get("AGENT_BOM_BLAST_INDEX", "1") != "0"


def match_by_window_enabled() -> bool:
    """A/B toggle: AGENT_BOM_MATCH_BY_WINDOW=0 makes the dedup path of
    ``EstateEngine.step`` match with one thread per distinct row
    (``native.match_launch``) instead of one thread per advisory window over
    the row search table (``native.match_by_window_launch``)."""
    import os

    return os.environ.get("AGENT_BOM_MATCH_BY_WINDOW", "1") != "0"


def findings_native_enabled() -> bool:
    """A/B toggle: AGENT_BOM_FINDINGS_NATIVE=0 makes the GPU dedup path of
    ``EstateEngine.step`` assemble findings with the torch op chain
    (``expand_dedup_matches`` + ``unique_consecutive`` + ``searchsorted``)
    instead of ops/csrc/findings.hip."""
    import os

    return os.environ.get("AGENT_BOM_FINDINGS_NATIVE", "1") != "0"


def findings_ahead_enabled() -> bool:
    """A/B toggle: AGENT_BOM_FINDINGS_AHEAD=0 makes ``EstateEngine.step`` run
    only the count phase of the finding assembly on the side stream and the
    emit phase and the blast counts after the reach BFS, sized by a host
    read, instead of running them all on the side stream under the BFS with
    output sizes predicted from the step before
    (``native.assemble_findings_begin_ahead``)."""
    import os

    return os.environ.get("AGENT_BOM_FINDINGS_AHEAD", "1") != "0"


def expand_dedup_matches(torch, layout: dict, su, sw):
    """Fan unique-row matches back out to per-package (orig_idx, win) pairs,
    sorted by (pkg << 32 | win) — identical to the non-dedup output.

    The torch reference of the finding assembly: the single-GPU step runs
    ops/csrc/findings.hip instead (no sort); this chain remains the oracle
    of its tests, the AGENT_BOM_FINDINGS_NATIVE=0 path and what the
    distributed engine and scripts/stage_timing.py call.

    Accepts UNSORTED (su, sw) — the one F-sized value sort at the end
    canonicalizes, so match_finalize can skip its pair sort (sort=False).
    A cross-product construction replacing the int64 value sort with a
    stable int32 argsort was A/B-measured at BOTH scales and rejected
    (2.50 vs 2.38 ms at 10M pkgs; 18.96 vs 18.69 ms at 100M): argsort
    internally sorts (key, index) pairs — the same 8 bytes/element the
    packed sort moves — so nothing is saved at any size; see
    profiles/r02_rank_kernel.md."""
    dev = su.device
    if su.numel() == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e.clone()
    run_off = layout["run_off"]
    cnt = run_off[su + 1] - run_off[su]
    rep = torch.repeat_interleave(
        torch.arange(su.numel(), device=dev), cnt)
    ends = torch.cumsum(cnt, 0)
    base = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), ends[:-1]])
    within = torch.arange(int(ends[-1].item()) if ends.numel() else 0,
                          device=dev) - base[rep]
    rows2 = run_off[su][rep] + within
    orig = layout["perm2"][rows2]
    packed = (orig << 32) | sw[rep]
    packed, _ = torch.sort(packed)
    return (packed >> 32), (packed & 0xFFFFFFFF)



_RANK_WS: dict = {}


def rank_order(torch, scores):
    """Deterministic finding rank: score desc (0.01 quantization), index asc.

    Scores are clipped to [0, 10] and serialized rounded, so 0.01 buckets
    preserve every visible distinction.  On GPU the rank is the stable
    1024-bin counting-sort kernel (ops/csrc/rank.hip — four small launches,
    no rocprim); the CPU path packs (bucket,
    index) into one integer key and sorts.  Both produce the identical
    (bucket asc, index asc) order -> bit-equal CPU/GPU.
    """
    n = scores.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=scores.device)
    if scores.is_cuda:
        from agentbom_amd.ops import native

        return native.rank_bucket_order(scores.contiguous(), _RANK_WS)
    q = (scores * 100).round().clamp(0, 1000).to(torch.int64)
    bits = max(1, (n - 1).bit_length())
    key = ((1000 - q) << bits) | torch.arange(n, device=scores.device)
    if (1010 << bits) < (1 << 31):
        key = key.to(torch.int32)
    skey, _ = torch.sort(key)
    return (skey.to(torch.int64)) & ((1 << bits) - 1)


# edge types dependency_reach() walks
_REACH_MASK = (1 << ET_USES) | (1 << ET_CONTAINS) | (1 << ET_HAS_CRED) | (1 << ET_PROVIDES_TOOL)


class EstateEngine:
    """Device-resident estate + advisory arena + the findings pipeline."""

    def __init__(self, estate: SyntheticEstate, device: str = "cuda"):
        import torch

        self.torch = torch
        self.estate = estate
        self.device = torch.device(device)
        self.N = estate.num_nodes
        dev = self.device

        src = torch.from_numpy(estate.edge_src).to(dev)
        dst = torch.from_numpy(estate.edge_dst).to(dev)
        et = torch.from_numpy(estate.edge_type).to(dev)

        self.fwd = self._build_csr(src, dst, et)
        self.rev = self._build_csr(dst, src, et)

        self.pkg_group_key = torch.from_numpy(estate.pkg_name_id.view(np.int64)).to(dev)
        self.pkg_key_hi = torch.from_numpy(estate.pkg_key_hi.view(np.int64)).to(dev)
        self.pkg_key_lo = torch.from_numpy(estate.pkg_key_lo.view(np.int64)).to(dev)
        self.pkg_flags = torch.from_numpy(estate.pkg_flags).to(dev)
        # Match-locality layout: packages sorted by group key so adjacent
        # lanes binary-search identical tree paths (L1/L2-resident) and walk
        # the same window runs.  ``pkg_perm`` maps sorted row -> original
        # package index for output reporting.
        self.pkg_perm = torch.argsort(self.pkg_group_key, stable=True)
        self.pkg_group_key_sorted = self.pkg_group_key[self.pkg_perm].contiguous()
        self.pkg_key_hi_sorted = self.pkg_key_hi[self.pkg_perm].contiguous()
        self.pkg_key_lo_sorted = self.pkg_key_lo[self.pkg_perm].contiguous()
        self.pkg_flags_sorted = self.pkg_flags[self.pkg_perm].contiguous()

        self.arena = estate.arena.to_torch(dev)
        # resident-estate match index: per-package advisory window range,
        # precomputed once (estate and arena are static between steps) so
        # the match kernel skips the per-package group binary search
        self.pkg_win_range = _precompute_win_ranges(
            torch, self.arena, self.pkg_group_key_sorted)
        # dedup-match layout (None when the estate is >90% distinct rows)
        self.match_dedup = build_dedup_match_layout(
            torch, self.arena, self.pkg_group_key, self.pkg_key_hi,
            self.pkg_key_lo, self.pkg_flags) if self.use_gpu else None
        # row search table of the window-per-thread match: the distinct rows
        # of every advisory group in version-key order, built once like the
        # layout it indexes
        self.match_table = build_match_search_table(
            torch, self.arena, self.match_dedup) if self.match_dedup is not None else None
        self.cred_is_db = torch.from_numpy(estate.cred_is_db).to(dev)
        self.tool_is_db = torch.from_numpy(estate.tool_is_db).to(dev)
        self.cred_lut = torch.from_numpy(_impact_lut(_FULL_CRED, _DB_CRED)).to(dev)
        self.tool_lut = torch.from_numpy(_impact_lut(_FULL_TOOL, _DB_TOOL)).to(dev)

        self.agent_ids = torch.arange(estate.n_agents, dtype=torch.int32, device=dev)
        self._bfs_ws: dict = {}
        self._reach_ws: dict = {}  # ops/csrc/reach_sets.hip state, see agent_reach
        # out-degree sum of the BFS sources: a property of the CSR and the
        # agent ids, like pkg_win_range, so the reach BFS need not read it
        # back from the device every step
        agents = self.agent_ids.to(torch.int64)
        self._agents_degree = int(
            (self.fwd["row_off"][agents + 1] - self.fwd["row_off"][agents]).sum())
        self._findings_ws: dict = {}  # ops/csrc/findings.hip workspace
        self._match_stream = None  # side stream: match ∥ reach BFS overlap

        # per-node db-credential / db-tool indicator (for impact filtering)
        self.node_is_db_cred = torch.zeros(self.N, dtype=torch.uint8, device=dev)
        self.node_is_db_cred[
            estate.cred_base + torch.arange(estate.n_creds, device=dev)
        ] = self.cred_is_db
        self.node_is_db_tool = torch.zeros(self.N, dtype=torch.uint8, device=dev)
        self.node_is_db_tool[
            estate.tool_base + torch.arange(estate.n_tools, device=dev)
        ] = self.tool_is_db

        # per-server reach index: a layout of the graph like fwd/rev, with
        # their lifetime; the step joins every matched package against it
        self._blast_ws: dict = {}
        self.reach_index = build_reach_index(
            torch, src, dst, et, estate.server_base, estate.n_servers,
            self.node_is_db_cred, self.node_is_db_tool) if self.use_gpu else None
        # parent index of the reach BFS's bottom-up pass: one word per vertex
        # of (rev, the mask of dependency_reach), same lifetime; 4N bytes
        self.bfs_parent_index = None
        if self.use_gpu:
            from agentbom_amd.ops import native

            self.bfs_parent_index = native.bfs_parent_index(self.rev, _REACH_MASK, self.N)
        # per-agent server index of the multi-hop expansion: same lifetime
        self._hops_ws: dict = {}
        self.agent_index = build_agent_index(
            torch, src, dst, et, estate.n_agents, self.reach_index) if self.use_gpu else None
        self._hop_factor = torch.tensor(
            [0.0] + [HOP_RISK_FACTORS[h] for h in range(1, 6)],
            dtype=torch.float32, device=dev)
        # remediation plan: package -> (name, version) item, built at first
        # use, and the workspace of ops/csrc/remediation.hip
        self._remed_items = None
        self._remed_ws: dict = {}
        # toxic combinations: the workspace of ops/csrc/toxic.hip, the server
        # table of the last caps tensor and the count of the last advisory map
        self._toxic_ws: dict = {}
        self._toxic_cache = None
        self._toxic_vuln_cache = None

    def _build_csr(self, src, dst, et):
        """GPU CSR construction: stable sort by src, bincount offsets."""
        torch = self.torch
        order = torch.argsort(src, stable=True)
        row_counts = torch.bincount(src, minlength=self.N)
        row_off = torch.zeros(self.N + 1, dtype=torch.int64, device=src.device)
        torch.cumsum(row_counts, 0, out=row_off[1:])
        return {
            "row_off": row_off,
            "col": dst[order].to(torch.int32),
            "etype": et[order].contiguous(),
            # col-aligned edge sources: enables edge-centric dense-frontier BFS
            "src": src[order].to(torch.int32),
        }

    # ── pipeline stages ────────────────────────────────────────────────────

    @property
    def use_gpu(self) -> bool:
        return self.device.type == "cuda"

    def match(self):
        """(finding_pkg_idx, finding_win_idx) int64 device tensors."""
        if self.use_gpu:
            from agentbom_amd.ops import native

            sp, sw = native.match(
                self.pkg_group_key_sorted, self.pkg_key_hi_sorted,
                self.pkg_key_lo_sorted, self.pkg_flags_sorted,
                self.arena["group_keys"], self.arena["group_off"], self.arena["windows"],
                pkg_win_range=self.pkg_win_range,
            )
            return self._unsort_matches(sp, sw)
        # CPU oracle path (tests / dev boxes)
        from agentbom_amd.ops import cpu_ref

        torch = self.torch
        win = {k: v.numpy().view(np.uint64) if v.dtype == torch.int64 else v.numpy()
               for k, v in self.arena["windows"].items()}
        pkg_i, win_i = cpu_ref.match(
            self.pkg_group_key.numpy().view(np.uint64),
            self.pkg_key_hi.numpy().view(np.uint64),
            self.pkg_key_lo.numpy().view(np.uint64),
            self.pkg_flags.numpy(),
            self.arena["group_keys"].numpy().view(np.uint64),
            self.arena["group_off"].numpy().view(np.uint32),
            win,
        )
        return torch.from_numpy(pkg_i), torch.from_numpy(win_i)

    def _unsort_matches(self, sp, sw):
        """Map sorted match rows back to original package indices and re-sort
        for the deterministic (pkg, window) output order."""
        orig = self.pkg_perm[sp]
        packed = (orig << 32) | sw
        packed, _ = self.torch.sort(packed)
        return (packed >> 32), (packed & 0xFFFFFFFF)

    def _reach_begin(self):
        """Enqueue the reach BFS's dist fill and seeding (no sync); follow
        with ``dependency_reach(begun=True)`` on the same stream."""
        from agentbom_amd.ops import native

        native.bfs_begin(self.fwd["row_off"], self.agent_ids, self.N, self._bfs_ws)

    def dependency_reach(self, begun: bool = False):
        """u32 hop distance from the nearest agent, per node (multi-source BFS).

        ``begun``: :meth:`_reach_begin` has been called for this pass."""
        mask = _REACH_MASK
        if self.use_gpu:
            from agentbom_amd.ops import native

            return native.bfs(
                self.fwd["row_off"], self.fwd["col"], self.agent_ids, self.N,
                etype=self.fwd["etype"], allowed_mask=mask, workspace=self._bfs_ws,
                edge_src=self.fwd["src"], rev=self.rev,
                begun=begun, sources_degree=self._agents_degree,
                parent_index=self.bfs_parent_index,
            )
        from agentbom_amd.ops import cpu_ref

        dist = cpu_ref.bfs(
            self.fwd["row_off"].numpy(), self.fwd["col"].numpy(),
            self.agent_ids.numpy(), self.N,
            etype=self.fwd["etype"].numpy(), allowed_mask=mask,
        )
        return self.torch.from_numpy(dist.view(np.int32)).to(self.torch.int32)

    def agent_reach(self, agent_ids, targets=None, max_depth: int = 16) -> dict:
        """Which of ``agent_ids`` reach which ``targets``, and in how many hops.

        ``agent_ids``: node ids of the source agents (any integer tensor or
        sequence; duplicates keep their own column).  ``targets``: distinct
        node ids, by default every package node of the estate; pass the
        matched unique packages of a step (``unique(step["pkg_idx"]) +
        estate.pkg_base``) to ask about those alone.  The walk is that of
        :meth:`dependency_reach`: forward CSR, same edge types, and a node at
        distance ``max_depth`` is recorded but not expanded.

        Returns tensors on the engine's device: ``hops`` uint8 [T, S] (255 =
        not reached within ``max_depth``), ``agents`` int32 [S], ``targets``
        int32 [T], ``n_reaching`` int32 [T] (sources with ``hops != 255``) and
        ``min_hop`` uint8 [T] (255 where none).  On a CUDA device the hops
        come from ``native.reach_hops`` (ops/csrc/reach_sets.hip), on the CPU
        from ``cpu_ref.reach_hops``."""
        torch = self.torch
        dev = self.device
        mask = (1 << ET_USES) | (1 << ET_CONTAINS) | (1 << ET_HAS_CRED) | (1 << ET_PROVIDES_TOOL)
        agents = torch.as_tensor(agent_ids, device=dev).to(torch.int32).reshape(-1).contiguous()
        if targets is None:
            targets = self.estate.pkg_base + torch.arange(
                self.N - self.estate.pkg_base, dtype=torch.int32, device=dev)
        targets = torch.as_tensor(targets, device=dev).to(torch.int32).reshape(-1).contiguous()
        if self.use_gpu:
            from agentbom_amd.ops import native

            hops = native.reach_hops(
                self.fwd["row_off"], self.fwd["col"], agents, targets, self.N,
                etype=self.fwd["etype"], allowed_mask=mask, max_depth=max_depth,
                workspace=self._reach_ws)
        else:
            from agentbom_amd.ops import cpu_ref

            hops = torch.from_numpy(cpu_ref.reach_hops(
                self.fwd["row_off"].numpy(), self.fwd["col"].numpy(), agents.numpy(),
                targets.numpy(), self.N, etype=self.fwd["etype"].numpy(),
                allowed_mask=mask, max_depth=max_depth))
        if agents.numel():
            min_hop = hops.min(dim=1).values
        else:
            min_hop = torch.full((targets.numel(),), 255, dtype=torch.uint8, device=dev)
        return {
            "hops": hops,
            "agents": agents,
            "targets": targets,
            "n_reaching": (hops != 255).sum(dim=1, dtype=torch.int32),
            "min_hop": min_hop,
        }

    def _expand(self, csr, rows, carry, want_type: int):
        """Segmented gather: neighbors of ``rows`` with ``carry`` repeated.

        Returns (neighbor_node, carried_value) filtered to edge type
        ``want_type``.
        """
        torch = self.torch
        row_off = csr["row_off"]
        beg = row_off[rows]
        cnt = row_off[rows + 1] - beg
        total = int(cnt.sum().item())
        if total == 0:
            empty = torch.empty(0, dtype=torch.int64, device=self.device)
            return empty, empty
        rep = torch.repeat_interleave(torch.arange(rows.numel(), device=self.device), cnt)
        cum = torch.zeros(rows.numel(), dtype=torch.int64, device=self.device)
        torch.cumsum(cnt, 0, out=cum)
        base = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), cum[:-1]])
        eidx = torch.arange(total, device=self.device) - base[rep] + beg[rep]
        keep = csr["etype"][eidx] == want_type
        nbr = csr["col"][eidx][keep].to(torch.int64)
        return nbr, carry[rep[keep]]

    def _distinct_counts(self, key_a, key_b, n_bins: int, weights=None):
        """Count distinct (a, b) pairs per a; optional 0/1 weight per b kind."""
        torch = self.torch
        if key_a.numel() == 0:
            z = torch.zeros(n_bins, dtype=torch.int32, device=self.device)
            return z if weights is None else (z, z.clone())
        pair = key_a * self.N + key_b
        uniq = torch.unique(pair)
        ua = uniq // self.N
        ub = uniq % self.N
        cnt = torch.bincount(ua, minlength=n_bins).to(torch.int32)
        if weights is None:
            return cnt
        w = weights[ub].to(torch.int64)
        cnt_w = torch.bincount(ua, weights=w.to(torch.float64), minlength=n_bins)
        return cnt, cnt_w.to(torch.int32)

    def blast_counts(self, finding_pkgs):
        """Per unique finding-package reach counts.

        GPU path: the indexed kernels of ops/csrc/blast.hip (thread per
        package from the per-server reach index, wave per multi-server
        package); zipf-head packages that overflow the LDS caps fall back to
        the exact sort-based join below.  CPU path: the sort-based join
        throughout.
        Returns dense tensors indexed by position in ``uniq_pkgs``.
        """
        torch = self.torch
        # finding_pkgs arrives sorted (the match-finalize pair sort), so
        # unique_consecutive avoids torch.unique's internal re-sort
        uniq_pkgs = torch.unique_consecutive(finding_pkgs)
        if self.use_gpu:
            return self._blast_counts_fused(uniq_pkgs)
        return self._blast_counts_join(uniq_pkgs)

    def _blast_counts_fused(self, uniq_pkgs, uniq_pkgs32=None):
        """``uniq_pkgs32``: the same ids as int32, when the caller already
        has them (the native finding assembly writes both)."""
        from agentbom_amd.ops import native

        torch = self.torch
        if uniq_pkgs32 is None:
            uniq_pkgs32 = uniq_pkgs.to(torch.int32).contiguous()
        if self.reach_index is not None and blast_index_enabled():
            # index path: the kernels count the overflowed rows, so nonzero()
            # and the join below run only when there are any
            counts, overflow, n_overflow = native.blast_counts_indexed(
                uniq_pkgs32, self.rev, self.reach_index, ET_CONTAINS,
                self.node_is_db_cred, self.node_is_db_tool, self._blast_ws)
        else:
            counts, overflow = native.blast_counts(
                uniq_pkgs32, self.rev, self.fwd,
                (ET_CONTAINS, ET_USES, ET_HAS_CRED, ET_PROVIDES_TOOL),
                self.node_is_db_cred, self.node_is_db_tool,
            )
            n_overflow = None
        return self._blast_counts_resolve(uniq_pkgs, counts, overflow, n_overflow)

    def _blast_counts_resolve(self, uniq_pkgs, counts, overflow, n_overflow,
                              counts_only: bool = False):
        """The kernels' counts [n, 6] as the result dict, the overflowed rows
        recomputed by the exact join.  ``n_overflow``: how many rows the
        kernels flagged, None when they did not count them.  ``counts_only``:
        the caller reads nothing but ``counts2d`` (the step, whose host time
        after the BFS is on the critical path), so the six column views are
        left out when no row overflowed."""
        torch = self.torch
        if n_overflow == 0 and counts_only:
            return {"uniq_pkgs": uniq_pkgs, "counts2d": counts}
        result = {
            "uniq_pkgs": uniq_pkgs,
            "n_servers": counts[:, 0].to(torch.int32),
            "n_agents": counts[:, 1].to(torch.int32),
            "n_creds_all": counts[:, 2].to(torch.int32),
            "n_creds_db": counts[:, 3].to(torch.int32),
            "n_tools_all": counts[:, 4].to(torch.int32),
            "n_tools_db": counts[:, 5].to(torch.int32),
        }
        if n_overflow == 0:
            result["counts2d"] = counts
            return result
        ov_idx = torch.nonzero(overflow).flatten()
        if ov_idx.numel():
            heavy = self._blast_counts_join(uniq_pkgs[ov_idx])
            counts = counts.clone()
            for k, key in enumerate(("n_servers", "n_agents", "n_creds_all",
                                     "n_creds_db", "n_tools_all", "n_tools_db")):
                result[key] = result[key].clone()
                result[key][ov_idx] = heavy[key]
                counts[ov_idx, k] = heavy[key]
        result["counts2d"] = counts  # [U,6] — feeds the fused score_gather
        return result

    def _blast_counts_join(self, uniq_pkgs):
        """Sort-based exact join (torch ops) — CPU path + overflow fallback."""
        torch = self.torch
        # position index for dense bincounts
        n_up = uniq_pkgs.numel()
        pos = torch.arange(n_up, device=self.device)

        # package -> servers (reverse CONTAINS)
        srv, carry = self._expand(self.rev, uniq_pkgs, pos, ET_CONTAINS)
        n_servers = self._distinct_counts(carry, srv, n_up)

        # servers -> agents (reverse USES), carry package position
        ag, carry2 = self._expand(self.rev, srv, carry, ET_USES)
        n_agents = self._distinct_counts(carry2, ag, n_up)

        # servers -> creds / tools (forward)
        cr, carry3 = self._expand(self.fwd, srv, carry, ET_HAS_CRED)
        n_creds_all, n_creds_db = self._distinct_counts(
            carry3, cr, n_up, weights=self.node_is_db_cred
        )
        tl, carry4 = self._expand(self.fwd, srv, carry, ET_PROVIDES_TOOL)
        n_tools_all, n_tools_db = self._distinct_counts(
            carry4, tl, n_up, weights=self.node_is_db_tool
        )
        return {
            "uniq_pkgs": uniq_pkgs,
            "n_servers": n_servers,
            "n_agents": n_agents,
            "n_creds_all": n_creds_all,
            "n_creds_db": n_creds_db,
            "n_tools_all": n_tools_all,
            "n_tools_db": n_tools_db,
        }

    def step(self, blast_depth: int = 1, reach_dist=None):
        """One full findings pass.  Returns summary dict.

        ``reach_dist`` overrides the locally-computed dependency-reach
        distances (multi-GPU mode passes the shard's slice of the
        distributed BFS result).

        ``blast_depth`` > 1 (clamped to 5) adds the multi-hop delegation
        expansion per finding: ``hop_depth`` uint8, ``transitive_agents`` and
        ``transitive_creds`` int32 (see :meth:`transitive_blast`) and
        ``transitive_scores`` fp32 = ``scores * HOP_RISK_FACTORS[hop_depth]``
        where ``hop_depth`` > 1, else 0.  At 1 the pass is the same as before
        and returns no such keys."""
        torch = self.torch
        assembled = None
        if self.use_gpu:
            # Overlap: the match kernel has no dependency on the reach BFS,
            # so it runs on a side HIP stream while the BFS host loop (which
            # syncs its own stream every level) drives the default stream.
            # The finding assembly and the blast counts follow the match on
            # that stream; the main stream joins it after the BFS and runs
            # what needs both arms (score, rank) or a size the side arm
            # could not predict.
            from agentbom_amd.ops import native

            if self._match_stream is None:
                self._match_stream = torch.cuda.Stream(device=self.device)
            side = self._match_stream
            if reach_dist is None:
                # the BFS's 4N-byte dist fill and its seeding go ahead of the
                # match: beside it the fill gets no wave slots (the match
                # grid holds all of them) and runs at a few % of bandwidth
                self._reach_begin()
            side.wait_stream(torch.cuda.current_stream())
            dd = self.match_dedup
            with torch.cuda.stream(side):
                if (dd is not None and self.match_table is not None
                        and match_by_window_enabled()):
                    # dedup-match by window: every advisory window searches
                    # the sorted distinct rows of its group; pairs are keyed
                    # by distinct row, as below
                    pending = native.match_by_window_launch(
                        self.arena["windows"], self.match_table)
                elif dd is not None:
                    # dedup-match: one kernel row per DISTINCT (name,
                    # version); results fan back out below
                    pending = native.match_launch(
                        dd["u_gk"], dd["u_hi"], dd["u_lo"], dd["u_flags"],
                        self.arena["group_keys"], self.arena["group_off"],
                        self.arena["windows"], pkg_win_range=dd["u_ranges"],
                        order=dd["heavy_order"])
                else:
                    pending = native.match_launch(
                        self.pkg_group_key_sorted, self.pkg_key_hi_sorted,
                        self.pkg_key_lo_sorted, self.pkg_flags_sorted,
                        self.arena["group_keys"], self.arena["group_off"],
                        self.arena["windows"], pkg_win_range=self.pkg_win_range)
                counting = None
                if (dd is not None and findings_native_enabled()
                        and self.reach_index is not None and blast_index_enabled()
                        and findings_ahead_enabled()):
                    # neither the finding assembly nor the blast counts need
                    # the BFS: with the output sizes of the last step as
                    # capacities, all of it follows the match on the side
                    # stream, enqueued by one call before the BFS loop starts
                    counting = native.assemble_findings_begin_ahead(
                        pending, dd, self._findings_ws, self.estate.pkg_base,
                        native.blast_inputs(
                            self.rev, self.reach_index, ET_CONTAINS,
                            self.node_is_db_cred, self.node_is_db_tool, self._blast_ws))
                elif dd is not None and findings_native_enabled():
                    # the count phase of the finding assembly needs the
                    # pairs and not the BFS: it follows the match on the side
                    # stream, and its totals are on the host by the time the
                    # BFS host loop returns
                    counting = native.assemble_findings_begin(
                        pending, dd, self._findings_ws)
            dist = (reach_dist if reach_dist is not None
                    else self.dependency_reach(begun=True))
            torch.cuda.current_stream().wait_stream(side)
            if counting is not None:
                # pairs -> sorted findings + unique packages + positions in
                # HIP (ops/csrc/findings.hip): no sort, one host read
                assembled = native.assemble_findings_finish(
                    counting, self.estate.pkg_base)
            else:
                # downstream always re-canonicalizes; skip the pair sort
                sp, sw = native.match_finalize(pending, sort=False)
                if dd is not None:
                    pkg_idx, win_idx = expand_dedup_matches(torch, dd, sp, sw)
                else:
                    pkg_idx, win_idx = self._unsort_matches(sp, sw)
        else:
            pkg_idx, win_idx = self.match()
            dist = reach_dist if reach_dist is not None else self.dependency_reach()

        if assembled is not None:
            pkg_idx, win_idx = assembled["pkg_idx"], assembled["win_idx"]
            pkg_nodes, pos = assembled["pkg_nodes"], assembled["pos"]
            if "blast_counts" in assembled:
                # counted on the side stream with the assembly; only rows
                # that overflowed an LDS cap are left, for the exact join
                counts = self._blast_counts_resolve(
                    assembled["uniq_pkgs"], assembled["blast_counts"],
                    assembled["blast_overflow"], assembled["blast_n_overflow"],
                    counts_only=True)
            else:
                counts = self._blast_counts_fused(assembled["uniq_pkgs"],
                                                  assembled["uniq_pkgs32"])
        else:
            pkg_nodes = pkg_idx + self.estate.pkg_base
            counts = self.blast_counts(pkg_nodes)
            # map each finding to its unique-package position
            pos = torch.searchsorted(counts["uniq_pkgs"], pkg_nodes)
        n_findings = pkg_idx.numel()

        if self.use_gpu:
            # fused gather + score: arena gathers, CWE-impact LUT count
            # selection, reachability and the risk formula in ONE kernel
            from agentbom_amd.ops import native

            scores, n_agents, n_creds, n_tools = native.score_gather(
                win_idx.contiguous(), pkg_nodes.contiguous(), pos.contiguous(),
                self.arena["severity"], self.arena["kev"], self.arena["epss"],
                self.arena["impact"], self.cred_lut, self.tool_lut,
                counts["counts2d"].contiguous(), dist)
        else:
            scores, n_agents, n_creds, n_tools = self._score_cpu(
                counts, pos, pkg_nodes, win_idx, dist)

        res = {
            "n_findings": int(n_findings),
            "scores": scores,
            # deterministic rank: quantized score desc, finding index asc
            "order": rank_order(torch, scores),
            "pkg_idx": pkg_idx,
            "win_idx": win_idx,
            "n_agents": n_agents,
            "n_creds": n_creds,
            "n_tools": n_tools,
            "reach_dist": dist,
        }
        if blast_depth > 1:
            # multi-hop expansion of the unique packages, on the main stream
            # after the join, fanned out to the findings through ``pos``
            hops = self._blast_hops(
                counts["uniq_pkgs"],
                assembled["uniq_pkgs32"] if assembled is not None else None, blast_depth)
            hop_depth = hops["hop_depth"][pos]
            res["hop_depth"] = hop_depth
            res["transitive_agents"] = hops["t_agents"][pos]
            res["transitive_creds"] = hops["t_creds"][pos]
            # one fp32 multiply, unrounded: rounding belongs to presentation
            res["transitive_scores"] = torch.where(
                hop_depth > 1, scores * self._hop_factor[hop_depth.to(torch.int64)],
                torch.zeros_like(scores))
        return res

    def _blast_hops(self, uniq_pkgs, uniq_pkgs32, max_depth: int) -> dict:
        """The multi-hop expansion of ``uniq_pkgs`` (node ids, int64): the
        kernels of ops/csrc/blast_hops.hip on the GPU, ``cpu_ref.blast_hops``
        on the CPU.  ``max_depth`` is clamped to [1, 5]."""
        torch = self.torch
        if self.use_gpu:
            from agentbom_amd.ops import native

            if uniq_pkgs32 is None:
                uniq_pkgs32 = uniq_pkgs.to(torch.int32).contiguous()
            out = native.blast_hops(uniq_pkgs32, self.rev, self.reach_index, self.agent_index,
                                    ET_CONTAINS, max_depth, self._hops_ws)
        else:
            from agentbom_amd.ops import cpu_ref

            hop_agents, t_creds, hop_depth = cpu_ref.blast_hops(
                uniq_pkgs.numpy(), self.rev["row_off"].numpy(), self.rev["col"].numpy(),
                self.rev["etype"].numpy(), ET_CONTAINS, ET_USES, ET_HAS_CRED,
                self.fwd["row_off"].numpy(), self.fwd["col"].numpy(),
                self.fwd["etype"].numpy(), max_depth)
            out = {"hop_agents": torch.from_numpy(hop_agents),
                   "t_creds": torch.from_numpy(t_creds),
                   "hop_depth": torch.from_numpy(hop_depth)}
        out["t_agents"] = out["hop_agents"].sum(dim=1, dtype=torch.int32)
        out["uniq_pkgs"] = uniq_pkgs
        return out

    def transitive_blast(self, step_res=None, max_depth: int = 3) -> dict:
        """Multi-hop delegation blast radius per unique matched package: who
        is exposed transitively through agents that share servers.

        Returns tensors on the engine's device, indexed by position in
        ``uniq_pkgs`` (ascending package node ids of ``step_res``):
        ``hop_agents`` int32 [U,4] (agents first reached at hop 2..5),
        ``t_agents`` int32 [U] (their sum), ``t_creds`` int32 [U] (distinct
        credentials on the servers of those agents) and ``hop_depth`` uint8
        [U] (deepest hop that reached a new agent, else 1).  Semantics:
        ``models.blast.expand_blast_radius_hops``; ``max_depth`` is clamped
        to [1, 5]."""
        torch = self.torch
        if step_res is None:
            step_res = self.step()
        pkg_nodes = (step_res["pkg_idx"] + self.estate.pkg_base).to(torch.int64)
        # pkg_idx arrives sorted: no re-sort needed
        return self._blast_hops(torch.unique_consecutive(pkg_nodes), None, max_depth)

    def remediation_items(self):
        """(item_of int32 [P], number of items): the index of every package's
        (pkg_group_key, pkg_key_hi, pkg_key_lo) triple among the distinct
        triples in ascending unsigned lexicographic order.  Built with torch
        at first use from the package columns alone, so it is the same with
        and without a dedup layout, and cached."""
        if self._remed_items is None:
            torch = self.torch
            P = self.pkg_group_key.numel()
            # stable sorts from the least significant column up; the sign
            # flip turns the int64 order into the u64 order
            order = torch.arange(P, device=self.device)
            for col in (self.pkg_key_lo, self.pkg_key_hi, self.pkg_group_key):
                order = order[torch.argsort((col ^ _SIGN64)[order], stable=True)]
            g, h, l = (c[order] for c in (self.pkg_group_key, self.pkg_key_hi, self.pkg_key_lo))
            new = torch.ones(P, dtype=torch.bool, device=self.device)
            new[1:] = (g[1:] != g[:-1]) | (h[1:] != h[:-1]) | (l[1:] != l[:-1])
            rank = torch.cumsum(new.to(torch.int32), 0, dtype=torch.int32) - 1
            item_of = torch.empty(P, dtype=torch.int32, device=self.device)
            item_of[order] = rank
            self._remed_items = (item_of, int(rank[-1]) + 1 if P else 0)
        return self._remed_items

    def remediation_plan(self, step_res=None, k: Optional[int] = 100) -> dict:
        """Fix-first remediation plan: the findings of a step grouped per
        (name, version) item -- "upgrade this and you clear that".

        Returns tensors on the engine's device, one entry per matched item,
        the first ``k`` (all with ``k=None``) in the order max_score
        descending, n_agents descending, item index ascending: the keys of
        ``cpu_ref.REMEDIATION_KEYS`` (semantics: ``cpu_ref.remediation_plan``)
        and ``agents_pct`` fp32 = 100 * n_agents / estate.n_agents; plus
        ``n_items``, the number of matched items.  On the GPU the per-item
        arrays come from the kernels of ops/csrc/remediation.hip
        (AGENT_BOM_REMEDIATION_NATIVE=0: from an exact torch join), on the
        CPU from the oracle.  Calls :meth:`step` when ``step_res`` is None."""
        torch = self.torch
        if step_res is None:
            step_res = self.step()
        item_of, n_items = self.remediation_items()
        pkg_idx, win_idx, scores = step_res["pkg_idx"], step_res["win_idx"], step_res["scores"]
        if self.use_gpu:
            from agentbom_amd.ops import native

            pkg_idx, win_idx = pkg_idx.contiguous(), win_idx.contiguous()
            scores = scores.contiguous()
            if native.remediation_native_enabled():
                per = native.remediation_items(
                    pkg_idx, win_idx, scores, item_of, n_items, self.arena, self.rev,
                    self.reach_index, ET_CONTAINS, self.estate.pkg_base, self._remed_ws)
            else:
                per = native.remediation_items_join(
                    pkg_idx, win_idx, scores, item_of, self.arena, self.rev,
                    self.reach_index, ET_CONTAINS, self.estate.pkg_base)
            pct = per["n_agents"].to(torch.float32) * 100.0 / float(self.estate.n_agents)
            # stable sorts from the last key up; positions are in item order
            order = torch.argsort(per["n_agents"], descending=True, stable=True)
            order = order[torch.argsort(per["max_score"][order], descending=True, stable=True)]
        else:
            from agentbom_amd.ops import cpu_ref

            windows = self.arena["windows"]
            ref = cpu_ref.remediation_plan(
                pkg_idx.numpy(), win_idx.numpy(), scores.numpy(), item_of.numpy(),
                self.rev["row_off"].numpy(), self.rev["col"].numpy(), self.rev["etype"].numpy(),
                self.fwd["row_off"].numpy(), self.fwd["col"].numpy(), self.fwd["etype"].numpy(),
                ET_CONTAINS, ET_USES, ET_HAS_CRED, ET_PROVIDES_TOOL, self.estate.pkg_base,
                windows["flags"].numpy(), windows["fixed_hi"].numpy(),
                windows["fixed_lo"].numpy(), self.arena["severity"].numpy(),
                self.arena["kev"].numpy(), self.estate.n_agents)
            per = {key: torch.from_numpy(ref[key]) for key in cpu_ref.REMEDIATION_KEYS}
            pct, order = torch.from_numpy(ref["agents_pct"]), torch.from_numpy(ref["order"])
        n_matched = order.numel()
        if k is not None:
            order = order[:max(int(k), 0)]
        plan = {key: value[order] for key, value in per.items()}
        plan["agents_pct"] = pct[order]
        plan["n_items"] = n_matched
        return plan

    def _toxic_caps(self, tool_caps):
        """(tool_caps uint8 [n_tools] on the device, its server table, its
        poison servers): the table and the poison servers depend on the graph
        and the caps alone, so they are kept for the last caps tensor seen
        (None: all-zero caps) until it is replaced or written to."""
        torch = self.torch
        key = None if tool_caps is None else (tool_caps.data_ptr(), tool_caps._version)
        cached = self._toxic_cache
        if cached is not None and cached["key"] == key:
            return cached["caps"], cached["table"], cached["poison"]
        n_tools = self.estate.n_tools
        if tool_caps is None:
            caps = torch.zeros(n_tools, dtype=torch.uint8, device=self.device)
        else:
            if tool_caps.dtype != torch.uint8:
                raise TypeError(f"tool_caps: expected torch.uint8, got {tool_caps.dtype}")
            if tool_caps.numel() != n_tools:
                raise ValueError(f"tool_caps: {tool_caps.numel()} elements, expected {n_tools}")
            caps = tool_caps.to(self.device).contiguous()
        table = poison = None
        if self.use_gpu:
            from agentbom_amd.ops import native

            table = native.toxic_server_table(self.reach_index, caps, self.tool_is_db,
                                              self.estate.tool_base)
            poison = native.toxic_poison_servers(table, self.reach_index["row_base"])
        # the caller's tensor is kept with the key: its address stays its own
        self._toxic_cache = {"key": key, "held": tool_caps, "caps": caps, "table": table,
                             "poison": poison}
        return caps, table, poison

    def _toxic_vuln_of(self, vuln_of):
        """(vuln_of int32 [W] on the device or None, number of advisories);
        the count of a map is read from it once and kept while the same
        tensor comes back."""
        torch = self.torch
        W = self.arena["severity"].numel()
        if vuln_of is None:
            return None, W
        if vuln_of.dtype != torch.int32:
            raise TypeError(f"vuln_of: expected torch.int32, got {vuln_of.dtype}")
        if vuln_of.numel() != W:
            raise ValueError(f"vuln_of: {vuln_of.numel()} elements, expected {W}")
        key = (vuln_of.data_ptr(), vuln_of._version)
        cached = self._toxic_vuln_cache
        if cached is None or cached["key"] != key:
            on_dev = vuln_of.to(self.device).contiguous()
            if W and int(on_dev.min()) < 0:
                raise ValueError("vuln_of: negative advisory index")
            cached = self._toxic_vuln_cache = {
                "key": key, "held": vuln_of, "map": on_dev,
                "n": int(on_dev.max()) + 1 if W else 0}
        return cached["map"], cached["n"]

    def toxic_combinations(self, step_res=None, tool_caps=None, vuln_of=None,
                           k: Optional[int] = 100) -> dict:
        """Toxic combinations of a step's findings: risks that are tolerable
        alone and critical together -- a critical or high CVE with exposed
        credentials, a KEV with credentials, a CVE behind an execute-capable
        or a retrieval tool, a CVE on a server that agents share, one
        advisory that reaches three or more agents -- per finding and per
        advisory, and the shared servers with a write and a read tool.
        Semantics, bits and scores: ``cpu_ref.toxic_combinations``.

        ``tool_caps`` uint8 [estate.n_tools] gives the ``cpu_ref.TC_*``
        capability bits of every tool (``toxic_combos.tool_caps_from_labels``
        derives them from tool names); None means no capabilities: the tool
        patterns and ``poison_servers`` are then empty.  ``vuln_of`` int32 [W]
        maps an advisory window to its advisory (default: a window is one).

        Returns tensors on the engine's device.  Aligned with ``step_res``:
        ``patterns`` uint8 and ``combo_score`` fp32; ``order`` int64, the
        findings with a pattern by combo_score descending, then finding index
        ascending, the first ``k`` (all with ``k=None``).  Under ``vulns``
        the arrays of ``cpu_ref.TOXIC_VULN_KEYS`` per matched advisory, the
        first ``k`` in the order max_score descending, n_agents descending,
        vuln ascending.  ``pkg_idx`` and ``win_idx`` are the step's,
        ``vuln_of`` the map on the device or None, for
        ``toxic_combos.estate_combinations``.  ``poison_servers`` int32 node
        ids, ascending;
        ``n_by_pattern`` int64 [6]; and as ints ``n_vulns`` (matched
        advisories) and ``n_multi_agent``.  On the GPU from the kernels of
        ops/csrc/toxic.hip, on the CPU from the oracle.  Calls :meth:`step`
        when ``step_res`` is None."""
        torch = self.torch
        from agentbom_amd.ops import cpu_ref

        if step_res is None:
            step_res = self.step()
        caps, table, poison = self._toxic_caps(tool_caps)
        vmap, n_vulns = self._toxic_vuln_of(vuln_of)
        pkg_idx, win_idx, scores = step_res["pkg_idx"], step_res["win_idx"], step_res["scores"]
        if self.use_gpu:
            from agentbom_amd.ops import native

            res = native.toxic_combinations(
                pkg_idx.contiguous(), win_idx.contiguous(), scores.contiguous(),
                step_res["n_creds"].contiguous(), self.arena, self.tool_lut, table, self.rev,
                self.reach_index, ET_CONTAINS, self.estate.pkg_base, vuln_of=vmap,
                n_vulns=n_vulns, workspace=self._toxic_ws)
            patterns, combo, per = res["patterns"], res["combo_score"], res["vulns"]
            # a finding with a pattern scores above 0, one without scores 0:
            # the stable descending sort puts the flagged ones first, by index
            order = torch.argsort(combo, descending=True, stable=True)[:res["n_flagged"]]
            # stable sorts from the last key up; positions are in vuln order
            v_order = torch.argsort(per["n_agents"], descending=True, stable=True)
            v_order = v_order[torch.argsort(per["max_score"][v_order], descending=True,
                                            stable=True)]
            n_by_pattern = torch.tensor(res["n_by_pattern"], dtype=torch.int64).to(self.device)
            n_multi = res["n_multi_agent"]
        else:
            ref = cpu_ref.toxic_combinations(
                pkg_idx.numpy(), win_idx.numpy(), scores.numpy(), step_res["n_creds"].numpy(),
                step_res["n_tools"].numpy(),
                self.rev["row_off"].numpy(), self.rev["col"].numpy(), self.rev["etype"].numpy(),
                self.fwd["row_off"].numpy(), self.fwd["col"].numpy(), self.fwd["etype"].numpy(),
                ET_CONTAINS, ET_USES, ET_PROVIDES_TOOL, self.estate.pkg_base,
                self.arena["severity"].numpy(), self.arena["kev"].numpy(),
                self.arena["impact"].numpy(), self.tool_lut.numpy(), self.estate.tool_base,
                self.tool_is_db.numpy(), caps.numpy(),
                None if vmap is None else vmap.numpy())
            patterns = torch.from_numpy(ref["patterns"])
            combo = torch.from_numpy(ref["combo_score"])
            per = {key: torch.from_numpy(ref["vulns"][key]) for key in cpu_ref.TOXIC_VULN_KEYS}
            flagged = torch.nonzero(patterns).flatten()
            order = flagged[torch.argsort(combo[flagged], descending=True, stable=True)]
            v_order = torch.from_numpy(ref["vulns"]["order"])
            poison = torch.from_numpy(ref["poison_servers"])
            n_by_pattern = torch.from_numpy(ref["n_by_pattern"])
            n_multi = ref["n_multi_agent"]
        n_matched = v_order.numel()
        if k is not None:
            order, v_order = order[:max(int(k), 0)], v_order[:max(int(k), 0)]
        return {"patterns": patterns, "combo_score": combo, "order": order,
                "pkg_idx": pkg_idx, "win_idx": win_idx, "vuln_of": vmap,
                "vulns": {key: value[v_order] for key, value in per.items()},
                "poison_servers": poison, "n_by_pattern": n_by_pattern,
                "n_vulns": n_matched, "n_multi_agent": n_multi}

    def _score_cpu(self, counts, pos, pkg_nodes, win_idx, dist):
        """CPU oracle of the fused score_gather kernel: (scores, n_agents,
        n_creds, n_tools) per finding."""
        torch = self.torch
        n_findings = win_idx.numel()
        # CWE-impact filtering via LUTs: 2=full, 1=db-only, 0=none
        impact = self.arena["impact"].to(torch.int64)[win_idx]
        cred_cls = self.cred_lut.to(torch.int64)[impact]
        tool_cls = self.tool_lut.to(torch.int64)[impact]
        n_creds = torch.where(
            cred_cls == 2, counts["n_creds_all"][pos],
            torch.where(cred_cls == 1, counts["n_creds_db"][pos],
                        torch.zeros_like(pos, dtype=torch.int32)),
        )
        n_tools = torch.where(
            tool_cls == 2, counts["n_tools_all"][pos],
            torch.where(tool_cls == 1, counts["n_tools_db"][pos],
                        torch.zeros_like(pos, dtype=torch.int32)),
        )
        n_agents = counts["n_agents"][pos]

        sev = self.arena["severity"][win_idx]
        kev = self.arena["kev"][win_idx]
        epss = self.arena["epss"][win_idx]
        flags = (kev.to(torch.uint8) << 1)  # bit1 kev; no ai_ctx/suppressed in synth
        scorecard = torch.full((n_findings,), -1.0, dtype=torch.float32, device=self.device)
        # dist is int32 with UNVISITED as the -1 bit pattern (comparing the
        # u32 literal would promote to int64 and never match)
        reach_known = dist[pkg_nodes] != -1
        reach = reach_known.to(torch.int8)

        from agentbom_amd.ops import cpu_ref

        scores = torch.from_numpy(
            cpu_ref.risk_score(
                sev.numpy(), n_agents.numpy().astype(np.uint32),
                n_creds.numpy().astype(np.uint32), n_tools.numpy().astype(np.uint32),
                flags.numpy(), epss.numpy(), scorecard.numpy(), reach.numpy(),
            )
        )
        return scores, n_agents, n_creds, n_tools

    def rollup(self, step_res=None):
        """Estate CONTAINS-tree collapse on device.

        The estate tree is two levels (agent -> server -> package), so the
        collapse is two segmented reductions kept on the GPU: per-server
        severity histograms over contained findings (severity_histogram
        HIP kernel on the GPU path), then index_add-merged up the USES
        edges into per-agent aggregates.  Returns device tensors:
        histograms [n,6] (codes 5..0 mapped to columns 0..5), worst code,
        finding counts — the estate-scale analog of graph/rollup.py's
        Python CONTAINS walk (reference graph/rollup.py:313-580).
        """
        torch = self.torch
        est = self.estate
        if step_res is None:
            step_res = self.step()
        win_idx = step_res["win_idx"].to(torch.int64)
        sev_code = self.arena["severity"].to(torch.int64)[win_idx]  # 5..1
        sev_col = (5 - sev_code).clamp(0, 5)  # 0=critical .. 5=unknown
        pkg_nodes = (step_res["pkg_idx"] + est.pkg_base).to(torch.int64)

        # finding -> containing servers (reverse CONTAINS), severity carried
        uniq = torch.unique(pkg_nodes)
        pos_of_uniq = torch.arange(uniq.numel(), device=self.device)
        srv, carry = self._expand(self.rev, uniq, pos_of_uniq, ET_CONTAINS)
        # distinct (package, server): duplicate CONTAINS edges count once
        pair = torch.unique((carry << 32) | srv)
        carry = pair >> 32
        srv = pair & 0xFFFFFFFF
        # map each (finding) to each server containing its package
        fpos = torch.searchsorted(uniq, pkg_nodes)
        # (uniq_pos -> servers) join back onto findings: build per-uniq run
        order = torch.argsort(carry, stable=True)
        srv_sorted = srv[order]
        carry_sorted = carry[order]
        run_counts = torch.bincount(carry_sorted, minlength=uniq.numel())
        run_off = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(run_counts, 0, out=run_off[1:])
        cnt_f = run_counts[fpos]
        rep = torch.repeat_interleave(
            torch.arange(pkg_nodes.numel(), device=self.device), cnt_f)
        ends = torch.cumsum(cnt_f, 0)
        base = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device),
                          ends[:-1]])
        within = torch.arange(int(ends[-1].item()) if ends.numel() else 0,
                              device=self.device) - base[rep]
        srv_per = srv_sorted[run_off[fpos[rep]] + within]
        sev_per = sev_col[rep]

        srv_local = (srv_per - est.server_base).to(torch.int64)
        if self.use_gpu:
            from agentbom_amd.ops import native

            # the histogram kernel reads u32 owner indices
            srv_hist = native.severity_histogram(
                srv_local.to(torch.int32).contiguous(),
                sev_per.to(torch.uint8).contiguous(), est.n_servers)
            srv_hist = srv_hist.to(torch.int64)
        else:
            flat = torch.bincount(srv_local * 6 + sev_per,
                                  minlength=est.n_servers * 6)
            srv_hist = flat.view(est.n_servers, 6)

        # server -> agent merge (reverse USES rows of servers)
        srv_ids = torch.arange(est.n_servers, device=self.device) + est.server_base
        ag, srv_carry = self._expand(self.rev, srv_ids,
                                     torch.arange(est.n_servers, device=self.device),
                                     ET_USES)
        agent_hist = torch.zeros(est.n_agents, 6, dtype=torch.int64,
                                 device=self.device)
        agent_hist.index_add_(0, ag, srv_hist[srv_carry])

        def worst_of(hist):
            has = hist > 0
            first = torch.argmax(has.to(torch.int8), dim=1)
            any_f = has.any(dim=1)
            return torch.where(any_f, first, torch.full_like(first, 6))

        return {
            "server_hist": srv_hist, "agent_hist": agent_hist,
            "server_worst": worst_of(srv_hist), "agent_worst": worst_of(agent_hist),
            "server_findings": srv_hist.sum(dim=1),
            "agent_findings": agent_hist.sum(dim=1),
        }

    # ── attack / exposure paths (GPU path DP) ──────────────────────────────

    ET_LATERAL = 4  # reversed USES edge (server -> agent): lateral movement

    def _path_edges(self):
        """Edge arrays for the path DP: forward edges + reversed USES edges
        (lateral movement via shared servers).  Cached device tensors."""
        cached = getattr(self, "_path_edges_cache", None)
        if cached is not None:
            return cached
        torch = self.torch
        est = self.estate
        uses = est.edge_type == ET_USES
        src = np.concatenate([est.edge_src, est.edge_dst[uses]])
        dst = np.concatenate([est.edge_dst, est.edge_src[uses]])
        et = np.concatenate([est.edge_type,
                             np.full(int(uses.sum()), self.ET_LATERAL, dtype=np.uint8)])
        dev = self.device
        cached = (
            torch.from_numpy(src).to(device=dev, dtype=torch.int32),
            torch.from_numpy(dst).to(device=dev, dtype=torch.int32),
            torch.from_numpy(et).to(device=dev, dtype=torch.uint8),
        )
        self._path_edges_cache = cached
        return cached

    def attack_paths(self, step_res=None, k: int = 100, max_depth: int = 6):
        """Top-k attack/exposure paths over the estate (HIP path DP).

        Entry class: agents.  Crown jewels: credentials and tools.  Gate:
        the path must traverse a server that contains a matched-vulnerable
        package (the estate analog of the vulnerable_to/exploitable_via
        edge gate in graph/attack_paths.py).  Node boosts mirror
        _node_boost: vulnerable +1.5, severity map, KEV +2.0.
        Replaces the reference's DFS at estate scale
        (src/agent_bom/graph/attack_path_fusion.py:194).
        """
        from agentbom_amd.graph.path_engine import run_path_dp

        torch = self.torch
        est = self.estate
        if step_res is None:
            step_res = self.step()

        pkg_nodes = (step_res["pkg_idx"] + est.pkg_base).to(torch.int64)
        win_idx = step_res["win_idx"].to(torch.int64)
        sev = self.arena["severity"].to(torch.int64)[win_idx]
        kev = self.arena["kev"].to(torch.int64)[win_idx]
        sev_boost = torch.zeros_like(sev, dtype=torch.float32)
        sev_boost[sev == 5] = 2.0   # critical
        sev_boost[sev == 4] = 1.2   # high
        sev_boost[sev == 3] = 0.6   # medium
        boost = 1.5 + sev_boost + kev.to(torch.float32) * 2.0

        node_boost = torch.zeros(self.N, dtype=torch.float32, device=self.device)
        node_boost.scatter_reduce_(0, pkg_nodes, boost, reduce="amax")

        # gated servers: contain >= 1 matched package; server boost = the
        # best boost among its matched packages (compromise value)
        uniq = torch.unique(pkg_nodes)
        pos = torch.arange(uniq.numel(), device=self.device)
        srv, carry = self._expand(self.rev, uniq, pos, ET_CONTAINS)
        node_gate = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        if srv.numel():
            node_gate[srv] = 1
            pkg_best = torch.zeros(uniq.numel(), dtype=torch.float32, device=self.device)
            pkg_best.scatter_reduce_(0, torch.searchsorted(uniq, pkg_nodes),
                                     boost, reduce="amax")
            node_boost.scatter_reduce_(0, srv, pkg_best[carry], reduce="amax")

        etype_boost = np.zeros(256, dtype=np.float32)
        etype_boost[ET_USES] = 0.3
        etype_boost[ET_CONTAINS] = 0.3
        etype_boost[ET_HAS_CRED] = 1.5       # exposes_cred class
        etype_boost[ET_PROVIDES_TOOL] = 0.3
        etype_boost[self.ET_LATERAL] = 1.0   # shares_server class
        etype_trav = np.zeros(256, dtype=np.uint8)
        etype_trav[[ET_USES, ET_CONTAINS, ET_HAS_CRED, ET_PROVIDES_TOOL,
                    self.ET_LATERAL]] = 1
        etype_gate = np.zeros(256, dtype=np.uint8)

        target_mask = np.zeros(self.N, dtype=np.uint8)
        target_mask[est.cred_base:est.cred_base + est.n_creds] = 1
        target_mask[est.tool_base:est.tool_base + est.n_tools] = 1

        src, dst, et = self._path_edges()
        return run_path_dp(
            src, dst, et, None, self.N, self.agent_ids.to(torch.int64),
            node_boost, etype_boost, etype_trav, etype_gate, node_gate,
            target_mask, max_depth=max_depth, k=k,
            device=self.device if self.use_gpu else None,
        )

    def enable_query_graph(self, batch: int = 1, max_hops: int = 4,
                           max_nodes: int = 4096) -> None:
        """Capture the blast-radius query into a hipGraph for serving.

        One capture per (batch, max_hops, max_nodes) shape: the kernel launch
        sequence is recorded once against static in/out buffers; each query
        then copies ids into the static input and REPLAYS the graph — no
        per-query launch construction on the hot path (the serving analog of
        capturing launch-bound inner loops in hipGraphs).
        """
        torch = self.torch
        from agentbom_amd.ops import native

        dev = self.device
        q_in = torch.zeros(batch, dtype=torch.int32, device=dev)
        out_nodes = torch.empty((batch, max_nodes), dtype=torch.int32, device=dev)
        out_hops = torch.empty((batch, max_nodes), dtype=torch.uint8, device=dev)
        out_counts = torch.zeros(batch, dtype=torch.int32, device=dev)
        out_trunc = torch.zeros(batch, dtype=torch.uint8, device=dev)

        def _launch():
            # with ``out`` given this is the single abom_impact_query launch
            native.impact_query(
                self.rev["row_off"], self.rev["col"], q_in, etype=None,
                allowed_mask=0xFFFFFFFF, max_hops=max_hops, max_nodes=max_nodes,
                out=(out_nodes, out_hops, out_counts, out_trunc))

        # warmup on a side stream, then capture
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _launch()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _launch()
        self._query_graph = {
            "graph": graph, "batch": batch, "max_hops": max_hops,
            "max_nodes": max_nodes, "q_in": q_in, "out_nodes": out_nodes,
            "out_hops": out_hops, "out_counts": out_counts,
            "out_trunc": out_trunc,
        }

    def blast_radius_query(self, node_ids, max_hops: int = 4, max_nodes: int = 4096):
        """Bounded blast-radius neighborhoods (reverse direction: who reaches
        this package / what this vuln exposes)."""
        q = node_ids.to(self.torch.int32)
        if self.use_gpu:
            g = getattr(self, "_query_graph", None)
            if (g is not None and q.numel() == g["batch"]
                    and max_hops == g["max_hops"]
                    and max_nodes == g["max_nodes"]):
                # the kernel fully writes counts/truncated per query, so
                # replay needs only the input copy
                g["q_in"].copy_(q.to(self.device))
                g["graph"].replay()
                return (g["out_nodes"], g["out_hops"], g["out_counts"],
                        g["out_trunc"])
            from agentbom_amd.ops import native

            return native.impact_query(
                self.rev["row_off"], self.rev["col"], q, etype=None,
                allowed_mask=0xFFFFFFFF, max_hops=max_hops, max_nodes=max_nodes,
            )
        from agentbom_amd.ops import cpu_ref

        torch = self.torch
        results = cpu_ref.impact_query(
            self.rev["row_off"].numpy(), self.rev["col"].numpy(), q.numpy(),
            max_hops=max_hops, max_nodes=max_nodes,
        )
        Q = q.numel()
        out_nodes = torch.zeros((Q, max_nodes), dtype=torch.int32)
        out_hops = torch.zeros((Q, max_nodes), dtype=torch.uint8)
        out_counts = torch.zeros(Q, dtype=torch.int32)
        out_trunc = torch.zeros(Q, dtype=torch.uint8)
        for qi, (hops, trunc) in enumerate(results):
            items = list(hops.items())[:max_nodes]
            for j, (node, hop) in enumerate(items):
                out_nodes[qi, j] = node
                out_hops[qi, j] = hop
            out_counts[qi] = len(items)
            out_trunc[qi] = 1 if trunc else 0
        return out_nodes, out_hops, out_counts, out_trunc

    # ── centrality on the resident estate (ops/csrc/centrality.hip) ────────

    def _centrality_ws(self) -> dict:
        ws = getattr(self, "_cen_ws", None)
        if ws is None:
            ws = self._cen_ws = {}
        return ws

    def pagerank(self, damping: float = 0.85, iterations: int = 50):
        """PageRank over every estate edge; fp64 tensor [N] on the engine's
        device.  Dangling mass (packages, credentials, tools) is spread
        uniformly, as in graph/backend.py."""
        torch = self.torch
        out_degree = (self.fwd["row_off"][1:] - self.fwd["row_off"][:-1]).to(torch.int32)
        if self.use_gpu:
            from agentbom_amd.ops import native

            return native.pagerank(self.rev["row_off"], self.rev["col"], out_degree, self.N,
                                   damping=damping, iterations=iterations,
                                   workspace=self._centrality_ws())
        from agentbom_amd.ops import cpu_ref

        return torch.from_numpy(cpu_ref.pagerank(
            self.rev["row_off"].numpy(), self.rev["col"].numpy(), out_degree.numpy(),
            self.N, damping=damping, iterations=iterations))

    def betweenness(self, sample: int = 64, allowed_mask: Optional[int] = None):
        """Brandes betweenness from the deterministic source sample of
        graph/backend.py (exact when ``sample >= N``), divided by
        (N-1)(N-2); fp64 tensor [N].  ``allowed_mask`` keeps only the edge
        types whose bit is set (None walks every edge)."""
        from agentbom_amd.graph.backend import brandes_sources

        torch = self.torch
        n = self.N
        if n < 3:
            return torch.zeros(n, dtype=torch.float64, device=self.device)
        sources = brandes_sources(n, sample)
        if self.use_gpu:
            from agentbom_amd.ops import native

            bc = native.betweenness(self.fwd, self.rev, n, sources,
                                    workspace=self._centrality_ws(),
                                    allowed_mask=allowed_mask)
        else:
            from agentbom_amd.ops import cpu_ref

            masked = allowed_mask is not None
            bc = torch.from_numpy(cpu_ref.betweenness(
                self.fwd["row_off"].numpy(), self.fwd["col"].numpy(), n, sources,
                etype=self.fwd["etype"].numpy() if masked else None,
                allowed_mask=allowed_mask if masked else 0xFFFFFFFF))
        return bc / float((n - 1) * (n - 2))

    # ── segmentation on the resident estate (ops/csrc/components.hip) ──────

    # node classes of lateral_domains, in estate id-range order
    KIND_AGENT, KIND_SERVER, KIND_CRED, KIND_TOOL, KIND_PACKAGE = range(5)

    def components(self, allowed_mask: Optional[int] = None):
        """Weakly connected components of the estate; int32 tensor [N] on the
        engine's device, each node labelled with the smallest node id of its
        component.  ``allowed_mask`` keeps only the edge types whose bit is
        set (None joins over every edge); direction is ignored."""
        masked = allowed_mask is not None
        if self.use_gpu:
            from agentbom_amd.ops import native

            return native.connected_components(
                self.fwd["src"], self.fwd["col"], self.N,
                etype=self.fwd["etype"] if masked else None,
                allowed_mask=allowed_mask, workspace=self._centrality_ws())
        from agentbom_amd.ops import cpu_ref

        return self.torch.from_numpy(cpu_ref.connected_components(
            self.fwd["src"].numpy(), self.fwd["col"].numpy(), self.N,
            etype=self.fwd["etype"].numpy() if masked else None,
            allowed_mask=allowed_mask if masked else 0xFFFFFFFF))

    def _node_kind(self):
        """uint8 [N]: the KIND_* class of every node, from the id ranges."""
        kind = getattr(self, "_node_kind_cache", None)
        if kind is None:
            est = self.estate
            bounds = self.torch.tensor(
                [est.server_base, est.cred_base, est.tool_base, est.pkg_base],
                device=self.device)
            kind = self.torch.bucketize(
                self.torch.arange(self.N, device=self.device), bounds,
                right=True).to(self.torch.uint8)
            self._node_kind_cache = kind
        return kind

    def lateral_domains(self, step_res=None, k: int = 20,
                        allowed_mask: int = (1 << ET_USES) | (1 << ET_HAS_CRED)):
        """Lateral-movement domains: the components under ``allowed_mask``
        (by default agents, servers and credentials tied together through
        USES and HAS_CRED edges) that contain at least one agent, with their
        findings rolled up.

        A domain's findings are the sum of ``rollup(step_res)
        ["server_findings"]`` over its servers and its worst severity the
        minimum of their ``server_worst`` column (0 = critical .. 6 = none).
        A package contained by several servers of one domain therefore
        counts once per server, exactly as in :meth:`rollup`.

        Returns device tensors over the domains, ordered by descending
        findings, ties by ascending root, truncated to ``k``: ``root`` (the
        component label), ``agents``, ``servers``, ``creds`` (int32),
        ``findings`` (int64), ``worst`` (int32); and the scalars
        ``n_domains`` (before truncation) and ``largest_agents``.
        """
        torch = self.torch
        est = self.estate
        labels = self.components(allowed_mask)
        # dense renumbering of the roots, ascending by root id
        is_root = labels == torch.arange(self.N, dtype=torch.int32, device=self.device)
        dense = torch.cumsum(is_root, 0, dtype=torch.int32) - 1
        comp = dense[labels.to(torch.int64)].contiguous()
        roots = torch.nonzero(is_root).flatten()
        n_comp = int(roots.numel())

        roll = self.rollup(step_res)
        servers = slice(est.server_base, est.server_base + est.n_servers)
        weight = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        weight[servers] = roll["server_findings"].to(torch.int32)
        worst = torch.full((self.N,), 6, dtype=torch.uint8, device=self.device)
        worst[servers] = roll["server_worst"].to(torch.uint8)
        kind = self._node_kind()
        if self.use_gpu:
            from agentbom_amd.ops import native

            kind_counts, findings, worst_min = native.component_stats(
                comp, kind, n_comp, 5, weight=weight, worst=worst)
        else:
            from agentbom_amd.ops import cpu_ref

            kind_counts, findings, worst_min = (torch.from_numpy(a) for a in (
                cpu_ref.component_stats(comp.numpy(), kind.numpy(), n_comp, 5,
                                        weight=weight.numpy(), worst=worst.numpy())))

        sel = torch.nonzero(kind_counts[:, self.KIND_AGENT] > 0).flatten()
        agents = kind_counts[sel, self.KIND_AGENT]
        # stable: equal findings stay in ascending-root order
        _neg, order = torch.sort(-findings[sel], stable=True)
        top = sel[order[:k]]
        return {
            "root": roots[top].to(torch.int32),
            "agents": kind_counts[top, self.KIND_AGENT],
            "servers": kind_counts[top, self.KIND_SERVER],
            "creds": kind_counts[top, self.KIND_CRED],
            "findings": findings[top],
            "worst": worst_min[top],
            "n_domains": int(sel.numel()),
            "largest_agents": int(agents.max().item()) if sel.numel() else 0,
        }

    def choke_points(self, k: int = 20, sample: int = 64):
        """The k nodes most shortest paths funnel through: (node_ids int64 [k],
        scores fp64 [k]) by descending betweenness, ties by ascending id."""
        scores = self.betweenness(sample=sample)
        # a stable ascending sort of the negated scores keeps equal scores
        # in ascending-id order
        _neg, order = self.torch.sort(-scores, stable=True)
        top = order[:k]
        return top, scores[top]
