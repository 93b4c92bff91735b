"""ctypes bindings for the gfx950 HIP engine (_abom_gpu.so).

Tensors are allocated and owned by PyTorch (the caching allocator manages
HBM); raw device pointers + the current torch HIP stream are handed to the
C ABI.  On a machine with a visible GPU the native library is REQUIRED —
a missing .so raises instead of silently falling back to a slow path
(AGENT_BOM_GPU_REQUIRED=0 opts out for CPU-only dev boxes).
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

import numpy as np

_SO_PATH = Path(__file__).resolve().parent / "_abom_gpu.so"
_lib: Optional[ctypes.CDLL] = None

_c = ctypes.c_void_p      # void* / const void*
_i64 = ctypes.c_longlong  # long long
_u32 = ctypes.c_uint      # unsigned int
_i32 = ctypes.c_int       # int
_f64 = ctypes.c_double    # double
_fp = ctypes.POINTER(ctypes.c_float)  # const float*

# The C ABI as ctypes (argtypes, restype): one entry per prototype of
# csrc/abom_api.h, one row per line of that prototype, arguments in order.
# tests/test_native_abi.py asserts the two agree.
_SIGNATURES = {
    "abom_abi_version": ([], _i32),
    "abom_device_count": ([], _i32),
    "abom_error_string": ([_i32], ctypes.c_char_p),
    "abom_match": ([
        _c, _c, _c,        # pkg_group_key, pkg_key_hi, pkg_key_lo
        _c, _i64,          # pkg_flags, num_packages
        _c, _c, _i64,      # group_keys, group_off, num_groups
        _c, _c, _c, _c,    # w_intro_hi, w_intro_lo, w_fixed_hi, w_fixed_lo
        _c, _c, _c, _c,    # w_last_hi, w_last_lo, w_flags, w_packed
        _c, _c, _c,        # pkg_wbeg, pkg_wend, p_order
        _c, _c, _i64, _c,  # out_pairs, out_count, capacity, stream
    ], _i32),
    "abom_match_by_window": ([
        _c, _c, _c, _c,    # w_intro_hi, w_intro_lo, w_fixed_hi, w_fixed_lo
        _c, _c, _c,        # w_last_hi, w_last_lo, w_flags
        _c, _c, _i64,      # w_rbeg, w_rend, num_windows
        _c, _c,            # s_key, s_row
        _c, _c, _i64, _c,  # out_pairs, out_count, capacity, stream
    ], _i32),
    "abom_match_by_window_tiled": ([
        _c, _c, _c, _c,    # w_intro_hi, w_intro_lo, w_fixed_hi, w_fixed_lo
        _c, _c, _c,        # w_last_hi, w_last_lo, w_flags
        _c, _c, _i64,      # w_rbeg, w_rend, num_windows
        _c, _c,            # s_key, s_row
        _c, _c, _i64, _c,  # out_pairs, out_count, capacity, stream
    ], _i32),
    "abom_bfs_expand": ([
        _c, _c, _c, _u32,    # row_off, col, etype, allowed_mask
        _c, _i64, _c, _u32,  # frontier, frontier_size, dist, next_level
        _c, _c, _c, _c,      # next_frontier, next_count, heavy_queue, heavy_count
        _c, _i64, _c,        # next_degree_sum, capacity, stream
    ], _i32),
    "abom_bfs_expand_heavy": ([
        _c, _c, _c, _u32,  # row_off, col, etype, allowed_mask
        _c, _c, _c, _u32,  # heavy_queue, heavy_size_ptr, dist, next_level
        _c, _c, _c, _i64,  # next_frontier, next_count, next_degree_sum, capacity
        _c,                # stream
    ], _i32),
    "abom_bfs_expand_edges": ([
        _c, _c, _c, _u32,    # edge_src, col, etype, allowed_mask
        _i64, _c, _c, _u32,  # num_edges, row_off, dist, cur_level
        _c, _c, _c, _i32,    # next_frontier, next_count, next_degree_sum, build_frontier
        _i64, _c,            # capacity, stream
    ], _i32),
    "abom_bfs_run": ([
        _c, _c, _c, _u32,      # row_off, col, etype, allowed_mask
        _c, _i64, _c, _i64,    # sources, n_sources, dist, num_nodes
        _c, _c, _c, _c,        # frontier_a, frontier_b, heavy_queue, counters
        _i32, _c, _i64, _f64,  # max_levels, edge_src, num_edges, avg_degree
        _c, _c, _c, _c,        # rev_off, rev_col, rev_et, stream
    ], _i32),
    "abom_bfs_begin": ([
        _c, _c, _i64, _c,    # row_off, sources, n_sources, dist
        _i64, _c, _c, _c,    # num_nodes, frontier_a, counters, stream
    ], _i32),
    "abom_bfs_run_ex": ([
        _c, _c, _c, _u32,     # row_off, col, etype, allowed_mask
        _c, _i64, _c, _i64,   # sources, n_sources, dist, num_nodes
        _c, _c, _c, _c,       # frontier_a, frontier_b, heavy_queue, counters
        _i32, _c, _i64,       # max_levels, edge_src, num_edges
        _c, _c, _c,           # rev_off, rev_col, rev_et
        _i32, _i64, _c, _c,   # begun, sources_degree, host_counters, stream
    ], _i32),
    "abom_bfs_parent_index": ([
        _c, _c, _c, _u32,  # rev_off, rev_col, rev_et, allowed_mask
        _i64, _c, _c,      # num_nodes, first_parent, stream
    ], _i32),
    "abom_bfs_bottom_up": ([
        _c, _c, _c, _u32,  # rev_off, rev_col, rev_et, allowed_mask
        _i64, _c, _u32,    # num_nodes, dist, cur_level
        _c, _c, _c,        # next_count, open_count, stream
    ], _i32),
    "abom_bfs_bottom_up_indexed": ([
        _c, _c, _c, _u32,    # rev_off, rev_col, rev_et, allowed_mask
        _i64, _c, _u32, _c,  # num_nodes, dist, cur_level, first_parent
        _c, _c, _c,          # next_count, open_count, stream
    ], _i32),
    "abom_bfs_run_indexed": ([
        _c, _c, _c, _u32,     # row_off, col, etype, allowed_mask
        _c, _i64, _c, _i64,   # sources, n_sources, dist, num_nodes
        _c, _c, _c, _c,       # frontier_a, frontier_b, heavy_queue, counters
        _i32, _c, _i64,       # max_levels, edge_src, num_edges
        _c, _c, _c, _c,       # rev_off, rev_col, rev_et, first_parent
        _i32, _i64, _c, _c,   # begun, sources_degree, host_counters, stream
    ], _i32),
    "abom_reach_hops": ([
        _c, _c, _c, _u32,        # row_off, col, etype, allowed_mask
        _c, _i32, _i32, _i64,    # sources, n_sources, words, num_nodes
        _c, _c, _i64, _i64,      # target_slot, hops, hops_stride, col_base
        _i32,                    # max_depth
        _c, _c, _c, _c, _c, _c,  # seen, cur, nxt, queue_a, queue_b, heavy_queue
        _c, _c, _c,              # counters, host_counters, stream
    ], _i32),
    "abom_impact_query": ([
        _c, _c, _c, _u32,      # row_off, col, etype, allowed_mask
        _c, _i32, _i32, _i32,  # query_sources, num_queries, max_hops, max_nodes_per_query
        _c, _c, _c, _c, _c,    # out_nodes, out_hops, out_counts, out_truncated, stream
    ], _i32),
    "abom_risk_score": ([
        _c, _c, _c, _c,     # severity, n_agents, n_creds, n_tools
        _c, _c, _c, _c,     # flags, epss, scorecard, reach
        _c, _i64, _fp, _c,  # out, n, weights22, stream
    ], _i32),
    "abom_score_gather": ([
        _c, _c, _c,         # win_idx, pkg_nodes, pos
        _c, _c, _c, _c,     # a_sev, a_kev, a_epss, a_impact
        _c, _c, _c,         # cred_lut, tool_lut, counts2d
        _c, _c, _c, _c,     # dist, out_scores, out_agents, out_creds
        _c, _i64, _fp, _c,  # out_tools, n, weights22, stream
    ], _i32),
    "abom_severity_histogram": ([_c, _c, _c, _i64, _c], _i32),  # owner, severity, hist, n, stream
    "abom_blast_counts": ([
        _c, _i64,                # pkgs, n
        _c, _c, _c,              # rev_off, rev_col, rev_et
        _c, _c, _c,              # fwd_off, fwd_col, fwd_et
        _i32, _i32, _i32, _i32,  # et_contains, et_uses, et_cred, et_tool
        _c, _c,                  # node_is_db_cred, node_is_db_tool
        _c, _c, _c,              # out_counts, out_overflow, stream
    ], _i32),
    "abom_blast_counts_indexed": ([
        _c, _i64,            # pkgs, n
        _c, _c, _c, _i32,    # rev_off, rev_col, rev_et, et_contains
        _c, _c, _c,          # reach_off, reach_col, reach_db
        _i64, _i64,          # row_base, num_rows
        _c, _c,              # node_is_db_cred, node_is_db_tool
        _c, _c, _c, _c, _c,  # queue, counters, out_counts, out_overflow, stream
    ], _i32),
    "abom_blast_counts_indexed_sized": ([
        _c, _c, _i64,      # pkgs, n_dev, n_cap
        _c, _c, _c, _i32,  # rev_off, rev_col, rev_et, et_contains
        _c, _c, _c,        # reach_off, reach_col, reach_db
        _i64, _i64,        # row_base, num_rows
        _c, _c,            # node_is_db_cred, node_is_db_tool
        _c, _c, _c,        # queue, counters, host_counters
        _c, _c, _c,        # out_counts, out_overflow, stream
    ], _i32),
    "abom_blast_hops_cap": ([_i32], _i32),  # which
    "abom_blast_hops": ([
        _c, _i64,              # pkgs, n
        _c, _c, _c, _i32,      # rev_off, rev_col, rev_et, et_contains
        _c, _c, _i64, _i64,    # reach_off, reach_col, row_base, num_rows
        _c, _c, _i64, _i32,    # agent_off, agent_srv, num_agents, max_depth
        _c, _c,                # queue, counters
        _c, _c, _c, _c, _c,    # out_hop_agents, out_creds, out_depth, out_overflow, stream
    ], _i32),
    "abom_blast_hops_sized": ([
        _c, _c, _i64,          # pkgs, n_dev, n_cap
        _c, _c, _c, _i32,      # rev_off, rev_col, rev_et, et_contains
        _c, _c, _i64, _i64,    # reach_off, reach_col, row_base, num_rows
        _c, _c, _i64, _i32,    # agent_off, agent_srv, num_agents, max_depth
        _c, _c, _c,            # queue, counters, host_counters
        _c, _c, _c, _c, _c,    # out_hop_agents, out_creds, out_depth, out_overflow, stream
    ], _i32),
    "abom_remediation_cap": ([_i32], _i32),  # which
    "abom_remediation_fold": ([
        _c, _c, _c, _i64,      # pkg_idx, win_idx, scores, num_findings
        _c, _c, _c,            # item_of, a_severity, a_kev
        _c, _c, _c, _c, _c,    # state, matched, counters, host_counters, stream
    ], _i32),
    "abom_remediation_gather": ([
        _c, _i64,              # items, num_items
        _c, _c, _i64,          # pkg_idx, win_idx, num_findings
        _c, _c, _c, _c,        # w_flags, w_fixed_hi, w_fixed_lo, state
        _c, _c, _c, _c,        # out_rep_pkg, out_installs, out_findings, out_vulns
        _c, _c, _c, _c, _c,    # out_score, out_sev, out_kev, out_fix_hi, out_fix_lo
        _c, _c,                # out_unfixed, stream
    ], _i32),
    "abom_remediation_scatter": ([
        _c, _i64, _c, _c,      # pkg_idx, num_findings, item_of, state
        _c, _i64, _i64, _c,    # items_off, num_items, num_installs, csr_pkgs
        _c,                    # stream
    ], _i32),
    "abom_remediation_union": ([
        _c, _i64, _c, _c,        # items, num_items, items_off, csr_pkgs
        _i64,                    # pkg_base
        _c, _c, _c, _i32,        # rev_off, rev_col, rev_et, et_contains
        _c, _c, _i64, _i64,      # reach_off, reach_col, row_base, num_rows
        _i64, _c, _c, _c, _i64,  # node_span, state, queue, pool, pool_slices
        _c, _c,                  # counters, host_counters
        _c, _c, _c, _c, _c,      # out_servers, out_agents, out_creds, out_tools, stream
    ], _i32),
    "abom_toxic_cap": ([_i32], _i32),  # which
    "abom_toxic_server_table": ([
        _c, _c, _i64,          # reach_off, reach_col, num_rows
        _c, _c, _i64, _i64,    # tool_caps, tool_is_db, tool_base, num_tools
        _c, _c,                # table, stream
    ], _i32),
    "abom_toxic_fold": ([
        _c, _c, _c, _c,        # pkg_idx, win_idx, scores, n_creds
        _i64, _c, _i64, _i64,  # num_findings, vuln_of, num_windows, num_vulns
        _c, _c, _c, _c,        # a_severity, a_kev, a_impact, tool_lut
        _c, _c, _c, _i32,      # rev_off, rev_col, rev_et, et_contains
        _i64, _c, _i64, _i64,  # pkg_base, table, row_base, num_rows
        _c, _c, _c, _c, _c,    # state, matched, counters, host_counters, out_patterns
        _c,                    # stream
    ], _i32),
    "abom_toxic_gather": ([
        _c, _i64, _c,          # vulns, num_matched, state
        _c, _c, _c, _c, _c,    # out_findings, out_packages, out_score, out_sev, out_kev
        _c, _c,                # out_patterns, stream
    ], _i32),
    "abom_toxic_scatter": ([
        _c, _c, _i64,          # pkg_idx, win_idx, num_findings
        _c, _i64, _i64, _c,    # vuln_of, num_windows, num_vulns, state
        _c, _i64, _i64, _c,    # vulns_off, num_matched, num_heads, csr_pkgs
        _c,                    # stream
    ], _i32),
    "abom_toxic_union": ([
        _i64, _c, _c, _i64,      # num_matched, vulns_off, csr_pkgs, pkg_base
        _c, _c, _c, _i32,        # rev_off, rev_col, rev_et, et_contains
        _c, _c, _i64, _i64,      # reach_off, reach_col, row_base, num_rows
        _i64, _c, _c, _i64, _c,  # node_span, queue, pool, pool_slices, counters
        _c, _c, _c,              # out_servers, out_agents, stream
    ], _i32),
    "abom_toxic_finish": ([
        _c, _c, _c, _i64,      # pkg_idx, win_idx, scores, num_findings
        _c, _i64, _i64,        # vuln_of, num_windows, num_vulns
        _c, _i64, _c,          # vulns, num_matched, state
        _c, _c, _c,            # v_agents, v_score, v_patterns
        _c, _c, _c, _c, _c,    # patterns, combo_score, counters, host_counters, stream
    ], _i32),
    "abom_path_relax": ([
        _c, _c, _c, _c,  # edge_src, col, etype, edge_weight
        _c, _c, _c, _c,  # cur, nxt, node_boost, etype_boost
        _c, _c, _c,      # etype_trav, etype_gate, node_gate
        _i64, _c,        # num_edges, stream
    ], _i32),
    "abom_rank_order": ([
        _c, _i64, _c, _c, _i32,  # scores, n, hist, bin_scratch, nblocks
        _c, _c,                  # order, stream
    ], _i32),
    "abom_findings_count": ([
        _c, _c, _i64,        # pairs, count, capacity
        _c, _c, _c,          # run_off, perm2, row_of
        _i64, _i64,          # num_rows, num_packages
        _c, _c, _c, _c,      # bitmap, row_cnt, row_tail, chain_prev
        _c, _c, _c, _c, _c,  # rank_of, word_f, block_sums, totals, stream
    ], _i32),
    "abom_findings_emit": ([
        _c, _c, _i64,     # pairs, count, capacity
        _c, _i64, _i64,   # row_of, num_rows, num_packages
        _c, _c, _c, _c,   # bitmap, row_cnt, row_tail, chain_prev
        _c, _c, _c,       # rank_of, word_f, block_off
        _i64, _i64, _i64,  # pkg_base, num_findings, num_unique
        _c, _c, _c, _c,   # out_pkg_idx, out_win_idx, out_pkg_nodes, out_pos
        _c, _c, _c,       # out_uniq64, out_uniq32, stream
    ], _i32),
    "abom_findings_emit_sized": ([
        _c, _c, _i64,         # pairs, count, capacity
        _c, _i64, _i64,       # row_of, num_rows, num_packages
        _c, _c, _c, _c,       # bitmap, row_cnt, row_tail, chain_prev
        _c, _c, _c,           # rank_of, word_f, block_off
        _i64, _c, _i64, _i64,  # pkg_base, totals, findings_cap, unique_cap
        _c,                   # num_sized
        _c, _c, _c, _c,       # out_pkg_idx, out_win_idx, out_pkg_nodes, out_pos
        _c, _c, _c,           # out_uniq64, out_uniq32, stream
    ], _i32),
    "abom_findings_ahead": ([
        _c, _c, _i64,          # pairs, count, capacity
        _c, _c, _c,            # run_off, perm2, row_of
        _i64, _i64,            # num_rows, num_packages
        _c, _c, _c, _c,        # bitmap, row_cnt, row_tail, chain_prev
        _c, _c, _c, _c, _c,    # rank_of, word_f, block_sums, totals, host_totals
        _i64, _i64, _i64, _c,  # pkg_base, findings_cap, unique_cap, num_sized
        _c, _c, _c, _c,        # out_pkg_idx, out_win_idx, out_pkg_nodes, out_pos
        _c, _c,                # out_uniq64, out_uniq32
        _c, _c, _c, _i32,      # rev_off, rev_col, rev_et, et_contains
        _c, _c, _c,            # reach_off, reach_col, reach_db
        _i64, _i64,            # row_base, reach_rows
        _c, _c,                # node_is_db_cred, node_is_db_tool
        _c, _c, _c,            # queue, counters, host_counters
        _c, _c, _c,            # out_counts, out_overflow, stream
    ], _i32),
    "abom_pagerank_run": ([
        _c, _c, _c, _i64,      # rev_off, rev_col, rev_heavy, num_rev_heavy
        _c, _i64, _f64, _f64,  # out_degree, num_nodes, damping, tolerance
        _i32, _c, _c, _c, _c,  # iterations, rank_a, rank_b, contrib_a, contrib_b
        _c, _c, _c,            # partials, scalars, stream
    ], _i32),
    "abom_brandes_run": ([
        _c, _c, _c,            # fwd_off, fwd_col, fwd_et
        _c, _c, _c, _u32,      # rev_off, rev_col, rev_et, allowed_mask
        _c, _i64,              # fwd_heavy, num_fwd_heavy
        _c, _i64,              # rev_heavy, num_rev_heavy
        _c, _i32, _i64,        # sources, batch, num_nodes
        _c, _c, _c, _c, _c, _c,  # dist, sigma, delta, bc, counter, stream
    ], _i32),
    "abom_components_run": ([
        _c, _c, _c, _u32,    # edge_src, col, etype, allowed_mask
        _i64, _i64, _c, _c,  # num_edges, num_nodes, labels, counters
        _i32, _c,            # max_rounds, stream
    ], _i32),
    "abom_component_stats": ([
        _c, _c, _c, _c,    # comp, kind, weight, worst
        _i64, _i64, _i32,  # num_nodes, num_components, num_kinds
        _c, _c, _c, _c,    # kind_counts, weight_sum, worst_min, stream
    ], _i32),
}

# Byte offsets into the BFS ``counters`` buffer (u32 slots of csrc/bfs.hip)
_CTR_NEXT, _CTR_HEAVY, _CTR_DEGREE, _CTR_OPEN = 0, 4, 8, 12
_CTR_SLOTS = 4

# Rows with at least this many scanned edges get one wave instead of one
# thread in the centrality kernels (CENTRALITY_HEAVY_DEGREE, csrc/centrality.hip)
CENTRALITY_HEAVY_DEGREE = 64
# PageRank stops after the first pass whose L1 change is below this
PAGERANK_TOLERANCE = 1e-10
# Block partial pairs of the PageRank reduction: both grids are capped at 2048
_PAGERANK_PARTIALS = 2 * 2048
# Bytes of per-source Brandes state per node: dist u32 + sigma f64 + delta f64
_BRANDES_CELL_BYTES = 20
_BRANDES_MAX_BATCH = 64


class NativeUnavailable(RuntimeError):
    pass


def load(required: Optional[bool] = None) -> ctypes.CDLL:
    """Load the engine .so, binding signatures once."""
    global _lib
    if _lib is not None:
        return _lib
    if not _SO_PATH.exists():
        if required is None:
            from agentbom_amd.utils import config as cfg

            required = cfg.GPU_REQUIRED and _torch_has_gpu()
        if required:
            raise NativeUnavailable(
                f"HIP engine missing: {_SO_PATH} not built. Run "
                "`python -m agentbom_amd.ops.build` (requires hipcc). The GPU "
                "path never silently falls back — set AGENT_BOM_GPU_REQUIRED=0 "
                "only on CPU-only development machines."
            )
        raise NativeUnavailable(f"{_SO_PATH} not built")
    lib = ctypes.CDLL(str(_SO_PATH))
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def _torch_has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


def available() -> bool:
    try:
        load(required=False)
        return True
    except NativeUnavailable:
        return False


def _check(rc: int, what: str) -> None:
    if rc != 0:
        lib = load()
        msg = lib.abom_error_string(abs(rc)).decode() if rc else ""
        raise RuntimeError(f"{what} failed: hip error {rc} ({msg})")


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _stream() -> ctypes.c_void_p:
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _buf(ws: dict, key: str, numel: int, dtype, dev, zero: bool = False):
    """Workspace buffer ``ws[key]`` with room for ``numel`` elements: reused
    when large enough, otherwise (re)allocated and stored back."""
    import torch

    t = ws.get(key)
    if t is None or t.numel() < numel:
        t = (torch.zeros if zero else torch.empty)(numel, dtype=dtype, device=dev)
        ws[key] = t
    return t


# ── High-level ops (torch tensors on cuda device) ──────────────────────────


def match_launch(pkg_group_key, pkg_key_hi, pkg_key_lo, pkg_flags, group_keys,
                 group_off, windows: dict, capacity: Optional[int] = None,
                 pkg_win_range=None, order=None) -> dict:
    """Launch the match kernel on the CURRENT stream without syncing.

    Returns a pending handle for :func:`match_finalize`.  Used by the engine
    to overlap the match with the reach BFS on a second HIP stream.
    ``pkg_win_range``: optional (wbeg u32[P], wend u32[P]) precomputed by the
    engine for a resident estate — the kernel then skips the group search.
    """
    import torch

    lib = load()
    P = pkg_group_key.numel()
    if P >= 1 << 32:
        raise ValueError(f"match: {P} packages exceeds the u32 pair encoding; shard the batch")
    G = group_keys.numel()
    cap = capacity or max(1024, P // 4)
    dev = pkg_group_key.device
    out_pairs = torch.empty(cap, dtype=torch.int64, device=dev)
    out_count = torch.zeros(1, dtype=torch.int32, device=dev)
    wbeg_p = wend_p = None
    if pkg_win_range is not None:
        wbeg_p, wend_p = _ptr(pkg_win_range[0]), _ptr(pkg_win_range[1])
    order_p = _ptr(order) if order is not None else None
    rc = lib.abom_match(
        _ptr(pkg_group_key), _ptr(pkg_key_hi), _ptr(pkg_key_lo), _ptr(pkg_flags), P,
        _ptr(group_keys), _ptr(group_off), G,
        _ptr(windows["intro_hi"]), _ptr(windows["intro_lo"]),
        _ptr(windows["fixed_hi"]), _ptr(windows["fixed_lo"]),
        _ptr(windows["last_hi"]), _ptr(windows["last_lo"]),
        _ptr(windows["flags"]),
        _ptr(windows["packed"]) if "packed" in windows else None,
        wbeg_p, wend_p, order_p,
        _ptr(out_pairs), _ptr(out_count), cap, _stream(),
    )
    _check(rc, "abom_match")
    return {"out_pairs": out_pairs, "out_count": out_count, "cap": cap,
            "relaunch": lambda capacity: match_launch(
                pkg_group_key, pkg_key_hi, pkg_key_lo, pkg_flags, group_keys,
                group_off, windows, capacity=capacity,
                pkg_win_range=pkg_win_range, order=order)}


def match_tiled_enabled() -> bool:
    """A/B toggle: AGENT_BOM_MATCH_TILED=0 makes :func:`match_by_window_launch`
    run ``match_by_window_kernel`` (a thread per window probing the search
    table in global memory) instead of ``match_by_window_tiled_kernel``."""
    return os.environ.get("AGENT_BOM_MATCH_TILED", "1") != "0"


def match_by_window_launch(windows: dict, table: dict,
                           capacity: Optional[int] = None) -> dict:
    """Launch the window-per-thread match on the CURRENT stream without
    syncing: every arena window binary-searches the run of its group in the
    row search table (``graph.gpu_engine.build_match_search_table``).  By
    default the block-tiled kernel, which stages each tile's rows in LDS;
    AGENT_BOM_MATCH_TILED=0 (:func:`match_tiled_enabled`) searches global
    memory from a grid-stride thread per window instead.

    Returns the same pending handle as :func:`match_launch`, for
    :func:`match_finalize` and :func:`assemble_findings`; the pairs carry the
    table's ``s_row`` (the row's index in the dedup layout), in no particular
    order.  On overflow the handle relaunches this kernel.
    """
    import torch

    lib = load()
    kernel = lib.abom_match_by_window_tiled if match_tiled_enabled() else lib.abom_match_by_window
    flags = windows["flags"]
    W = flags.numel()
    R = table["s_row"].numel()
    if W >= 1 << 32:
        raise ValueError(f"match: {W} windows exceeds the u32 pair encoding")
    if table["w_rbeg"].numel() != W or table["w_rend"].numel() != W:
        raise ValueError("match: search table was built for another arena")
    cap = capacity or max(1024, R // 4)
    dev = flags.device
    out_pairs = torch.empty(cap, dtype=torch.int64, device=dev)
    out_count = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = kernel(
        _ptr(windows["intro_hi"]), _ptr(windows["intro_lo"]),
        _ptr(windows["fixed_hi"]), _ptr(windows["fixed_lo"]),
        _ptr(windows["last_hi"]), _ptr(windows["last_lo"]), _ptr(flags),
        _ptr(table["w_rbeg"]), _ptr(table["w_rend"]), W,
        _ptr(table["s_key"]), _ptr(table["s_row"]),
        _ptr(out_pairs), _ptr(out_count), cap, _stream(),
    )
    _check(rc, "abom_match_by_window")
    return {"out_pairs": out_pairs, "out_count": out_count, "cap": cap,
            "relaunch": lambda capacity: match_by_window_launch(
                windows, table, capacity=capacity)}


def match_finalize(pending: dict, sort: bool = True):
    """Read the pending match count and produce (pkg_idx, win_idx).

    On capacity overflow (count > cap) the handle's ``relaunch`` runs the
    kernel that filled it again, synchronously, with a grown buffer — rare,
    the launch heuristic is P//4.

    ``sort=False`` skips the canonical (pkg<<32|win) sort — for callers that
    impose their own order downstream (the dedup-expand path re-sorts after
    fanning out to package rows, so sorting the distinct-row pairs here is
    pure waste).
    """
    import torch

    n = int(pending["out_count"].item())
    if n < 0:
        # int32 device counter wrapped: >2^31 candidate matches. Fail loudly
        # rather than slicing with a wrapped count.
        raise RuntimeError("match: device match count overflowed int32; shard the package batch")
    if n > pending["cap"]:
        relaunched = pending["relaunch"](int(n * 1.2) + 1024)
        return match_finalize(relaunched, sort=sort)
    pairs = pending["out_pairs"][:n]
    if sort:
        pairs, _ = torch.sort(pairs)
    return (pairs >> 32).to(torch.int64), (pairs & 0xFFFFFFFF).to(torch.int64)


_FINDINGS_BLOCK = 256  # bitmap words per block (FA_BLOCK, csrc/findings.hip)


def assemble_findings(pending: dict, layout: dict, pkg_base: int, workspace: dict) -> dict:
    """Dedup-match pairs -> the canonical finding stream, without a sort.

    Takes the pending handle of a :func:`match_launch` or
    :func:`match_by_window_launch` over the DISTINCT rows of ``layout`` (``run_off``, ``perm2``, ``row_of``) and returns, equal to
    ``expand_dedup_matches`` + ``unique_consecutive`` + ``searchsorted``:

      pkg_idx, win_idx   int64 [F], sorted by (pkg << 32 | win)
      pkg_nodes          int64 [F] = pkg_idx + pkg_base
      pos                int64 [F], index of the finding's package in uniq_pkgs
      uniq_pkgs          int64 [NU], ascending distinct pkg_nodes
      uniq_pkgs32        int32 [NU], the same (abom_blast_counts input)

    One host read (findings, unique packages, match count) sizes the outputs.
    On capacity overflow the handle relaunches its match with a grown buffer,
    as in :func:`match_finalize`.  ``workspace`` persists between calls and is
    all-zero outside a call; a call that did not finish leaves it flagged and
    the next call clears it in full.

    The call is :func:`assemble_findings_begin` followed by
    :func:`assemble_findings_finish`; a caller with other work to wait for
    runs the first on a side stream behind the match and the second later.
    """
    return assemble_findings_finish(
        assemble_findings_begin(pending, layout, workspace), pkg_base)


def _findings_state(pending: dict, layout: dict, workspace: dict) -> dict:
    """Workspace set-up shared by the begin variants: the buffers of
    csrc/findings.hip sized for this match, cleared if the last call did not
    finish, and flagged dirty.  ``bufs`` is None when there is nothing to do."""
    import torch

    pairs = pending["out_pairs"]
    cap = min(int(pending["cap"]), pairs.numel())
    dev = pairs.device
    run_off, perm2 = layout["run_off"], layout["perm2"]
    U, P = run_off.numel() - 1, perm2.numel()
    state = {"pending": pending, "layout": layout, "ws": workspace, "cap": cap, "bufs": None}
    if P == 0 or cap == 0:
        return state
    ws = workspace
    fresh = []  # allocated in this call, on this stream's pool

    def buf(key, numel, dtype, zero=False):
        before = ws.get(key)
        t = _buf(ws, key, numel, dtype, dev, zero=zero)
        if t is not before:
            fresh.append(t)
        return t

    W = (P + 63) // 64
    nblocks = (W + _FINDINGS_BLOCK - 1) // _FINDINGS_BLOCK
    bitmap = buf("fa_bitmap", W, torch.int64, zero=True)
    row_cnt = buf("fa_row_cnt", U, torch.int32, zero=True)
    row_tail = buf("fa_row_tail", U, torch.int32, zero=True)
    chain_prev = buf("fa_chain_prev", cap, torch.int32)
    rank_of = buf("fa_rank_of", cap, torch.int32)
    word_f = buf("fa_word_f", W, torch.int32)
    block_sums = buf("fa_block_sums", 2 * nblocks, torch.int64)
    # {findings, unique packages, match count} and the sized emit's word
    totals = buf("fa_totals", 4, torch.int64)
    if "fa_host_totals" not in ws:
        # pinned, so the copy of the totals is asynchronous and the read a plain load
        ws["fa_host_totals"] = torch.zeros(3, dtype=torch.int64, pin_memory=True)
        ws["fa_counted"] = torch.cuda.Event()
    if ws.get("fa_dirty"):
        bitmap.zero_()
        row_cnt.zero_()
        row_tail.zero_()
    ws["fa_dirty"] = True
    state.update(bufs=(bitmap, row_cnt, row_tail, chain_prev, rank_of, word_f, block_sums),
                 totals=totals, fresh=fresh, stream=torch.cuda.current_stream(), U=U, P=P)
    return state


def assemble_findings_begin(pending: dict, layout: dict, workspace: dict) -> dict:
    """The count phase of :func:`assemble_findings`, enqueued on the CURRENT
    stream without a host read: workspace set-up, ``abom_findings_count`` and
    a copy of its three totals to pinned host memory.  It needs the match
    pairs and nothing else.  Returns the state that
    :func:`assemble_findings_finish` takes; until that call the workspace is
    flagged dirty."""
    lib = load()
    state = _findings_state(pending, layout, workspace)
    if state["bufs"] is None:
        return state
    ws = workspace
    pairs, count, cap = pending["out_pairs"], pending["out_count"], state["cap"]
    bitmap, row_cnt, row_tail, chain_prev, rank_of, word_f, block_sums = state["bufs"]
    totals = state["totals"]
    rc = lib.abom_findings_count(
        _ptr(pairs), _ptr(count), cap, _ptr(layout["run_off"]), _ptr(layout["perm2"]),
        _ptr(layout["row_of"]), state["U"], state["P"],
        _ptr(bitmap), _ptr(row_cnt), _ptr(row_tail), _ptr(chain_prev),
        _ptr(rank_of), _ptr(word_f), _ptr(block_sums), _ptr(totals), _stream(),
    )
    _check(rc, "abom_findings_count")
    ws["fa_host_totals"].copy_(totals[:3], non_blocking=True)
    ws["fa_counted"].record()
    return state


def findings_ahead_capacity(n: int) -> int:
    """Output capacity :func:`assemble_findings_begin_ahead` allocates for a
    quantity that was ``n`` in the last finished call: a sixteenth of headroom
    and 64 elements, so an estate that grows a little between two calls still
    fits, and one that had nothing still gets room for a first few."""
    n = max(int(n), 0)
    return n + (n >> 4) + 64


def blast_inputs(rev: dict, index: dict, et_contains: int, node_is_db_cred,
                 node_is_db_tool, workspace: dict) -> dict:
    """The arguments of :func:`blast_counts_indexed` other than the packages,
    bundled for :func:`assemble_findings_begin_ahead`."""
    return {"rev": rev, "index": index, "et_contains": int(et_contains),
            "node_is_db_cred": node_is_db_cred, "node_is_db_tool": node_is_db_tool,
            "ws": workspace}


def _blast_host_counters(workspace: dict):
    import torch

    host = workspace.get("host_counters")
    if host is None:
        # pinned: {queued packages, overflowed rows} arrive by an asynchronous copy
        host = workspace["host_counters"] = torch.zeros(2, dtype=torch.int32, pin_memory=True)
    return host


def assemble_findings_begin_ahead(pending: dict, layout: dict, workspace: dict,
                                  pkg_base: int, blast: dict) -> dict:
    """:func:`assemble_findings_begin` that also runs the emit phase and the
    indexed blast counts of the emitted packages on the CURRENT stream, with
    no host read, when the workspace holds a prediction of the output sizes
    (``workspace["fa_ahead_cap"]`` = (findings, unique packages) capacities,
    stored by every finish of such a state, which also leaves in
    ``workspace["fa_ahead_hit"]`` whether it could take the arm's outputs).  The outputs are fresh tensors of
    those capacities; the kernels read the true sizes from the device and do
    nothing if they do not fit.  One call, ``abom_findings_ahead``, enqueues
    it all.  Without a prediction only the count phase runs.  Either way
    :func:`assemble_findings_finish` returns the assembled findings plus
    ``blast_counts`` [NU, 6], ``blast_overflow`` [NU] and
    ``blast_n_overflow``, as :func:`blast_counts_indexed` (``blast``:
    :func:`blast_inputs`) gives for ``uniq_pkgs32``."""
    import torch

    caps = workspace.get("fa_ahead_cap")
    if caps is None:
        state = assemble_findings_begin(pending, layout, workspace)
        state["ahead"] = {"blast": blast, "caps": None}
        return state
    lib = load()
    state = _findings_state(pending, layout, workspace)
    state["ahead"] = {"blast": blast, "caps": None}
    if state["bufs"] is None:
        return state
    ws, bws = workspace, blast["ws"]
    pairs, count, cap = pending["out_pairs"], pending["out_count"], state["cap"]
    dev = pairs.device
    F_cap, NU_cap = int(caps[0]), int(caps[1])
    fresh = state["fresh"]
    # two allocations, not eight: this runs on the host before the BFS loop
    # starts, and every call here delays the first BFS level.  The outputs of
    # one call share the two blocks; those of two calls share nothing.
    blob64 = torch.empty(4 * F_cap + NU_cap, dtype=torch.int64, device=dev)
    blob32 = torch.empty(7 * NU_cap + (NU_cap + 3) // 4, dtype=torch.int32, device=dev)
    out64 = [blob64[k * F_cap:(k + 1) * F_cap] for k in range(4)]
    uniq64 = blob64[4 * F_cap:]
    counts, uniq32 = blob32[:6 * NU_cap], blob32[6 * NU_cap:7 * NU_cap]  # 8-byte rows first
    overflow = blob32[7 * NU_cap:].view(torch.uint8)
    fresh.extend((blob64, blob32))
    for key, numel in (("queue", NU_cap), ("counters", 2)):
        before = bws.get(key)
        if _buf(bws, key, numel, torch.int32, dev) is not before:
            fresh.append(bws[key])
    host_counters = _blast_host_counters(bws)
    bitmap, row_cnt, row_tail, chain_prev, rank_of, word_f, block_sums = state["bufs"]
    totals = state["totals"]
    rev, index = blast["rev"], blast["index"]
    rc = lib.abom_findings_ahead(
        _ptr(pairs), _ptr(count), cap,
        _ptr(layout["run_off"]), _ptr(layout["perm2"]), _ptr(layout["row_of"]),
        state["U"], state["P"],
        _ptr(bitmap), _ptr(row_cnt), _ptr(row_tail), _ptr(chain_prev),
        _ptr(rank_of), _ptr(word_f), _ptr(block_sums), _ptr(totals),
        _ptr(ws["fa_host_totals"]),
        int(pkg_base), F_cap, NU_cap, ctypes.c_void_p(totals.data_ptr() + 24),
        _ptr(out64[0]), _ptr(out64[1]), _ptr(out64[2]), _ptr(out64[3]),
        _ptr(uniq64), _ptr(uniq32),
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), blast["et_contains"],
        _ptr(index["reach_off"]), _ptr(index["reach_col"]), _ptr(index["reach_db"]),
        index["row_base"], index["reach_off"].shape[0],
        _ptr(blast["node_is_db_cred"]), _ptr(blast["node_is_db_tool"]),
        _ptr(bws["queue"]), _ptr(bws["counters"]), _ptr(host_counters),
        _ptr(counts), _ptr(overflow), _stream(),
    )
    _check(rc, "abom_findings_ahead")
    ws["fa_counted"].record()  # behind both host copies
    state["ahead"].update(caps=(F_cap, NU_cap), outs=(out64, uniq64, uniq32, counts, overflow),
                          host_counters=host_counters)
    return state


def _finish_ahead(state: dict, out: dict) -> dict:
    """A finish that did not take the outputs of the ahead arm: blast counts
    of what the host-sized path assembled, and the next prediction."""
    ahead = state.get("ahead")
    if ahead is None:
        return out
    b = ahead["blast"]
    counts, overflow, n_overflow = blast_counts_indexed(
        out["uniq_pkgs32"], b["rev"], b["index"], b["et_contains"],
        b["node_is_db_cred"], b["node_is_db_tool"], b["ws"])
    out.update(blast_counts=counts, blast_overflow=overflow, blast_n_overflow=n_overflow)
    state["ws"]["fa_ahead_hit"] = False
    state["ws"]["fa_ahead_cap"] = (findings_ahead_capacity(out["pkg_idx"].numel()),
                                   findings_ahead_capacity(out["uniq_pkgs"].numel()))
    return out


def assemble_findings_finish(state: dict, pkg_base: int) -> dict:
    """The rest of :func:`assemble_findings`, on the CURRENT stream, which
    must be ordered behind the stream the begin part ran on (the same stream,
    or one that has waited for it): read the totals, relaunch the match on
    overflow, size the outputs and emit them.  For a state of
    :func:`assemble_findings_begin_ahead` whose sizes fit the prediction the
    outputs exist already and nothing is launched."""
    import torch

    lib = load()
    pending, layout, ws, cap = state["pending"], state["layout"], state["ws"], state["cap"]
    pairs, count = pending["out_pairs"], pending["out_count"]
    dev = pairs.device
    if state["bufs"] is None:
        e64 = [torch.empty(0, dtype=torch.int64, device=dev) for _ in range(5)]
        return _finish_ahead(state, dict(
            zip(("pkg_idx", "win_idx", "pkg_nodes", "pos", "uniq_pkgs"), e64),
            uniq_pkgs32=torch.empty(0, dtype=torch.int32, device=dev)))
    cur = torch.cuda.current_stream()
    if cur != state["stream"]:
        # buffers first allocated under the other stream are used here from
        # now on: tell the allocator, which frees a block to the pool of the
        # stream it was allocated on
        for t in state["fresh"]:
            t.record_stream(cur)
    ws["fa_counted"].synchronize()  # the one host sync of the assembly
    F, NU, n = ws["fa_host_totals"].tolist()
    if n < 0:
        raise RuntimeError("match: device match count overflowed int32; shard the package batch")
    ahead = state.get("ahead")
    if ahead is not None and ahead["caps"] is not None:
        F_cap, NU_cap = ahead["caps"]
        if F <= F_cap and NU <= NU_cap and n <= cap:
            # the condition the kernels evaluated: they emitted, counted and reset
            out64, uniq64, uniq32, counts, overflow = ahead["outs"]
            ws["fa_dirty"] = False
            ws["fa_ahead_hit"] = True
            ws["fa_ahead_cap"] = (findings_ahead_capacity(F), findings_ahead_capacity(NU))
            return {"pkg_idx": out64[0][:F], "win_idx": out64[1][:F],
                    "pkg_nodes": out64[2][:F], "pos": out64[3][:F],
                    "uniq_pkgs": uniq64[:NU], "uniq_pkgs32": uniq32[:NU],
                    "blast_counts": counts[:NU * 6].view(NU, 6),
                    "blast_overflow": overflow[:NU],
                    "blast_n_overflow": int(ahead["host_counters"][1])}
    if n > cap:
        relaunched = pending["relaunch"](int(n * 1.2) + 1024)
        return _finish_ahead(state, assemble_findings(relaunched, layout, pkg_base, ws))
    if F >= 1 << 31:
        raise RuntimeError(f"assemble_findings: {F} findings exceed int32; shard the package batch")
    U, P = state["U"], state["P"]
    bitmap, row_cnt, row_tail, chain_prev, rank_of, word_f, block_sums = state["bufs"]
    pkg_idx, win_idx, pkg_nodes, pos = (
        torch.empty(F, dtype=torch.int64, device=dev) for _ in range(4))
    uniq64 = torch.empty(NU, dtype=torch.int64, device=dev)
    uniq32 = torch.empty(NU, dtype=torch.int32, device=dev)
    rc = lib.abom_findings_emit(
        _ptr(pairs), _ptr(count), cap, _ptr(layout["row_of"]), U, P,
        _ptr(bitmap), _ptr(row_cnt), _ptr(row_tail), _ptr(chain_prev),
        _ptr(rank_of), _ptr(word_f), _ptr(block_sums),
        int(pkg_base), F, NU,
        _ptr(pkg_idx), _ptr(win_idx), _ptr(pkg_nodes), _ptr(pos),
        _ptr(uniq64), _ptr(uniq32), _stream(),
    )
    _check(rc, "abom_findings_emit")
    ws["fa_dirty"] = False
    return _finish_ahead(state, {
        "pkg_idx": pkg_idx, "win_idx": win_idx, "pkg_nodes": pkg_nodes, "pos": pos,
        "uniq_pkgs": uniq64, "uniq_pkgs32": uniq32})


def match(pkg_group_key, pkg_key_hi, pkg_key_lo, pkg_flags, group_keys, group_off,
          windows: dict, capacity: Optional[int] = None, pkg_win_range=None):
    """Bulk version-range match.  Returns sorted (pkg_idx u32, window_idx u32).

    All tensors device-resident; ``windows`` carries intro/fixed/last hi+lo
    (int64 bit-patterns) and flags (uint8).  Retries with a larger buffer if
    capacity overflows.
    """
    pending = match_launch(pkg_group_key, pkg_key_hi, pkg_key_lo, pkg_flags,
                           group_keys, group_off, windows, capacity=capacity,
                           pkg_win_range=pkg_win_range)
    return match_finalize(pending)


def _bfs_buffers(ws: dict, num_nodes: int, dev):
    """dist, frontier_a, frontier_b, heavy queue and counters of a BFS workspace."""
    import torch

    return (_buf(ws, "dist", num_nodes, torch.int32, dev),
            _buf(ws, "frontier_a", num_nodes, torch.int32, dev),
            _buf(ws, "frontier_b", num_nodes, torch.int32, dev),
            _buf(ws, "heavy", num_nodes, torch.int32, dev),
            _buf(ws, "counters", _CTR_SLOTS, torch.int32, dev, zero=True))


def bfs_begin(row_off, sources, num_nodes: int, workspace: dict) -> None:
    """Enqueue the first part of :func:`bfs` on the current stream without
    syncing: fill ``dist``, zero the counters, seed the sources.  Follow it
    with ``bfs(..., workspace=workspace, begun=True)`` on the same stream,
    graph and sources; work enqueued on other streams in between starts after
    the fill instead of beside it."""
    lib = load()
    dist, fa, _fb, _hq, ctr = _bfs_buffers(workspace, num_nodes, row_off.device)
    rc = lib.abom_bfs_begin(_ptr(row_off), _ptr(sources), sources.numel(), _ptr(dist),
                            num_nodes, _ptr(fa), _ptr(ctr), _stream())
    _check(rc, "abom_bfs_begin")


def bfs_parent_index(rev: dict, allowed_mask: int, num_nodes: int) -> dict:
    """The parent index of the bottom-up pass for the reverse CSR ``rev`` and
    ``allowed_mask``: ``first_parent`` int32 ``[num_nodes]`` (read as u32:
    0xFFFFFFFF = no allowed in-edge, else the source of the first allowed
    in-edge of the reverse row in bits 0-30 and bit 31 set when the row holds
    another allowed in-edge), returned with the mask it was built for as
    ``{"first_parent", "allowed_mask"}``.  Graph structure only: it holds for
    as long as ``rev`` does, for every BFS with that mask.  Pass it to
    :func:`bfs` or :func:`bfs_level_bottom_up` as ``parent_index``.
    """
    import torch

    if num_nodes >= 2**31 - 1:
        raise ValueError("bfs_parent_index: a vertex id must fit 31 bits "
                         f"(num_nodes = {num_nodes})")
    lib = load()
    first_parent = torch.empty(num_nodes, dtype=torch.int32, device=rev["row_off"].device)
    et = _ptr(rev["etype"]) if rev.get("etype") is not None else None
    rc = lib.abom_bfs_parent_index(_ptr(rev["row_off"]), _ptr(rev["col"]), et, allowed_mask,
                                   num_nodes, _ptr(first_parent), _stream())
    _check(rc, "abom_bfs_parent_index")
    return {"first_parent": first_parent, "allowed_mask": allowed_mask}


def _parent_index_ptr(parent_index: Optional[dict], allowed_mask: int, num_nodes: int, what: str):
    """Pointer to the index's words after checking that it was built for this
    mask and this many nodes; None without an index or with the A/B toggle
    AGENT_BOM_BFS_PARENT_INDEX=0 (bottom-up passes then walk the reverse rows)."""
    if parent_index is None:
        return None
    if parent_index["allowed_mask"] != allowed_mask:
        raise ValueError(f"{what}: parent index built for mask "
                         f"{parent_index['allowed_mask']:#x}, called with {allowed_mask:#x}")
    if parent_index["first_parent"].numel() != num_nodes:
        raise ValueError(f"{what}: parent index of {parent_index['first_parent'].numel()} "
                         f"nodes, called with {num_nodes}")
    if os.environ.get("AGENT_BOM_BFS_PARENT_INDEX", "1") == "0":
        return None
    return _ptr(parent_index["first_parent"])


def bfs(row_off, col, sources, num_nodes: int, etype=None, allowed_mask: int = 0xFFFFFFFF,
        max_levels: int = 64, workspace: Optional[dict] = None, edge_src=None,
        rev=None, begun: bool = False, sources_degree: Optional[int] = None,
        parent_index: Optional[dict] = None):
    """Multi-source BFS over CSR; returns u32 dist (UNVISITED = 0xFFFFFFFF).

    ``workspace`` may carry preallocated buffers (dist/frontier_a/frontier_b/
    heavy/counters) to avoid reallocation in steady-state serving; it is left
    holding the number of levels run in ``workspace["levels"]``.
    ``begun``: :func:`bfs_begin` has been called on this workspace for this
    call.  ``sources_degree``: the sum of the out-degrees of the entries of
    ``sources`` (duplicates counted), when the caller knows it; the read of
    that sum from the device and its sync are then skipped.
    ``parent_index``: what :func:`bfs_parent_index` returned for ``rev`` and
    ``allowed_mask``; the bottom-up levels then read one index word per
    vertex and walk a reverse row only when its first parent is outside the
    frontier.  An index built for another mask or node count raises
    ``ValueError``; without ``rev`` there is no bottom-up level to use it;
    AGENT_BOM_BFS_PARENT_INDEX=0 runs the levels without it (A/B toggle).
    """
    import torch

    lib = load()
    dev = row_off.device
    ws = workspace if workspace is not None else {}
    if begun and (workspace is None or "dist" not in workspace):
        raise ValueError("bfs: begun=True needs the workspace bfs_begin was called on")
    first_parent_p = _parent_index_ptr(parent_index, allowed_mask, num_nodes, "bfs")
    dist, fa, fb, hq, ctr = _bfs_buffers(ws, num_nodes, dev)
    host_ctr = ws.get("host_counters")
    if host_ctr is None:
        # pinned, so the per-level count read is a direct copy
        host_ctr = ws["host_counters"] = torch.zeros(
            _CTR_SLOTS, dtype=torch.int32, pin_memory=True)

    et = _ptr(etype) if etype is not None else None
    if os.environ.get("AGENT_BOM_BFS_DENSE", "1") == "0":
        edge_src = None  # A/B toggle: disable edge-centric dense-frontier mode
    es = _ptr(edge_src) if edge_src is not None else None
    num_edges = col.numel()
    # direction-optimized dense levels: pass the reverse CSR for bottom-up
    rev_off_p = rev_col_p = rev_et_p = None
    if rev is not None and os.environ.get("AGENT_BOM_BFS_BOTTOMUP", "1") != "0":
        rev_off_p = _ptr(rev["row_off"])
        rev_col_p = _ptr(rev["col"])
        rev_et_p = _ptr(rev["etype"]) if rev.get("etype") is not None else None
    rc = lib.abom_bfs_run_indexed(
        _ptr(row_off), _ptr(col), et, allowed_mask,
        _ptr(sources), sources.numel(), _ptr(dist), num_nodes,
        _ptr(fa), _ptr(fb), _ptr(hq), _ptr(ctr), max_levels,
        es, num_edges, rev_off_p, rev_col_p, rev_et_p, first_parent_p,
        1 if begun else 0, -1 if sources_degree is None else int(sources_degree),
        _ptr(host_ctr), _stream(),
    )
    if rc < 0:
        _check(-rc, "abom_bfs_run_indexed")
    ws["levels"] = rc
    return dist[:num_nodes]


def bfs_level_bottom_up(rev: dict, dist, cur_level: int, num_nodes: int,
                        allowed_mask: int = 0xFFFFFFFF, parent_index: Optional[dict] = None,
                        workspace: Optional[dict] = None):
    """ONE bottom-up pass over the first ``num_nodes`` words of ``dist`` (in
    place): every unvisited vertex with an allowed in-edge from a vertex at
    ``cur_level`` gets ``cur_level + 1``.  Returns ``(claimed, open)``: the
    vertices claimed, and the vertices left unvisited that have an allowed
    in-edge.  With ``parent_index`` (:func:`bfs_parent_index`) the pass is the
    indexed kernel, else the walk over the reverse rows; ``dist`` may be
    longer than the graph and need not start on a 16-byte boundary.
    """
    import torch

    lib = load()
    if dist.numel() < num_nodes:
        raise ValueError("bfs_level_bottom_up: dist is shorter than the graph")
    first_parent_p = _parent_index_ptr(parent_index, allowed_mask, num_nodes,
                                       "bfs_level_bottom_up")
    ws = workspace if workspace is not None else {}
    ctr = _buf(ws, "counters", _CTR_SLOTS, torch.int32, dist.device, zero=True)
    ctr.zero_()
    et = _ptr(rev["etype"]) if rev.get("etype") is not None else None
    next_ptr, open_ptr = (ctypes.c_void_p(ctr.data_ptr() + off) for off in (_CTR_NEXT, _CTR_OPEN))
    if first_parent_p is not None:
        rc = lib.abom_bfs_bottom_up_indexed(
            _ptr(rev["row_off"]), _ptr(rev["col"]), et, allowed_mask, num_nodes, _ptr(dist),
            cur_level, first_parent_p, next_ptr, open_ptr, _stream())
        _check(rc, "abom_bfs_bottom_up_indexed")
    else:
        rc = lib.abom_bfs_bottom_up(
            _ptr(rev["row_off"]), _ptr(rev["col"]), et, allowed_mask, num_nodes, _ptr(dist),
            cur_level, next_ptr, open_ptr, _stream())
        _check(rc, "abom_bfs_bottom_up")
    counts = ctr.cpu()
    return int(counts[_CTR_NEXT // 4]), int(counts[_CTR_OPEN // 4])


def bfs_level(row_off, col, frontier, dist, level: int, etype=None,
              allowed_mask: int = 0xFFFFFFFF, workspace: Optional[dict] = None):
    """Expand ONE BFS level; returns the next frontier (claimed vertices).

    ``dist`` may be larger than the local graph (distributed mode: the tail
    indexes remote nodes and a claim there marks "queued for send").  Used by
    parallel/dist_bfs.py between RCCL frontier exchanges.
    """
    import torch

    lib = load()
    dev = row_off.device
    ws = workspace if workspace is not None else {}
    cap = dist.numel()
    nxt = _buf(ws, "next", cap, torch.int32, dev)
    hq = _buf(ws, "heavy", max(frontier.numel(), 1024), torch.int32, dev)
    ctr = _buf(ws, "counters", 4, torch.int32, dev, zero=True)
    ctr.zero_()
    et = _ptr(etype) if etype is not None else None
    next_ptr, heavy_ptr, deg_ptr = (
        ctypes.c_void_p(ctr.data_ptr() + off) for off in (_CTR_NEXT, _CTR_HEAVY, _CTR_DEGREE))
    rc = lib.abom_bfs_expand(
        _ptr(row_off), _ptr(col), et, allowed_mask, _ptr(frontier), frontier.numel(),
        _ptr(dist), level, _ptr(nxt), next_ptr, _ptr(hq),
        heavy_ptr, deg_ptr, cap, _stream(),
    )
    _check(rc, "abom_bfs_expand")
    rc = lib.abom_bfs_expand_heavy(
        _ptr(row_off), _ptr(col), et, allowed_mask, _ptr(hq),
        heavy_ptr, _ptr(dist), level, _ptr(nxt), next_ptr,
        deg_ptr, cap, _stream(),
    )
    _check(rc, "abom_bfs_expand_heavy")
    n = int(ctr[0].item())
    return nxt[:n].clone()


def bfs_level_edges(row_off, col, edge_src, frontier_dist_level: int, dist,
                    etype=None, allowed_mask: int = 0xFFFFFFFF,
                    workspace: Optional[dict] = None):
    """Edge-centric ONE-level expansion (dense frontiers, distributed mode).

    Claims every unvisited neighbor of vertices whose dist equals
    ``frontier_dist_level`` and RETURNS the claimed list (local + remote ids
    alike) — the materialized frontier the RCCL exchange needs.  Used by
    parallel/dist_bfs.py when the frontier's degree sum is a large share of
    the shard's edges (same threshold as the single-GPU dense mode).
    """
    import torch

    lib = load()
    dev = row_off.device
    ws = workspace if workspace is not None else {}
    cap = dist.numel()
    nxt = _buf(ws, "next", cap, torch.int32, dev)
    ctr = _buf(ws, "counters", 4, torch.int32, dev, zero=True)
    ctr.zero_()
    et = _ptr(etype) if etype is not None else None
    rc = lib.abom_bfs_expand_edges(
        _ptr(edge_src), _ptr(col), et, allowed_mask, col.numel(),
        _ptr(row_off), _ptr(dist), frontier_dist_level, _ptr(nxt),
        ctypes.c_void_p(ctr.data_ptr() + _CTR_NEXT),
        ctypes.c_void_p(ctr.data_ptr() + _CTR_DEGREE), 1, cap, _stream(),
    )
    _check(rc, "abom_bfs_expand_edges")
    n = int(ctr[0].item())
    return nxt[:n].clone()


# Sources per 64-bit word and words per node of a reach pass (csrc/reach_sets.hip)
REACH_WORD_SOURCES = 64
REACH_MAX_WORDS = 4
REACH_UNREACHED = 255


def reach_hops_chunks(row_off, col, sources, targets, num_nodes: int, etype=None,
                      allowed_mask: int = 0xFFFFFFFF, max_depth: int = 16,
                      workspace: Optional[dict] = None, chunk_sources: Optional[int] = None):
    """Per-source reach in pieces: a generator of ``(first, hops)`` where
    ``hops`` is the u8 ``[T, n]`` device tensor of sources ``first .. first+n``
    (``n <= chunk_sources``; one piece of all S sources when it is None).  A
    caller that cannot hold ``T * S`` bytes consumes one piece at a time; see
    :func:`reach_hops` for the contract of a piece.

    A piece is walked in passes of up to 64 * W sources, W = the fewest 64-bit
    words per node that hold the pass, at most 4: the sources of a pass share
    one bit-parallel BFS.  ``workspace`` keeps the state buffers between calls
    and is left with ``levels`` (the deepest pass) and ``passes`` as ints.
    """
    import torch

    dev = row_off.device
    if dev.type != "cuda":
        raise ValueError("reach_hops: the graph must be on a cuda device")
    _require(sources, "sources", torch.int32, dev)
    _require(targets, "targets", torch.int32, dev)
    S, T = sources.numel(), targets.numel()
    ws = workspace if workspace is not None else {}
    ws["levels"], ws["passes"] = 0, 0
    if S == 0:
        yield 0, torch.empty((T, 0), dtype=torch.uint8, device=dev)
        return
    chunk = S if chunk_sources is None else int(chunk_sources)
    if chunk < 1:
        raise ValueError("reach_hops: chunk_sources must be positive")
    if T == 0:
        for first in range(0, S, chunk):
            yield first, torch.empty((0, min(chunk, S - first)), dtype=torch.uint8, device=dev)
        return
    lib = load()
    per_word = REACH_WORD_SOURCES
    max_words = min(REACH_MAX_WORDS, (min(chunk, S) + per_word - 1) // per_word)
    if num_nodes * max_words >= 1 << 32:
        raise ValueError(f"reach_hops: {num_nodes} nodes x {max_words} words exceeds the "
                         "u32 frontier entries; use fewer sources per chunk")
    cells = num_nodes * max_words
    seen = _buf(ws, "reach_seen", cells, torch.int64, dev)
    cur = _buf(ws, "reach_cur", cells, torch.int64, dev, zero=True)
    nxt = _buf(ws, "reach_nxt", cells, torch.int64, dev, zero=True)
    qa = _buf(ws, "reach_queue_a", cells, torch.int32, dev)
    qb = _buf(ws, "reach_queue_b", cells, torch.int32, dev)
    hq = _buf(ws, "reach_heavy", cells, torch.int32, dev)
    ctr = _buf(ws, "reach_counters", 2, torch.int32, dev, zero=True)
    host_ctr = ws.get("reach_host_counters")
    if host_ctr is None:
        # pinned, so the per-level count read is a direct copy
        host_ctr = ws["reach_host_counters"] = torch.zeros(2, dtype=torch.int32, pin_memory=True)
    if ws.get("reach_dirty"):
        # a pass that did not finish may have left bits behind
        cur.zero_()
        nxt.zero_()
    slot = _buf(ws, "reach_target_slot", num_nodes, torch.int32, dev)[:num_nodes]
    slot.fill_(-1)
    slot[targets.to(torch.int64)] = torch.arange(T, dtype=torch.int32, device=dev)
    sources = sources.contiguous()
    et = _ptr(etype) if etype is not None else None
    for first in range(0, S, chunk):
        n = min(chunk, S - first)
        hops = torch.full((T, n), REACH_UNREACHED, dtype=torch.uint8, device=dev)
        done = 0
        while done < n:
            words = min(REACH_MAX_WORDS, (n - done + per_word - 1) // per_word)
            count = min(n - done, words * per_word)
            ws["reach_dirty"] = True
            rc = lib.abom_reach_hops(
                _ptr(row_off), _ptr(col), et, allowed_mask,
                ctypes.c_void_p(sources.data_ptr() + 4 * (first + done)), count, words,
                num_nodes, _ptr(slot), _ptr(hops), n, done, max_depth,
                _ptr(seen), _ptr(cur), _ptr(nxt), _ptr(qa), _ptr(qb), _ptr(hq),
                _ptr(ctr), _ptr(host_ctr), _stream(),
            )
            if rc < 0:
                _check(-rc, "abom_reach_hops")
            ws["reach_dirty"] = False
            ws["levels"] = max(ws["levels"], rc)
            ws["passes"] += 1
            done += count
        yield first, hops


def reach_hops(row_off, col, sources, targets, num_nodes: int, etype=None,
               allowed_mask: int = 0xFFFFFFFF, max_depth: int = 16,
               workspace: Optional[dict] = None):
    """Per-source reach: u8 ``hops[t, s]`` = BFS distance from ``sources[s]``
    to ``targets[t]`` over the CSR (``row_off`` int64, ``col`` int32, edges
    filtered by ``etype``/``allowed_mask``) when it is at most ``max_depth``
    (clamped to [0, 254]), else 255.  ``sources`` and ``targets`` are int32
    node ids in [0, num_nodes) on the graph's device; duplicate sources each
    keep their column, targets are distinct.  ``max_depth`` is that of
    ``UnifiedGraph.bfs``: a node at that distance is recorded, not expanded.
    S == 0 or T == 0 returns an empty tensor without a launch.

    The whole ``[T, S]`` matrix is one tensor here; :func:`reach_hops_chunks`
    yields it in column pieces when it would be too large.  ``workspace``:
    see there (``levels`` and ``passes`` are left as ints).
    """
    for _first, hops in reach_hops_chunks(row_off, col, sources, targets, num_nodes,
                                          etype=etype, allowed_mask=allowed_mask,
                                          max_depth=max_depth, workspace=workspace):
        return hops


def impact_query(row_off, col, query_sources, etype=None, allowed_mask: int = 0xFFFFFFFF,
                 max_hops: int = 4, max_nodes: int = 4096, out=None):
    """Batched bounded blast-radius queries (one block per query).

    Returns (nodes u32 [Q, max_nodes], hops u8 [Q, max_nodes], counts u32 [Q],
    truncated u8 [Q]).  ``out`` may carry those four tensors preallocated; the
    call then allocates nothing and is exactly one kernel launch, which is
    what a hipGraph capture needs.  Hops are reported as uint8, so
    ``max_hops`` above 255 is refused.
    """
    import torch

    if max_hops > 255:
        raise ValueError(f"max_hops {max_hops} does not fit the uint8 hop output (max 255)")
    lib = load()
    dev = row_off.device
    Q = query_sources.numel()
    if out is None:
        out = (torch.empty((Q, max_nodes), dtype=torch.int32, device=dev),
               torch.empty((Q, max_nodes), dtype=torch.uint8, device=dev),
               torch.zeros(Q, dtype=torch.int32, device=dev),
               torch.zeros(Q, dtype=torch.uint8, device=dev))
    out_nodes, out_hops, out_counts, out_trunc = out
    et = _ptr(etype) if etype is not None else None
    rc = lib.abom_impact_query(
        _ptr(row_off), _ptr(col), et, allowed_mask, _ptr(query_sources), Q,
        max_hops, max_nodes, _ptr(out_nodes), _ptr(out_hops), _ptr(out_counts),
        _ptr(out_trunc), _stream(),
    )
    _check(rc, "abom_impact_query")
    return out_nodes, out_hops, out_counts, out_trunc


def blast_counts(pkgs, rev, fwd, et_codes: tuple[int, int, int, int],
                 node_is_db_cred, node_is_db_tool):
    """Fused per-package reach counts.  Returns (counts [n,6] int32,
    overflow u8 [n]) — overflowed rows must be recomputed by the caller's
    sort-based path."""
    import torch

    lib = load()
    n = pkgs.numel()
    dev = pkgs.device
    out_counts = torch.zeros(n * 6, dtype=torch.int32, device=dev)
    out_overflow = torch.zeros(n, dtype=torch.uint8, device=dev)
    rc = lib.abom_blast_counts(
        _ptr(pkgs), n,
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]),
        _ptr(fwd["row_off"]), _ptr(fwd["col"]), _ptr(fwd["etype"]),
        et_codes[0], et_codes[1], et_codes[2], et_codes[3],
        _ptr(node_is_db_cred), _ptr(node_is_db_tool),
        _ptr(out_counts), _ptr(out_overflow), _stream(),
    )
    _check(rc, "abom_blast_counts")
    return out_counts.view(n, 6), out_overflow


def blast_counts_indexed(pkgs, rev, index: dict, et_contains: int,
                         node_is_db_cred, node_is_db_tool, workspace: dict):
    """Per-package reach counts from the per-server reach index
    (``graph.gpu_engine.build_reach_index``): a thread-per-package pass that
    finishes packages with at most one containing server and queues the rest
    for a wave-per-package pass.  Returns (counts [n,6] int32, overflow u8
    [n], number of overflowed rows); the one host read is that number.  The
    two kernels write every row, so the outputs are not pre-filled.
    ``workspace["counters"]`` keeps {queued packages, overflowed rows} of the
    last call."""
    import torch

    lib = load()
    n = pkgs.numel()
    dev = pkgs.device
    out_counts = torch.empty(n * 6, dtype=torch.int32, device=dev)
    out_overflow = torch.empty(n, dtype=torch.uint8, device=dev)
    queue = _buf(workspace, "queue", n, torch.int32, dev)
    counters = _buf(workspace, "counters", 2, torch.int32, dev)
    rc = lib.abom_blast_counts_indexed(
        _ptr(pkgs), n,
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), et_contains,
        _ptr(index["reach_off"]), _ptr(index["reach_col"]), _ptr(index["reach_db"]),
        index["row_base"], index["reach_off"].shape[0],
        _ptr(node_is_db_cred), _ptr(node_is_db_tool),
        _ptr(queue), _ptr(counters), _ptr(out_counts), _ptr(out_overflow), _stream(),
    )
    _check(rc, "abom_blast_counts_indexed")
    n_overflow = int(counters[1].item())
    return out_counts.view(n, 6), out_overflow, n_overflow


def blast_counts_indexed_sized(pkgs, n_dev, rev, index: dict, et_contains: int,
                               node_is_db_cred, node_is_db_tool, workspace: dict):
    """:func:`blast_counts_indexed` for a package count that is on the device:
    ``pkgs`` (int32) is a buffer of some capacity, ``n_dev`` an int64 tensor
    whose first element says how many of its entries count.  Grids are sized
    from the capacity; {queued packages, overflowed rows} come back through
    pinned host memory.  Returns (counts [capacity * 6], overflow
    [capacity], queued, overflowed rows); rows from ``n_dev`` on are not
    written.  The step runs the same entry point inside
    ``abom_findings_ahead``."""
    import torch

    lib = load()
    n_cap = pkgs.numel()
    dev = pkgs.device
    out_counts = torch.empty(n_cap * 6, dtype=torch.int32, device=dev)
    out_overflow = torch.empty(n_cap, dtype=torch.uint8, device=dev)
    queue = _buf(workspace, "queue", n_cap, torch.int32, dev)
    counters = _buf(workspace, "counters", 2, torch.int32, dev)
    host = _blast_host_counters(workspace)
    rc = lib.abom_blast_counts_indexed_sized(
        _ptr(pkgs), _ptr(n_dev), n_cap,
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), et_contains,
        _ptr(index["reach_off"]), _ptr(index["reach_col"]), _ptr(index["reach_db"]),
        index["row_base"], index["reach_off"].shape[0],
        _ptr(node_is_db_cred), _ptr(node_is_db_tool),
        _ptr(queue), _ptr(counters), _ptr(host),
        _ptr(out_counts), _ptr(out_overflow), _stream(),
    )
    _check(rc, "abom_blast_counts_indexed_sized")
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    queued, n_overflow = host.tolist()
    return out_counts, out_overflow, queued, n_overflow


# ── Multi-hop delegation expansion (ops/csrc/blast_hops.hip) ───────────────

# LDS caps of blast_hops_wave_kernel (HOPS_*_CAP, csrc/blast_hops.hip): a
# package whose visited servers, visited agents or credential union pass one
# is resolved by the exact join.  ``abom_blast_hops_cap`` reports the values
# the library was built with.
BLAST_HOPS_SRV_CAP = 448
BLAST_HOPS_AG_CAP = 192
BLAST_HOPS_CR_CAP = 448
BLAST_HOPS_MAX_DEPTH = 5


def _hops_inputs(pkgs32, rev: dict, index: dict, agent_index: dict):
    """Argument checks shared by the blast_hops bindings; returns the device."""
    import torch

    dev = pkgs32.device
    if dev.type != "cuda":
        raise ValueError(f"blast_hops: pkgs32 on {dev}, expected a GPU tensor")
    _require(pkgs32, "pkgs32", torch.int32, dev)
    _require(rev["row_off"], "rev.row_off", torch.int64, dev)
    E = rev["col"].numel()
    _require(rev["col"], "rev.col", torch.int32, dev)
    _require(rev["etype"], "rev.etype", torch.uint8, dev, E)
    _require(index["reach_off"], "index.reach_off", torch.int32, dev)
    if index["reach_off"].dim() != 2 or index["reach_off"].shape[1] != 4:
        raise ValueError("blast_hops: index.reach_off is not [rows, 4]")
    _require(index["reach_col"], "index.reach_col", torch.int32, dev)
    _require(agent_index["agent_off"], "agent_index.agent_off", torch.int32, dev)
    if agent_index["agent_off"].numel() < 1:
        raise ValueError("blast_hops: agent_index.agent_off is empty")
    _require(agent_index["agent_srv"], "agent_index.agent_srv", torch.int32, dev)
    return dev


def _hops_expand(torch, beg, cnt, carry, col):
    """Segment gather: ``col[beg[i]:beg[i]+cnt[i]]`` for every i, each entry
    paired with ``carry[i]``."""
    dev = beg.device
    total = int(cnt.sum().item())
    if total == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e.clone()
    rep = torch.repeat_interleave(torch.arange(beg.numel(), device=dev), cnt)
    ends = torch.cumsum(cnt, 0)
    within = torch.arange(total, device=dev) - (ends - cnt)[rep]
    return col[beg[rep] + within].to(torch.int64), carry[rep]


def _blast_hops_join(pkgs, rev: dict, index: dict, agent_index: dict, et_contains: int,
                     depth: int):
    """The expansion of :func:`blast_hops` as sort-based set operations on
    (package position << 32 | node) keys: exact for any set size, the path of
    the rows that overflowed an LDS cap.  ``pkgs`` int64 [k]; returns
    (hop_agents int32 [k,4], t_creds int32 [k], hop_depth uint8 [k])."""
    import torch

    dev = pkgs.device
    k = pkgs.numel()
    reach_off = index["reach_off"].to(torch.int64)
    reach_col = index["reach_col"]
    row_base, S = int(index["row_base"]), reach_off.shape[0]
    agent_off = agent_index["agent_off"].to(torch.int64)
    agent_srv = agent_index["agent_srv"]
    A = agent_off.numel() - 1

    def split(keys):
        return keys >> 32, keys & 0xFFFFFFFF

    def server_segment(keys, first):
        # segment ``first`` (0 agents, 1 creds) of the servers' index rows;
        # a server without a row has no neighbours, as in the kernel
        pos, node = split(keys)
        row = node - row_base
        ok = (row >= 0) & (row < S)
        row = row.clamp(0, max(S - 1, 0))
        if S == 0:
            return keys[:0]
        beg = reach_off[row, first]
        cnt = torch.where(ok, reach_off[row, first + 1] - beg, torch.zeros_like(beg))
        nbr, carry = _hops_expand(torch, beg, cnt, pos, reach_col)
        return torch.unique((carry << 32) | nbr)

    def servers_of(keys):
        pos, node = split(keys)
        ok = node < A
        if A == 0:
            return keys[:0]
        a = node.clamp(0, A - 1)
        beg = agent_off[a]
        cnt = torch.where(ok, agent_off[a + 1] - beg, torch.zeros_like(beg))
        nbr, carry = _hops_expand(torch, beg, cnt, pos, agent_srv)
        return torch.unique((carry << 32) | nbr)

    def minus(keys, seen):
        return keys[~torch.isin(keys, seen)]

    def per_pos(keys):
        return torch.bincount(keys >> 32, minlength=k).to(torch.int32)

    pos = torch.arange(k, device=dev)
    row_off = rev["row_off"]
    beg = row_off[pkgs]
    e_col, e_pos = _hops_expand(torch, beg, row_off[pkgs + 1] - beg, pos,
                                torch.arange(rev["col"].numel(), device=dev))
    held = rev["etype"][e_col] == et_contains
    s0 = torch.unique((e_pos[held] << 32) | rev["col"][e_col[held]].to(torch.int64))
    a1 = server_segment(s0, 0)
    seen_s, seen_a = s0, a1
    frontier = minus(servers_of(a1), seen_s)
    seen_s = torch.cat([seen_s, frontier])
    hop_agents = torch.zeros(k, 4, dtype=torch.int32, device=dev)
    levels = []
    for h in range(1, depth):
        level = minus(server_segment(frontier, 0), seen_a)
        if level.numel() == 0:
            break
        seen_a = torch.cat([seen_a, level])
        levels.append(level)
        hop_agents[:, h - 1] = per_pos(level)
        if h + 1 < depth:
            frontier = minus(servers_of(level), seen_s)
            seen_s = torch.cat([seen_s, frontier])
    t_creds = torch.zeros(k, dtype=torch.int32, device=dev)
    if levels:
        t_creds = per_pos(server_segment(servers_of(torch.cat(levels)), 1))
    # a level is empty for a package once one before it was
    hop_depth = (1 + (hop_agents > 0).sum(dim=1)).to(torch.uint8)
    return hop_agents, t_creds, hop_depth


def blast_hops(pkgs32, rev: dict, index: dict, agent_index: dict, et_contains: int,
               max_depth: int, workspace: Optional[dict] = None) -> dict:
    """Multi-hop delegation blast radius of package nodes (csrc/blast_hops.hip;
    semantics: ``cpu_ref.blast_hops``).  ``index`` is the per-server reach
    index, ``agent_index`` the per-agent server index
    (``graph.gpu_engine.build_reach_index`` / ``build_agent_index``);
    ``max_depth`` is clamped to [1, 5].

    Returns device tensors ``hop_agents`` int32 [n,4] (agents first reached
    at hop 2..5), ``t_creds`` int32 [n] and ``hop_depth`` uint8 [n].  A
    thread-per-package pass finishes the packages whose direct agents use no
    server outside the holders; a wave-per-package pass walks the rest in LDS;
    rows that pass a cap (BLAST_HOPS_*_CAP) are recomputed by the exact join.
    The one host read is {queued, overflowed}, left as ints in
    ``workspace["hops_queued"]`` and ``workspace["hops_overflow"]``.  Depth 1
    and an empty package list launch nothing."""
    import torch

    dev = _hops_inputs(pkgs32, rev, index, agent_index)
    ws = workspace if workspace is not None else {}
    depth = max(1, min(int(max_depth), BLAST_HOPS_MAX_DEPTH))
    n = pkgs32.numel()
    ws["hops_queued"] = ws["hops_overflow"] = 0
    if n == 0 or depth == 1:
        return {"hop_agents": torch.zeros(n, 4, dtype=torch.int32, device=dev),
                "t_creds": torch.zeros(n, dtype=torch.int32, device=dev),
                "hop_depth": torch.ones(n, dtype=torch.uint8, device=dev)}
    lib = load()
    hop_agents = torch.empty(n, 4, dtype=torch.int32, device=dev)
    t_creds = torch.empty(n, dtype=torch.int32, device=dev)
    hop_depth = torch.empty(n, dtype=torch.uint8, device=dev)
    overflow = torch.empty(n, dtype=torch.uint8, device=dev)
    queue = _buf(ws, "hops_queue", n, torch.int32, dev)
    counters = _buf(ws, "hops_counters", 2, torch.int32, dev)
    rc = lib.abom_blast_hops(
        _ptr(pkgs32), n,
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), int(et_contains),
        _ptr(index["reach_off"]), _ptr(index["reach_col"]),
        int(index["row_base"]), index["reach_off"].shape[0],
        _ptr(agent_index["agent_off"]), _ptr(agent_index["agent_srv"]),
        agent_index["agent_off"].numel() - 1, depth,
        _ptr(queue), _ptr(counters),
        _ptr(hop_agents), _ptr(t_creds), _ptr(hop_depth), _ptr(overflow), _stream(),
    )
    _check(rc, "abom_blast_hops")
    ws["hops_queued"], ws["hops_overflow"] = counters.tolist()
    if ws["hops_overflow"]:
        ov = torch.nonzero(overflow).flatten()
        heavy = _blast_hops_join(pkgs32[ov].to(torch.int64), rev, index, agent_index,
                                 int(et_contains), depth)
        hop_agents[ov], t_creds[ov], hop_depth[ov] = heavy
    return {"hop_agents": hop_agents, "t_creds": t_creds, "hop_depth": hop_depth}


def blast_hops_sized(pkgs32, n_dev, rev: dict, index: dict, agent_index: dict,
                     et_contains: int, max_depth: int, workspace: dict):
    """The two passes of :func:`blast_hops` for a package count that is on the
    device: ``pkgs32`` is a buffer of some capacity, ``n_dev`` an int64 tensor
    whose first element says how many of its entries count, so the call can
    be enqueued behind the kernel that writes them with no host read.  Rows
    from ``n_dev`` on are not written, and overflowed rows are left flagged:
    returns (hop_agents [capacity,4], t_creds, hop_depth, overflow u8
    [capacity], queued, overflowed rows), the last two through pinned host
    memory after a wait for the stream."""
    import torch

    dev = _hops_inputs(pkgs32, rev, index, agent_index)
    _require(n_dev, "n_dev", torch.int64, dev)
    lib = load()
    n_cap = pkgs32.numel()
    hop_agents = torch.empty(n_cap, 4, dtype=torch.int32, device=dev)
    t_creds = torch.empty(n_cap, dtype=torch.int32, device=dev)
    hop_depth = torch.empty(n_cap, dtype=torch.uint8, device=dev)
    overflow = torch.empty(n_cap, dtype=torch.uint8, device=dev)
    queue = _buf(workspace, "hops_queue", n_cap, torch.int32, dev)
    counters = _buf(workspace, "hops_counters", 2, torch.int32, dev)
    host = workspace.get("hops_host_counters")
    if host is None:
        host = workspace["hops_host_counters"] = torch.zeros(
            2, dtype=torch.int32, pin_memory=True)
    rc = lib.abom_blast_hops_sized(
        _ptr(pkgs32), _ptr(n_dev), n_cap,
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), int(et_contains),
        _ptr(index["reach_off"]), _ptr(index["reach_col"]),
        int(index["row_base"]), index["reach_off"].shape[0],
        _ptr(agent_index["agent_off"]), _ptr(agent_index["agent_srv"]),
        agent_index["agent_off"].numel() - 1, int(max_depth),
        _ptr(queue), _ptr(counters), _ptr(host),
        _ptr(hop_agents), _ptr(t_creds), _ptr(hop_depth), _ptr(overflow), _stream(),
    )
    _check(rc, "abom_blast_hops_sized")
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    queued, n_overflow = host.tolist()
    return hop_agents, t_creds, hop_depth, overflow, queued, n_overflow


# ── Remediation plan (ops/csrc/remediation.hip) ─────────────────────────────

# LDS caps of the remediation tier-1 kernel and the install count above which an
# item goes straight to the bitmap tier (REMED_*, csrc/remediation.hip);
# ``abom_remediation_cap`` reports the values the library was built with.
REMEDIATION_SRV_CAP = 256
REMEDIATION_AG_CAP = 256
REMEDIATION_CR_CAP = 256
REMEDIATION_TL_CAP = 512
REMEDIATION_T1_INSTALLS = 1024
# workspace tensors that are all-zero between calls
REMEDIATION_ZERO_KEYS = ("remed_state", "remed_counters", "remed_pool")
# the bitmap pool of the union tiers, whoever uses them
_UNION_POOL_BYTES = 256 << 20
_UNION_POOL_SLICES = 256
_WF_HAS_FIXED = 2


def remediation_native_enabled() -> bool:
    """A/B toggle: AGENT_BOM_REMEDIATION_NATIVE=0 makes
    ``EstateEngine.remediation_plan`` compute the per-item arrays with the
    exact torch join (:func:`remediation_items_join`) instead of the kernels
    of csrc/remediation.hip."""
    return os.environ.get("AGENT_BOM_REMEDIATION_NATIVE", "1") != "0"


def _reach_node_span(index: dict) -> int:
    """1 + the largest node id the reach index names, as a row or an entry;
    read from the device once and kept on the index."""
    span = index.get("node_span")
    if span is None:
        span = int(index["row_base"]) + index["reach_off"].shape[0]
        if index["reach_col"].numel():
            span = max(span, int(index["reach_col"].max().item()) + 1)
        index["node_span"] = span
    return span


def _require_union_graph(rev: dict, index: dict, dev) -> None:
    """The reverse CSR and the per-server reach index, as the union tiers of
    csrc/abom_union.h read them."""
    import torch

    _require(rev["row_off"], "rev.row_off", torch.int64, dev)
    _require(rev["col"], "rev.col", torch.int32, dev)
    _require(rev["etype"], "rev.etype", torch.uint8, dev, rev["col"].numel())
    _require(index["reach_off"], "index.reach_off", torch.int32, dev)
    _require(index["reach_col"], "index.reach_col", torch.int32, dev)


def _union_workspace(who: str, ws: dict, prefix: str, index: dict, planes: int, n_groups: int,
                     n_counters: int, n_matched: int, pool_slices: Optional[int], dev):
    """The workspace of a per-group analysis that ends in the union tiers:
    ``<prefix>_state`` (8 words per group), ``<prefix>_counters`` and
    ``<prefix>_pool`` (``pool_slices`` slices of one bit per reach-index row
    and ``planes`` planes of one bit per node id), all zeroed on creation;
    ``<prefix>_matched`` and the pinned ``<prefix>_host_counters``.  Returns
    (rows, span, pool_slices, state, counters, pool, matched, host)."""
    import torch

    rows = index["reach_off"].shape[0]
    span = _reach_node_span(index)
    slice_words = (rows + 31) // 32 + planes * ((span + 31) // 32)
    if pool_slices is None:
        pool_slices = max(1, min(_UNION_POOL_SLICES, _UNION_POOL_BYTES // (4 * slice_words)))
    if pool_slices < 1:
        raise ValueError(f"{who}: pool_slices < 1")
    state = _buf(ws, f"{prefix}_state", 8 * n_groups, torch.int32, dev, zero=True)
    counters = _buf(ws, f"{prefix}_counters", n_counters, torch.int32, dev, zero=True)
    pool = _buf(ws, f"{prefix}_pool", pool_slices * slice_words, torch.int32, dev, zero=True)
    matched = _buf(ws, f"{prefix}_matched", n_matched, torch.int32, dev)
    host = ws.get(f"{prefix}_host_counters")
    if host is None:
        host = ws[f"{prefix}_host_counters"] = torch.zeros(
            n_counters, dtype=torch.int32, pin_memory=True)
    return rows, span, pool_slices, state, counters, pool, matched, host


def _read_counters(done, host) -> list:
    """The pinned counters once the copy enqueued before this call has landed."""
    done.record()
    done.synchronize()
    return host.tolist()


def _remediation_empty(torch, dev) -> dict:
    from agentbom_amd.ops.cpu_ref import REMEDIATION_KEYS

    dtypes = dict.fromkeys(REMEDIATION_KEYS, torch.int32)
    dtypes.update(max_score=torch.float32, worst_sev=torch.uint8, kev=torch.uint8,
                  fix_hi=torch.int64, fix_lo=torch.int64)
    return {k: torch.empty(0, dtype=dtypes[k], device=dev) for k in REMEDIATION_KEYS}


def remediation_items(pkg_idx, win_idx, scores, item_of, n_items: int, arena: dict,
                      rev: dict, index: dict, et_contains: int, pkg_base: int,
                      workspace: Optional[dict] = None,
                      pool_slices: Optional[int] = None) -> dict:
    """The per-item arrays of the remediation plan (csrc/remediation.hip;
    semantics and keys: ``cpu_ref.remediation_plan``) for the findings
    ``pkg_idx`` (int64, ascending), ``win_idx`` (int64) and ``scores`` (fp32,
    >= 0).  ``item_of`` int32 [P] maps a package to one of ``n_items`` items,
    ``index`` is the per-server reach index, which must hold a row for every
    source of a CONTAINS edge.  Exact on the device: an item too large for
    the LDS sets of the wave kernel is counted in a slice of a bitmap pool of
    ``pool_slices`` slices (default: as many as fit 256 MiB, at most 256).

    Two host reads: {matched items, matched installs} after the fold, to size
    the outputs, and {tier-2 items, pool rounds} at the end, left as ints in
    ``workspace["remed_queued"]`` and ``workspace["remed_rounds"]``.  The
    workspace tensors named by ``REMEDIATION_ZERO_KEYS`` are all-zero before
    and after a call."""
    import torch

    dev = pkg_idx.device
    if dev.type != "cuda":
        raise ValueError(f"remediation_items: pkg_idx on {dev}, expected a GPU tensor")
    F = pkg_idx.numel()
    _require(pkg_idx, "pkg_idx", torch.int64, dev)
    _require(win_idx, "win_idx", torch.int64, dev, F)
    _require(scores, "scores", torch.float32, dev, F)
    _require(item_of, "item_of", torch.int32, dev)
    _require_union_graph(rev, index, dev)
    windows = arena["windows"]
    W = windows["flags"].numel()
    _require(windows["flags"], "windows.flags", torch.uint8, dev)
    _require(windows["fixed_hi"], "windows.fixed_hi", torch.int64, dev, W)
    _require(windows["fixed_lo"], "windows.fixed_lo", torch.int64, dev, W)
    _require(arena["severity"], "arena.severity", torch.uint8, dev, W)
    _require(arena["kev"], "arena.kev", torch.uint8, dev, W)
    ws = workspace if workspace is not None else {}
    ws["remed_queued"] = ws["remed_rounds"] = 0
    if F == 0:
        return _remediation_empty(torch, dev)
    if F >= 1 << 31:
        raise RuntimeError(f"remediation_items: {F} findings exceed int32")
    lib = load()
    rows, span, pool_slices, state, counters, pool, matched, host = _union_workspace(
        "remediation_items", ws, "remed", index, 3, n_items, 4, min(n_items, F), pool_slices, dev)
    rc = lib.abom_remediation_fold(
        _ptr(pkg_idx), _ptr(win_idx), _ptr(scores), F,
        _ptr(item_of), _ptr(arena["severity"]), _ptr(arena["kev"]),
        _ptr(state), _ptr(matched), _ptr(counters), _ptr(host), _stream())
    _check(rc, "abom_remediation_fold")
    done = torch.cuda.Event()
    M, _, _, NI = _read_counters(done, host)  # the host read that sizes the outputs
    items = torch.sort(matched[:M]).values
    i32 = {k: torch.empty(M, dtype=torch.int32, device=dev)
           for k in ("rep_pkg", "installs", "n_findings", "n_vulns", "max_score", "n_unfixed",
                     "n_servers", "n_agents", "n_creds", "n_tools")}
    u8 = {k: torch.empty(M, dtype=torch.uint8, device=dev) for k in ("worst_sev", "kev")}
    i64 = {k: torch.empty(M, dtype=torch.int64, device=dev) for k in ("fix_hi", "fix_lo")}
    rc = lib.abom_remediation_gather(
        _ptr(items), M, _ptr(pkg_idx), _ptr(win_idx), F,
        _ptr(windows["flags"]), _ptr(windows["fixed_hi"]), _ptr(windows["fixed_lo"]),
        _ptr(state),
        _ptr(i32["rep_pkg"]), _ptr(i32["installs"]), _ptr(i32["n_findings"]),
        _ptr(i32["n_vulns"]), _ptr(i32["max_score"]), _ptr(u8["worst_sev"]), _ptr(u8["kev"]),
        _ptr(i64["fix_hi"]), _ptr(i64["fix_lo"]), _ptr(i32["n_unfixed"]), _stream())
    _check(rc, "abom_remediation_gather")
    # item -> its matched installs as a CSR; order within an item is free
    items_off = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    torch.cumsum(i32["installs"], 0, out=items_off[1:])
    csr_pkgs = torch.empty(NI, dtype=torch.int32, device=dev)
    rc = lib.abom_remediation_scatter(
        _ptr(pkg_idx), F, _ptr(item_of), _ptr(state), _ptr(items_off), M, NI,
        _ptr(csr_pkgs), _stream())
    _check(rc, "abom_remediation_scatter")
    queue = _buf(ws, "remed_queue", M, torch.int32, dev)
    rc = lib.abom_remediation_union(
        _ptr(items), M, _ptr(items_off), _ptr(csr_pkgs), int(pkg_base),
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), int(et_contains),
        _ptr(index["reach_off"]), _ptr(index["reach_col"]), int(index["row_base"]), rows,
        span, _ptr(state), _ptr(queue), _ptr(pool), int(pool_slices),
        _ptr(counters), _ptr(host),
        _ptr(i32["n_servers"]), _ptr(i32["n_agents"]), _ptr(i32["n_creds"]),
        _ptr(i32["n_tools"]), _stream())
    _check(rc, "abom_remediation_union")
    _, ws["remed_queued"], ws["remed_rounds"], _ = _read_counters(done, host)
    out = {"item": items, **i32, **u8, **i64}
    out["max_score"] = out["max_score"].view(torch.float32)
    return out


def remediation_items_join(pkg_idx, win_idx, scores, item_of, arena: dict, rev: dict,
                           index: dict, et_contains: int, pkg_base: int) -> dict:
    """The outputs of :func:`remediation_items` as sort-based set operations
    in torch on the tensors' device: (item position << 32 | node) pairs, then
    ``unique``.  Exact for any set size; the comparison arm of
    AGENT_BOM_REMEDIATION_NATIVE=0."""
    import torch

    dev = pkg_idx.device
    F = pkg_idx.numel()
    if F == 0:
        return _remediation_empty(torch, dev)
    sign = -0x8000000000000000
    windows = arena["windows"]
    W = windows["flags"].numel()
    items, inv = torch.unique(item_of[pkg_idx].to(torch.int64), return_inverse=True)
    M = items.numel()

    def count(pos):
        return torch.bincount(pos, minlength=M).to(torch.int32)

    def reduce(src, how, init):
        return torch.full((M,), init, dtype=src.dtype, device=dev).scatter_reduce_(
            0, inv, src, how)

    head = torch.ones(F, dtype=torch.bool, device=dev)
    head[1:] = pkg_idx[1:] != pkg_idx[:-1]
    out = {"item": items.to(torch.int32),
           "rep_pkg": reduce(pkg_idx, "amin", 1 << 62).to(torch.int32),
           "installs": count(inv[head]), "n_findings": count(inv)}
    # distinct (item, window) pairs
    iw = torch.unique(inv * W + win_idx)
    m_iw, w_iw = iw // W, iw % W
    out["n_vulns"] = count(m_iw)
    # scores are >= 0, so 0 is neutral for the max
    out["max_score"] = reduce(scores, "amax", 0.0)
    out["worst_sev"] = reduce(arena["severity"][win_idx].to(torch.int64), "amax", 0).to(torch.uint8)
    out["kev"] = reduce((arena["kev"][win_idx] != 0).to(torch.int64), "amax", 0).to(torch.uint8)
    fixed = (windows["flags"][w_iw] & _WF_HAS_FIXED) != 0
    # largest fixed key as unsigned 128 bits: the sign flip turns the int64
    # order into the u64 order; the best hi first, then the best lo among them
    m_fx = m_iw[fixed]
    hi, lo = windows["fixed_hi"][w_iw[fixed]] ^ sign, windows["fixed_lo"][w_iw[fixed]] ^ sign
    best_hi = torch.full((M,), sign, dtype=torch.int64, device=dev).scatter_reduce_(
        0, m_fx, hi, "amax")
    top = hi == best_hi[m_fx]
    best_lo = torch.full((M,), sign, dtype=torch.int64, device=dev).scatter_reduce_(
        0, m_fx[top], lo[top], "amax")
    has = torch.bincount(m_fx, minlength=M) > 0
    zero = torch.zeros(M, dtype=torch.int64, device=dev)
    out["fix_hi"] = torch.where(has, best_hi ^ sign, zero)
    out["fix_lo"] = torch.where(has, best_lo ^ sign, zero)
    out["n_unfixed"] = count(m_iw[~fixed])
    # (item, server): the CONTAINS sources of the matched installs
    nodes = pkg_idx[head] + int(pkg_base)
    beg = rev["row_off"][nodes]
    e, carry = _hops_expand(torch, beg, rev["row_off"][nodes + 1] - beg, inv[head],
                            torch.arange(rev["col"].numel(), device=dev))
    held = rev["etype"][e] == et_contains
    ms = torch.unique((carry[held] << 32) | rev["col"][e[held]].to(torch.int64))
    out["n_servers"] = count(ms >> 32)
    reach_off = index["reach_off"].to(torch.int64)
    S = reach_off.shape[0]
    row = (ms & 0xFFFFFFFF) - int(index["row_base"])
    ok = (row >= 0) & (row < S)
    row = row.clamp(0, max(S - 1, 0))
    for seg, key in enumerate(("n_agents", "n_creds", "n_tools")):
        if S == 0:
            out[key] = torch.zeros(M, dtype=torch.int32, device=dev)
            continue
        sbeg = reach_off[row, seg]
        cnt = torch.where(ok, reach_off[row, seg + 1] - sbeg, torch.zeros_like(sbeg))
        nbr, pos = _hops_expand(torch, sbeg, cnt, ms >> 32, index["reach_col"])
        out[key] = count(torch.unique((pos << 32) | nbr) >> 32)
    return out


# LDS caps of the toxic tier-1 kernel and the package count above which an
# advisory goes straight to the bitmap tier (TOXIC_*, csrc/toxic.hip);
# ``abom_toxic_cap`` reports the values the library was built with.
TOXIC_SRV_CAP = 256
TOXIC_AG_CAP = 256
TOXIC_T1_PKGS = 1024
# workspace tensors that are all-zero between calls
TOXIC_ZERO_KEYS = ("toxic_state", "toxic_counters", "toxic_pool")
_TOXIC_COUNTERS = 16
_TOXIC_SHARED = 1 << 16  # server-table bit: the row has two or more agents


def toxic_server_table(index: dict, tool_caps, tool_is_db, tool_base: int):
    """The server table of csrc/toxic.hip: int32 [rows of ``index``], read as
    u32 = caps_all | caps_db << 8 | shared << 16 -- the OR of ``tool_caps``
    (uint8 [n_tools], indexed by node id - ``tool_base``) over the row's
    tools, the same over its tools with ``tool_is_db`` set, and whether the
    row has two or more agents.  Graph and caps only: it holds for as long as
    the reach index and the caps tensor do."""
    import torch

    dev = index["reach_off"].device
    if dev.type != "cuda":
        raise ValueError(f"toxic_server_table: reach index on {dev}, expected a GPU tensor")
    n_tools = tool_caps.numel()
    _require(tool_caps, "tool_caps", torch.uint8, dev)
    _require(tool_is_db, "tool_is_db", torch.uint8, dev, n_tools)
    _require(index["reach_off"], "index.reach_off", torch.int32, dev)
    _require(index["reach_col"], "index.reach_col", torch.int32, dev)
    rows = index["reach_off"].shape[0]
    table = torch.empty(rows, dtype=torch.int32, device=dev)
    rc = load().abom_toxic_server_table(
        _ptr(index["reach_off"]), _ptr(index["reach_col"]), rows,
        _ptr(tool_caps), _ptr(tool_is_db), int(tool_base), n_tools, _ptr(table), _stream())
    _check(rc, "abom_toxic_server_table")
    return table


def toxic_poison_servers(table, row_base: int):
    """``poison_servers`` of ``cpu_ref.toxic_combinations`` from the server
    table: ascending int32 node ids of the rows with two or more agents whose
    unfiltered caps hold TC_WRITE and TC_READ or TC_RETRIEVAL."""
    import torch

    from agentbom_amd.ops.cpu_ref import TC_READ, TC_RETRIEVAL, TC_WRITE

    hit = ((table & _TOXIC_SHARED) != 0) & ((table & TC_WRITE) != 0) \
        & ((table & (TC_READ | TC_RETRIEVAL)) != 0)
    return (torch.nonzero(hit).flatten() + int(row_base)).to(torch.int32)


def _toxic_empty(torch, dev) -> dict:
    from agentbom_amd.ops.cpu_ref import TOXIC_VULN_KEYS

    dtypes = dict.fromkeys(TOXIC_VULN_KEYS, torch.int32)
    dtypes.update(max_score=torch.float32, worst_sev=torch.uint8, kev=torch.uint8,
                  patterns=torch.uint8)
    return {k: torch.empty(0, dtype=dtypes[k], device=dev) for k in TOXIC_VULN_KEYS}


def toxic_combinations(pkg_idx, win_idx, scores, n_creds, arena: dict, tool_lut, table,
                       rev: dict, index: dict, et_contains: int, pkg_base: int,
                       vuln_of=None, n_vulns: Optional[int] = None,
                       workspace: Optional[dict] = None,
                       pool_slices: Optional[int] = None) -> dict:
    """Toxic combinations of the findings ``pkg_idx`` (int64, ascending),
    ``win_idx`` (int64), ``scores`` (fp32, >= 0) and ``n_creds`` (int32) by
    the kernels of csrc/toxic.hip; semantics: ``cpu_ref.toxic_combinations``.
    ``table`` is :func:`toxic_server_table` of ``index``, the per-server reach
    index, which must hold a row for every source of a CONTAINS edge;
    ``arena`` gives ``severity``, ``kev`` and ``impact`` per window;
    ``vuln_of`` int32 [W] maps a window to one of ``n_vulns`` advisories
    (default: the identity; ``n_vulns`` is read from the device when not given).

    Returns ``patterns`` uint8 [F] and ``combo_score`` fp32 [F]; ``vulns``,
    the arrays of ``cpu_ref.TOXIC_VULN_KEYS`` per matched advisory, ascending;
    and as host ints ``n_by_pattern`` (a list of six), ``n_multi_agent`` and
    ``n_flagged``, the findings with a pattern.  Exact on the device: an
    advisory too large for the LDS sets of the wave kernel is counted in a
    slice of a bitmap pool of ``pool_slices`` slices (default: as many as fit
    256 MiB, at most 256).

    Two host reads: {matched advisories, (package, advisory) heads} after the
    fold, to size the outputs, and the totals at the end, with {tier-2
    advisories, pool rounds} left as ints in ``workspace["toxic_queued"]`` and
    ``workspace["toxic_rounds"]``.  The workspace tensors named by
    ``TOXIC_ZERO_KEYS`` are all-zero before and after a call."""
    import torch

    dev = pkg_idx.device
    if dev.type != "cuda":
        raise ValueError(f"toxic_combinations: pkg_idx on {dev}, expected a GPU tensor")
    F = pkg_idx.numel()
    W = arena["severity"].numel()
    _require(pkg_idx, "pkg_idx", torch.int64, dev)
    _require(win_idx, "win_idx", torch.int64, dev, F)
    _require(scores, "scores", torch.float32, dev, F)
    _require(n_creds, "n_creds", torch.int32, dev, F)
    _require(arena["severity"], "arena.severity", torch.uint8, dev)
    _require(arena["kev"], "arena.kev", torch.uint8, dev, W)
    _require(arena["impact"], "arena.impact", torch.uint8, dev, W)
    _require(tool_lut, "tool_lut", torch.uint8, dev, 9)
    _require_union_graph(rev, index, dev)
    rows = index["reach_off"].shape[0]
    _require(table, "table", torch.int32, dev, rows)
    if vuln_of is None:
        V = W
    else:
        _require(vuln_of, "vuln_of", torch.int32, dev, W)
        V = int(n_vulns) if n_vulns is not None else (int(vuln_of.max().item()) + 1 if W else 0)
    ws = workspace if workspace is not None else {}
    ws["toxic_queued"] = ws["toxic_rounds"] = 0
    if F == 0:
        return {"patterns": torch.empty(0, dtype=torch.uint8, device=dev),
                "combo_score": torch.empty(0, dtype=torch.float32, device=dev),
                "vulns": _toxic_empty(torch, dev), "n_by_pattern": [0] * 6,
                "n_multi_agent": 0, "n_flagged": 0}
    if F >= 1 << 31 or V >= 1 << 31:
        raise RuntimeError(f"toxic_combinations: {F} findings / {V} advisories exceed int32")
    lib = load()
    rows, span, pool_slices, state, counters, pool, matched, host = _union_workspace(
        "toxic_combinations", ws, "toxic", index, 1, V, _TOXIC_COUNTERS, min(V, F), pool_slices,
        dev)
    vuln_p = _ptr(vuln_of) if vuln_of is not None else None
    patterns = torch.empty(F, dtype=torch.uint8, device=dev)
    combo = torch.empty(F, dtype=torch.float32, device=dev)
    rc = lib.abom_toxic_fold(
        _ptr(pkg_idx), _ptr(win_idx), _ptr(scores), _ptr(n_creds), F, vuln_p, W, V,
        _ptr(arena["severity"]), _ptr(arena["kev"]), _ptr(arena["impact"]), _ptr(tool_lut),
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), int(et_contains),
        int(pkg_base), _ptr(table), int(index["row_base"]), rows,
        _ptr(state), _ptr(matched), _ptr(counters), _ptr(host), _ptr(patterns), _stream())
    _check(rc, "abom_toxic_fold")
    done = torch.cuda.Event()
    M, _, _, NH = _read_counters(done, host)[:4]  # the host read that sizes the outputs
    vulns = torch.sort(matched[:M]).values
    i32 = {k: torch.empty(M, dtype=torch.int32, device=dev)
           for k in ("n_findings", "n_packages", "n_servers", "n_agents", "max_score")}
    u8 = {k: torch.empty(M, dtype=torch.uint8, device=dev)
          for k in ("worst_sev", "kev", "patterns")}
    rc = lib.abom_toxic_gather(
        _ptr(vulns), M, _ptr(state), _ptr(i32["n_findings"]), _ptr(i32["n_packages"]),
        _ptr(i32["max_score"]), _ptr(u8["worst_sev"]), _ptr(u8["kev"]), _ptr(u8["patterns"]),
        _stream())
    _check(rc, "abom_toxic_gather")
    # advisory -> its distinct matched packages as a CSR; order within one is free
    vulns_off = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    torch.cumsum(i32["n_packages"], 0, out=vulns_off[1:])
    csr_pkgs = torch.empty(NH, dtype=torch.int32, device=dev)
    rc = lib.abom_toxic_scatter(
        _ptr(pkg_idx), _ptr(win_idx), F, vuln_p, W, V, _ptr(state), _ptr(vulns_off), M, NH,
        _ptr(csr_pkgs), _stream())
    _check(rc, "abom_toxic_scatter")
    queue = _buf(ws, "toxic_queue", M, torch.int32, dev)
    rc = lib.abom_toxic_union(
        M, _ptr(vulns_off), _ptr(csr_pkgs), int(pkg_base),
        _ptr(rev["row_off"]), _ptr(rev["col"]), _ptr(rev["etype"]), int(et_contains),
        _ptr(index["reach_off"]), _ptr(index["reach_col"]), int(index["row_base"]), rows,
        span, _ptr(queue), _ptr(pool), int(pool_slices), _ptr(counters),
        _ptr(i32["n_servers"]), _ptr(i32["n_agents"]), _stream())
    _check(rc, "abom_toxic_union")
    rc = lib.abom_toxic_finish(
        _ptr(pkg_idx), _ptr(win_idx), _ptr(scores), F, vuln_p, W, V, _ptr(vulns), M,
        _ptr(state), _ptr(i32["n_agents"]), _ptr(i32["max_score"]), _ptr(u8["patterns"]),
        _ptr(patterns), _ptr(combo), _ptr(counters), _ptr(host), _stream())
    _check(rc, "abom_toxic_finish")
    totals = _read_counters(done, host)
    ws["toxic_queued"], ws["toxic_rounds"] = totals[1], totals[2]
    per = {"vuln": vulns, **i32, **u8}
    per["max_score"] = per["max_score"].view(torch.float32)
    return {"patterns": patterns, "combo_score": combo, "vulns": per,
            "n_by_pattern": totals[4:10], "n_multi_agent": totals[10], "n_flagged": totals[11]}


def risk_weights_array() -> np.ndarray:
    """The 22-float weight vector, in kernel order, from live config."""
    from agentbom_amd.utils import config as cfg

    return np.array(
        [
            cfg.RISK_BASE_CRITICAL, cfg.RISK_BASE_HIGH, cfg.RISK_BASE_MEDIUM, cfg.RISK_BASE_LOW,
            cfg.RISK_AGENT_WEIGHT, cfg.RISK_AGENT_CAP, cfg.RISK_CRED_WEIGHT, cfg.RISK_CRED_CAP,
            cfg.RISK_TOOL_WEIGHT, cfg.RISK_TOOL_CAP, cfg.RISK_AI_BOOST, cfg.RISK_KEV_BOOST,
            cfg.RISK_EPSS_BOOST, cfg.EPSS_CRITICAL_THRESHOLD,
            cfg.RISK_SCORECARD_TIER1_THRESHOLD, cfg.RISK_SCORECARD_TIER1_BOOST,
            cfg.RISK_SCORECARD_TIER2_THRESHOLD, cfg.RISK_SCORECARD_TIER2_BOOST,
            cfg.RISK_SCORECARD_TIER3_THRESHOLD, cfg.RISK_SCORECARD_TIER3_BOOST,
            cfg.RISK_REACHABLE_BOOST, cfg.RISK_UNREACHABLE_PENALTY,
        ],
        dtype=np.float32,
    )


def risk_score(severity, n_agents, n_creds, n_tools, flags, epss, scorecard, reach):
    """GPU risk scoring — same formula as models/blast.risk_score_from_counts."""
    import torch

    lib = load()
    n = severity.numel()
    out = torch.empty(n, dtype=torch.float32, device=severity.device)
    w = risk_weights_array()
    rc = lib.abom_risk_score(
        _ptr(severity), _ptr(n_agents), _ptr(n_creds), _ptr(n_tools), _ptr(flags),
        _ptr(epss), _ptr(scorecard), _ptr(reach), _ptr(out), n,
        w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _stream(),
    )
    _check(rc, "abom_risk_score")
    return out


def score_gather(win_idx, pkg_nodes, pos, arena_sev, arena_kev, arena_epss,
                 arena_impact, cred_lut, tool_lut, counts2d, dist):
    """Fused per-finding gather + risk score (one kernel for the whole
    post-counts chain).  Returns (scores f32, n_agents i32, n_creds i32,
    n_tools i32)."""
    import torch

    lib = load()
    n = win_idx.numel()
    dev = win_idx.device
    out_scores = torch.empty(n, dtype=torch.float32, device=dev)
    out_agents = torch.empty(n, dtype=torch.int32, device=dev)
    out_creds = torch.empty(n, dtype=torch.int32, device=dev)
    out_tools = torch.empty(n, dtype=torch.int32, device=dev)
    w = risk_weights_array()
    rc = lib.abom_score_gather(
        _ptr(win_idx), _ptr(pkg_nodes), _ptr(pos), _ptr(arena_sev),
        _ptr(arena_kev), _ptr(arena_epss), _ptr(arena_impact), _ptr(cred_lut),
        _ptr(tool_lut), _ptr(counts2d), _ptr(dist), _ptr(out_scores),
        _ptr(out_agents), _ptr(out_creds), _ptr(out_tools), n,
        w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _stream(),
    )
    _check(rc, "abom_score_gather")
    return out_scores, out_agents, out_creds, out_tools


def severity_histogram(owner, severity, num_containers: int):
    import torch

    lib = load()
    hist = torch.zeros(num_containers * 6, dtype=torch.int32, device=owner.device)
    rc = lib.abom_severity_histogram(_ptr(owner), _ptr(severity), _ptr(hist),
                                     owner.numel(), _stream())
    _check(rc, "abom_severity_histogram")
    return hist.view(num_containers, 6)


def path_relax(edge_src, col, etype, edge_weight, cur, nxt, node_boost,
               etype_boost, etype_trav, etype_gate, node_gate):
    """One hop of the max-score path DP (ops/csrc/paths.hip).

    ``cur``/``nxt``: int64 [N*2] tensors holding the packed u64 labels
    ((ordered_f32(score) << 32) | winner_edge); ``nxt`` must be pre-zeroed.
    ``edge_weight`` and ``node_gate`` may be None.
    """
    lib = load()
    rc = lib.abom_path_relax(
        _ptr(edge_src), _ptr(col), _ptr(etype),
        _ptr(edge_weight) if edge_weight is not None else None,
        _ptr(cur), _ptr(nxt), _ptr(node_boost), _ptr(etype_boost),
        _ptr(etype_trav), _ptr(etype_gate),
        _ptr(node_gate) if node_gate is not None else None,
        etype.numel(), _stream(),
    )
    _check(rc, "abom_path_relax")


_RANK_BINS = 1024
_RANK_CHUNK = 256


def rank_bucket_order(scores, workspace: Optional[dict] = None):
    """Deterministic finding rank via the stable counting-sort kernel.

    Bit-equal to gpu_engine.rank_order's quantized key sort (bucket asc,
    index asc) — four small launches, no rocprim (ops/csrc/rank.hip)."""
    import torch

    lib = load()
    n = scores.numel()
    dev = scores.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    nblocks = (n + _RANK_CHUNK - 1) // _RANK_CHUNK
    ws = workspace if workspace is not None else {}
    hist = _buf(ws, "rank_hist", nblocks * _RANK_BINS, torch.int32, dev)
    scratch = _buf(ws, "rank_scratch", 2 * _RANK_BINS, torch.int32, dev)
    order = torch.empty(n, dtype=torch.int64, device=dev)
    rc = lib.abom_rank_order(_ptr(scores), n, _ptr(hist), _ptr(scratch),
                             nblocks, _ptr(order), _stream())
    _check(rc, "abom_rank_order")
    return order


# ── Centrality (ops/csrc/centrality.hip) ───────────────────────────────────


def _heavy_rows(row_off):
    """Ids of the rows with >= CENTRALITY_HEAVY_DEGREE edges (int32, ascending):
    the rows the centrality kernels hand to one wave each."""
    import torch

    deg = row_off[1:] - row_off[:-1]
    return torch.nonzero(deg >= CENTRALITY_HEAVY_DEGREE).flatten().to(torch.int32)


def pagerank(rev_off, rev_col, out_degree, num_nodes: int, damping: float = 0.85,
             iterations: int = 50, workspace: Optional[dict] = None):
    """PageRank by pull power iteration over the reverse CSR; fp64 [N].

    ``rev_off`` int64 [N+1], ``rev_col`` int32 [E] (in-neighbours per node),
    ``out_degree`` int32 [N].  Dangling mass is spread uniformly.  Stops after
    ``iterations`` passes or after the first pass whose L1 change is below
    PAGERANK_TOLERANCE.  Bit-reproducible: no floating-point atomics.
    """
    import torch

    lib = load()
    dev = rev_off.device
    if num_nodes == 0:
        return torch.empty(0, dtype=torch.float64, device=dev)
    ws = workspace if workspace is not None else {}
    rank_a = _buf(ws, "pr_rank_a", num_nodes, torch.float64, dev)
    rank_b = _buf(ws, "pr_rank_b", num_nodes, torch.float64, dev)
    contrib_a = _buf(ws, "pr_contrib_a", num_nodes, torch.float64, dev)
    contrib_b = _buf(ws, "pr_contrib_b", num_nodes, torch.float64, dev)
    partials = _buf(ws, "pr_partials", 2 * _PAGERANK_PARTIALS, torch.float64, dev)
    scalars = _buf(ws, "pr_scalars", 2, torch.float64, dev)
    heavy = _heavy_rows(rev_off)
    rc = lib.abom_pagerank_run(
        _ptr(rev_off), _ptr(rev_col), _ptr(heavy), heavy.numel(),
        _ptr(out_degree), num_nodes, float(damping), PAGERANK_TOLERANCE,
        int(iterations), _ptr(rank_a), _ptr(rank_b), _ptr(contrib_a), _ptr(contrib_b),
        _ptr(partials), _ptr(scalars), _stream(),
    )
    if rc < 0:
        _check(-rc, "abom_pagerank_run")
    ws["pr_iterations"] = rc  # passes actually run (early stop below the tolerance)
    # the loop ping-pongs: an even number of passes ends in rank_a
    return (rank_a if rc % 2 == 0 else rank_b)[:num_nodes].clone()


def brandes_batch_size(num_sources: int, num_nodes: int) -> int:
    """Default Brandes batch: as many sources as fit the workspace budget
    ($AGENT_BOM_CENTRALITY_WS_MB), at most 64, at least 1."""
    from agentbom_amd.utils import config as cfg

    budget = cfg.CENTRALITY_WS_MB << 20
    fit = budget // (_BRANDES_CELL_BYTES * max(num_nodes, 1))
    return max(1, min(num_sources, _BRANDES_MAX_BATCH, fit))


def betweenness(fwd: dict, rev: dict, num_nodes: int, sources, batch: Optional[int] = None,
                workspace: Optional[dict] = None, allowed_mask: Optional[int] = None):
    """Un-normalised Brandes betweenness (unweighted) from ``sources``; fp64 [N].

    ``fwd`` / ``rev`` are CSR dicts (``row_off`` int64 [N+1], ``col`` int32
    [E], optional ``etype`` uint8 [E]).  Sources run ``batch`` at a time with
    [batch, N] dist/sigma/delta workspaces; the result does not depend on the
    batch size, bit for bit.  ``workspace["bc_deepest"]`` is left holding the
    deepest BFS level any source reached.  ``allowed_mask`` filters edges by type bit (needs
    ``etype`` in both dicts); None walks every edge.
    """
    import torch

    lib = load()
    dev = fwd["row_off"].device
    bc = torch.zeros(num_nodes, dtype=torch.float64, device=dev)
    src = np.asarray(sources.cpu() if hasattr(sources, "cpu") else sources, dtype=np.int64)
    if num_nodes == 0 or src.size == 0:
        return bc
    if src.min() < 0 or src.max() >= num_nodes:
        raise ValueError("betweenness: source id outside [0, num_nodes)")
    if batch is None:
        batch = brandes_batch_size(int(src.size), num_nodes)
    batch = max(1, min(int(batch), int(src.size), 65535))
    fwd_et = rev_et = None
    mask = 0xFFFFFFFF
    if allowed_mask is not None:
        fwd_et, rev_et, mask = _ptr(fwd["etype"]), _ptr(rev["etype"]), int(allowed_mask)
    ws = workspace if workspace is not None else {}
    cells = batch * num_nodes
    dist = _buf(ws, "bc_dist", cells, torch.int32, dev)
    sigma = _buf(ws, "bc_sigma", cells, torch.float64, dev)
    delta = _buf(ws, "bc_delta", cells, torch.float64, dev)
    counter = _buf(ws, "bc_counter", 1, torch.int32, dev, zero=True)
    fwd_heavy = _heavy_rows(fwd["row_off"])
    rev_heavy = _heavy_rows(rev["row_off"])
    src_dev = torch.from_numpy(src.astype(np.int32)).to(dev)
    for lo in range(0, int(src.size), batch):
        chunk = src_dev[lo:lo + batch]
        rc = lib.abom_brandes_run(
            _ptr(fwd["row_off"]), _ptr(fwd["col"]), fwd_et,
            _ptr(rev["row_off"]), _ptr(rev["col"]), rev_et, mask,
            _ptr(fwd_heavy), fwd_heavy.numel(),
            _ptr(rev_heavy), rev_heavy.numel(),
            _ptr(chunk), chunk.numel(), num_nodes,
            _ptr(dist), _ptr(sigma), _ptr(delta), _ptr(bc), _ptr(counter), _stream(),
        )
        if rc < 0:
            _check(-rc, "abom_brandes_run")
        ws["bc_deepest"] = max(rc, ws.get("bc_deepest", 0) if lo else 0)
    return bc


# ── Connected components (ops/csrc/components.hip) ─────────────────────────

# component_stats packs one 8-bit counter per node class (CC_MAX_KINDS)
COMPONENT_MAX_KINDS = 8


def _require(t, name: str, dtype, dev, numel: Optional[int] = None) -> None:
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.device != dev:
        raise ValueError(f"{name}: on {t.device}, expected {dev}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: {t.numel()} elements, expected {numel}")


def components_max_rounds(num_nodes: int) -> int:
    """Default round cap of :func:`connected_components`: ``num_nodes + 1``.

    A round that hooks anything turns at least one root into a non-root, and
    a non-root never becomes a root again (csrc/components.hip, header).  N
    nodes start as N roots and at least one survives, so at most N-1 rounds
    hook; the round after them hooks nothing and ends the loop.  N rounds
    therefore always suffice, whatever the schedule, and the one on top keeps
    the cap itself out of reach: hitting it means the engine is broken, not
    that the graph was hard.  Real graphs take a handful of rounds.
    """
    return min(int(num_nodes) + 1, (1 << 31) - 2)


def connected_components(edge_src, col, num_nodes: int, etype=None,
                         allowed_mask: Optional[int] = None, workspace: Optional[dict] = None,
                         max_rounds: Optional[int] = None):
    """Weakly connected components of an edge list; int32 labels [N].

    ``edge_src`` / ``col`` are int32 [E] device tensors (edge e joins
    ``edge_src[e]`` and ``col[e]``; direction is ignored, self-loops and
    parallel edges are harmless).  ``labels[v]`` is the smallest node id of
    v's component, so the result is the same bit for bit on every run.
    ``allowed_mask`` keeps only the edges whose ``etype`` (uint8 [E]) bit is
    set; None walks every edge.  Raises if ``max_rounds`` (default
    :func:`components_max_rounds`) rounds did not reach the fixed point;
    unconverged labels are never returned.  ``workspace["cc_rounds"]`` is
    left holding the rounds run.
    """
    import torch

    lib = load()
    num_nodes = int(num_nodes)
    if not 0 <= num_nodes < 1 << 31:
        raise ValueError(f"connected_components: num_nodes {num_nodes} outside [0, 2^31)")
    dev = edge_src.device
    if dev.type != "cuda":
        raise ValueError(f"connected_components: edge_src on {dev}, expected a GPU tensor")
    num_edges = edge_src.numel()
    _require(edge_src, "edge_src", torch.int32, dev)
    _require(col, "col", torch.int32, dev, num_edges)
    et, mask = None, 0xFFFFFFFF
    if allowed_mask is not None:
        if etype is None:
            raise ValueError("connected_components: allowed_mask needs etype")
        _require(etype, "etype", torch.uint8, dev, num_edges)
        et, mask = _ptr(etype), int(allowed_mask) & 0xFFFFFFFF
    if max_rounds is None:
        max_rounds = components_max_rounds(num_nodes)
    ws = workspace if workspace is not None else {}
    labels = torch.empty(num_nodes, dtype=torch.int32, device=dev)
    counters = _buf(ws, "cc_counters", 1, torch.int32, dev, zero=True)
    rc = lib.abom_components_run(
        _ptr(edge_src), _ptr(col), et, mask, num_edges, num_nodes,
        _ptr(labels), _ptr(counters), int(max_rounds), _stream(),
    )
    if rc < 0:
        _check(-rc, "abom_components_run")
    if rc > max_rounds:
        raise RuntimeError(
            f"connected_components: no fixed point after {max_rounds} rounds")
    ws["cc_rounds"] = rc
    return labels


def component_stats(comp, kind, num_components: int, num_kinds: int, weight=None, worst=None):
    """Per-component roll-up of node columns; integer atomics only, so the
    result is bit-reproducible.

    ``comp`` int32 [N] is a dense component index in [0, num_components),
    ``kind`` uint8 [N] a node class in [0, num_kinds) (at most 8 classes),
    ``weight`` int32 [N] and ``worst`` uint8 [N] (lower is worse) are
    optional.  Returns ``(kind_counts int32 [C, num_kinds], weight_sum int64
    [C], worst_min int32 [C])``; without ``weight`` the sums are 0, without
    ``worst`` worst_min is -1 (the u32 fill pattern).
    """
    import torch

    lib = load()
    dev = comp.device
    if dev.type != "cuda":
        raise ValueError(f"component_stats: comp on {dev}, expected a GPU tensor")
    n, C, K = comp.numel(), int(num_components), int(num_kinds)
    if not 1 <= K <= COMPONENT_MAX_KINDS:
        raise ValueError(f"component_stats: num_kinds {K} outside [1, {COMPONENT_MAX_KINDS}]")
    if not 0 <= C < 1 << 31:
        raise ValueError(f"component_stats: num_components {C} outside [0, 2^31)")
    _require(comp, "comp", torch.int32, dev)
    _require(kind, "kind", torch.uint8, dev, n)
    if weight is not None:
        _require(weight, "weight", torch.int32, dev, n)
    if worst is not None:
        _require(worst, "worst", torch.uint8, dev, n)
    kind_counts = torch.zeros(C * K, dtype=torch.int32, device=dev)
    weight_sum = torch.zeros(C, dtype=torch.int64, device=dev)
    worst_min = torch.full((C,), -1, dtype=torch.int32, device=dev)
    rc = lib.abom_component_stats(
        _ptr(comp), _ptr(kind),
        _ptr(weight) if weight is not None else None,
        _ptr(worst) if worst is not None else None,
        n, C, K, _ptr(kind_counts), _ptr(weight_sum), _ptr(worst_min), _stream(),
    )
    _check(rc, "abom_component_stats")
    return kind_counts.view(C, K), weight_sum, worst_min
