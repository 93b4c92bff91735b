"""The per-server reach index (graph/gpu_engine.py build_reach_index) against
a brute-force set computation over the estate's edge arrays.  Runs on CPU
tensors through the same builder the GPU engine calls."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from agentbom_amd.graph.gpu_engine import build_reach_index
from agentbom_amd.scan.synth import (
    ET_CONTAINS, ET_HAS_CRED, ET_PROVIDES_TOOL, ET_USES, generate_estate)


@pytest.fixture(scope="module")
def estate():
    return generate_estate(n_agents=50, n_servers=200, n_packages=3000,
                           name_catalog=500, extra_pkg_share=2.0, seed=7)


def _db_flags(est):
    cred = np.zeros(est.num_nodes, dtype=np.uint8)
    cred[est.cred_base:est.cred_base + est.n_creds] = est.cred_is_db
    tool = np.zeros(est.num_nodes, dtype=np.uint8)
    tool[est.tool_base:est.tool_base + est.n_tools] = est.tool_is_db
    return cred, tool


@pytest.fixture(scope="module")
def built(estate):
    cred, tool = _db_flags(estate)
    index = build_reach_index(
        torch, torch.from_numpy(estate.edge_src), torch.from_numpy(estate.edge_dst),
        torch.from_numpy(estate.edge_type), estate.server_base, estate.n_servers,
        torch.from_numpy(cred), torch.from_numpy(tool))
    return index, cred, tool


def test_estate_exercises_dedup_and_empty_segments(estate):
    src, dst, et = estate.edge_src, estate.edge_dst, estate.edge_type
    cred_pairs = np.stack([src[et == ET_HAS_CRED], dst[et == ET_HAS_CRED]], 1)
    assert len(cred_pairs) - len(np.unique(cred_pairs, axis=0)) > 0
    holds = np.stack([src[et == ET_CONTAINS], dst[et == ET_CONTAINS]], 1)
    assert len(holds) - len(np.unique(holds, axis=0)) > 0
    servers = np.arange(estate.server_base, estate.server_base + estate.n_servers)
    assert np.setdiff1d(servers, src[et == ET_HAS_CRED]).size > 0


def test_layout(estate, built):
    index, _, _ = built
    off, col, db = index["reach_off"], index["reach_col"], index["reach_db"]
    assert index["row_base"] == estate.server_base
    assert off.dtype == torch.int32 and col.dtype == torch.int32 and db.dtype == torch.int32
    assert off.shape == (estate.n_servers, 4) and db.shape == (estate.n_servers, 2)
    assert off.is_contiguous() and col.is_contiguous() and db.is_contiguous()
    off = off.numpy()
    assert off[0, 0] == 0
    assert (off[1:, 0] == off[:-1, 3]).all()      # rows chain
    assert off[-1, 3] == col.numel()              # last end == T
    assert (np.diff(off, axis=1) >= 0).all()


def test_segments_match_brute_force(estate, built):
    index, cred_flag, tool_flag = built
    off = index["reach_off"].numpy()
    col = index["reach_col"].numpy()
    db = index["reach_db"].numpy()
    src, dst, et = estate.edge_src, estate.edge_dst, estate.edge_type

    agents, creds, tools = {}, {}, {}
    for s, d, t in zip(src.tolist(), dst.tolist(), et.tolist()):
        if t == ET_USES:
            agents.setdefault(d, set()).add(s)
        elif t == ET_HAS_CRED:
            creds.setdefault(s, set()).add(d)
        elif t == ET_PROVIDES_TOOL:
            tools.setdefault(s, set()).add(d)

    empty_seen = 0
    for r in range(estate.n_servers):
        node = estate.server_base + r
        segs = [col[off[r, k]:off[r, k + 1]] for k in range(3)]
        for seg, want in zip(segs, (agents, creds, tools)):
            assert (np.diff(seg) > 0).all(), f"server {node}: segment not strictly ascending"
            assert seg.tolist() == sorted(want.get(node, ())), f"server {node}"
            empty_seen += seg.size == 0
        assert db[r, 0] == sum(int(cred_flag[c]) for c in creds.get(node, ()))
        assert db[r, 1] == sum(int(tool_flag[c]) for c in tools.get(node, ()))
    assert empty_seen > 0


def test_rows_cover_contains_sources_outside_the_server_range(estate):
    """A CONTAINS edge whose source lies outside [server_base, +n_servers)
    widens the row range, so the kernels can index every containing node."""
    src = estate.edge_src.copy()
    first_contains = int(np.nonzero(estate.edge_type == ET_CONTAINS)[0][0])
    src[first_contains] = 3  # an agent id, below server_base
    cred, tool = _db_flags(estate)
    index = build_reach_index(
        torch, torch.from_numpy(src), torch.from_numpy(estate.edge_dst),
        torch.from_numpy(estate.edge_type), estate.server_base, estate.n_servers,
        torch.from_numpy(cred), torch.from_numpy(tool))
    assert index["row_base"] == 3
    rows = estate.server_base + estate.n_servers - 3
    assert index["reach_off"].shape == (rows, 4)
    off = index["reach_off"].numpy()
    assert (off[1:, 0] == off[:-1, 3]).all() and off[-1, 3] == index["reach_col"].numel()
