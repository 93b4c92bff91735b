"""Indexed blast counts (ops/csrc/blast.hip, abom_blast_counts_indexed)
against the exact sort-based join ``EstateEngine._blast_counts_join``.

Every comparison is ``torch.equal`` on all six count keys.  The overflow
fallback of ``_blast_counts_fused`` is itself the join, so the tests also
look at the kernels' own overflow flags: few rows may take the fallback.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

from agentbom_amd.scan.synth import (
    ET_CONTAINS, ET_HAS_CRED, ET_PROVIDES_TOOL, ET_USES, generate_estate)

pytestmark = pytest.mark.gpu

KEYS = ("n_servers", "n_agents", "n_creds_all", "n_creds_db", "n_tools_all", "n_tools_db")
SRV_CAP = 64    # caps of ops/csrc/blast.hip
TL_CAP = 512


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _engine(est, dev):
    from agentbom_amd.graph.gpu_engine import EstateEngine

    return EstateEngine(est, device=str(dev))


def _all_packages(est, dev):
    return torch.arange(est.pkg_base, est.pkg_base + est.n_packages,
                        dtype=torch.int64, device=dev)


def _native_indexed(eng, pkgs):
    """(counts, overflow flags, overflow word, queue length) of the kernels."""
    from agentbom_amd.ops import native

    counts, overflow, n_overflow = native.blast_counts_indexed(
        pkgs.to(torch.int32).contiguous(), eng.rev, eng.reach_index, ET_CONTAINS,
        eng.node_is_db_cred, eng.node_is_db_tool, eng._blast_ws)
    return counts, overflow, n_overflow, int(eng._blast_ws["counters"][0].item())


def _servers_per_package(est):
    """Distinct containing servers per package index (numpy)."""
    m = est.edge_type == ET_CONTAINS
    pairs = np.unique(np.stack([est.edge_dst[m] - est.pkg_base, est.edge_src[m]], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=est.n_packages)


def _assert_equal(got, want):
    for key in KEYS:
        assert torch.equal(got[key], want[key]), key
    assert torch.equal(got["uniq_pkgs"], want["uniq_pkgs"])


# ── test 1 and 3: random estate ────────────────────────────────────────────


@pytest.fixture(scope="module")
def random_case(dev):
    est = generate_estate(n_agents=50, n_servers=200, n_packages=3000,
                          name_catalog=500, extra_pkg_share=2.0, seed=7)
    eng = _engine(est, dev)
    pkgs = _all_packages(est, dev)
    return est, eng, pkgs, eng._blast_counts_join(pkgs)


def test_random_estate_matches_join(random_case):
    est, eng, pkgs, want = random_case
    got = eng._blast_counts_fused(pkgs)
    _assert_equal(got, want)
    counts2d = got["counts2d"]
    assert counts2d.shape == (est.n_packages, 6) and counts2d.dtype == torch.int32
    for k, key in enumerate(KEYS):
        assert torch.equal(counts2d[:, k], want[key]), key


def test_random_estate_fallback_cannot_hide_the_kernels(random_case):
    est, eng, pkgs, want = random_case
    counts, overflow, n_overflow, n_queued = _native_indexed(eng, pkgs)
    per_pkg = _servers_per_package(est)
    flagged = overflow.cpu().numpy().astype(bool)
    n = est.n_packages
    print(f"packages {n}, multi-server {int((per_pkg > 1).sum())}, queued {n_queued}, "
          f"flagged {int(flagged.sum())}, overflow word {n_overflow}, max servers {per_pkg.max()}")
    assert flagged.sum() >= 1
    assert flagged.sum() <= 0.05 * n
    assert n_overflow == int(flagged.sum())
    assert n_queued == int((per_pkg > 1).sum())
    # the SRV_CAP boundary: 64 distinct servers fit, 65 do not
    assert (per_pkg == SRV_CAP).sum() >= 1
    assert not flagged[per_pkg == SRV_CAP].any()
    assert flagged[per_pkg > SRV_CAP].all()
    # rows the kernels answered themselves equal the join
    keep = torch.from_numpy(~flagged).to(counts.device)
    for k, key in enumerate(KEYS):
        assert torch.equal(counts[keep, k], want[key][keep]), key


def test_index_off_uses_the_row_walk_kernel(random_case, monkeypatch):
    est, eng, pkgs, want = random_case
    with_index = eng._blast_counts_fused(pkgs)
    monkeypatch.setenv("AGENT_BOM_BLAST_INDEX", "0")
    eng._blast_ws["counters"].fill_(-1)
    without = eng._blast_counts_fused(pkgs)
    # the indexed entry point did not run: it would have reset its counters
    assert eng._blast_ws["counters"].tolist() == [-1, -1]
    _assert_equal(without, with_index)
    assert torch.equal(without["counts2d"], with_index["counts2d"])


def test_second_call_resets_queue_and_overflow_word(random_case):
    est, eng, pkgs, want = random_case
    per_pkg = _servers_per_package(est)
    _, _, first_overflow, first_queued = _native_indexed(eng, pkgs)
    assert first_overflow > 0 and first_queued > 0
    # shorter list without any overflowing package
    idx = np.nonzero(per_pkg <= SRV_CAP)[0][::7]
    short = pkgs[torch.from_numpy(idx).to(pkgs.device)]
    counts, overflow, n_overflow, n_queued = _native_indexed(eng, short)
    assert n_overflow == 0 and int(overflow.sum().item()) == 0
    assert n_queued == int((per_pkg[idx] > 1).sum())
    _assert_equal(eng._blast_counts_fused(short), eng._blast_counts_join(short))


# ── test 2: hand-built edge lists ──────────────────────────────────────────


def _hand_estate():
    base = generate_estate(n_agents=8, n_servers=160, n_packages=16,
                           name_catalog=8, seed=3)
    A, S, C, T, P = (base.agent_base, base.server_base, base.cred_base,
                     base.tool_base, base.pkg_base)
    edges = []

    def add(etype, src, dst, times=1):
        edges.extend([(src, dst, etype)] * times)

    pk = {name: P + i for i, name in enumerate(
        ("none", "triple", "bare", "last", "last_pair", "shared", "fit", "over"))}
    # triple: one server, listed three times; its own edges carry duplicates
    add(ET_CONTAINS, S + 131, pk["triple"], times=3)
    add(ET_USES, A + 1, S + 131, times=2)
    add(ET_USES, A + 2, S + 131)
    add(ET_HAS_CRED, S + 131, C + 5, times=2)
    add(ET_HAS_CRED, S + 131, C + 6)
    add(ET_PROVIDES_TOOL, S + 131, T + 9, times=3)
    # bare: a server with no agent, no cred and no tool
    add(ET_CONTAINS, S + 130, pk["bare"])
    # last: the highest-numbered server, alone and together with another one
    add(ET_USES, A + 7, S + 159)
    add(ET_HAS_CRED, S + 159, C + 79)
    add(ET_PROVIDES_TOOL, S + 159, T + 159)
    add(ET_PROVIDES_TOOL, S + 159, T + 158)
    add(ET_CONTAINS, S + 159, pk["last"])
    add(ET_CONTAINS, S + 159, pk["last_pair"])
    add(ET_CONTAINS, S + 131, pk["last_pair"])
    # shared: two servers with one agent, cred and tool in common
    for srv, own in ((S + 132, 0), (S + 133, 1)):
        add(ET_CONTAINS, srv, pk["shared"])
        add(ET_USES, A + 3, srv)
        add(ET_USES, A + 4 + own, srv)
        add(ET_HAS_CRED, srv, C + 10)
        add(ET_HAS_CRED, srv, C + 11 + own)
        add(ET_PROVIDES_TOOL, srv, T + 20)
        add(ET_PROVIDES_TOOL, srv, T + 21 + own)
    # fit: 64 servers (two of them listed twice) x 8 tools = 512 candidates;
    # over: 64 servers, 513 candidates
    for name, first in (("fit", 0), ("over", 64)):
        for i in range(64):
            add(ET_CONTAINS, S + first + i, pk[name], times=2 if name == "fit" and i in (0, 63) else 1)
            for k in range(8):
                add(ET_PROVIDES_TOOL, S + first + i, T + (i * 8 + k) % base.n_tools)
    add(ET_PROVIDES_TOOL, S + 64, T + 100)
    src, dst, et = (np.array(col) for col in zip(*edges))
    est = dataclasses.replace(base, edge_src=src.astype(np.int64),
                              edge_dst=dst.astype(np.int64), edge_type=et.astype(np.uint8))
    return est, pk


def test_hand_built_cases(dev):
    est, pk = _hand_estate()
    eng = _engine(est, dev)
    pkgs = _all_packages(est, dev)
    want = eng._blast_counts_join(pkgs)
    _assert_equal(eng._blast_counts_fused(pkgs), want)

    counts, overflow, n_overflow, n_queued = _native_indexed(eng, pkgs)
    counts, overflow = counts.cpu().numpy(), overflow.cpu().numpy()
    row = {name: node - est.pkg_base for name, node in pk.items()}
    db_c = lambda *ids: int(sum(est.cred_is_db[i] for i in ids))  # noqa: E731
    db_t = lambda *ids: int(sum(est.tool_is_db[i] for i in ids))  # noqa: E731
    assert counts[row["none"]].tolist() == [0, 0, 0, 0, 0, 0]
    assert counts[row["triple"]].tolist() == [1, 2, 2, db_c(5, 6), 1, db_t(9)]
    assert counts[row["bare"]].tolist() == [1, 0, 0, 0, 0, 0]
    assert counts[row["last"]].tolist() == [1, 1, 1, db_c(79), 2, db_t(158, 159)]
    assert counts[row["last_pair"]].tolist() == [
        2, 3, 3, db_c(5, 6, 79), 3, db_t(9, 158, 159)]
    assert counts[row["shared"]].tolist() == [
        2, 3, 3, db_c(10, 11, 12), 3, db_t(20, 21, 22)]
    # 512 tool candidates fit the cap, 513 do not
    assert overflow[row["fit"]] == 0
    assert counts[row["fit"], 0] == 64 and counts[row["fit"], 4] == est.n_tools
    assert overflow[row["over"]] == 1
    assert n_overflow == 1 and int(overflow.sum()) == 1
    assert n_queued == 4  # last_pair, shared, fit, over
    # packages beyond the named ones have no edges at all
    assert not counts[len(pk):].any()
