"""The wave pass of the indexed blast counts (ops/csrc/blast.hip,
blast_index_wave_kernel) on packages that make its first-occurrence scan
work: many servers, long segments, duplicates at every offset of the scan's
four-wide step.  Counts are compared with the exact join
``EstateEngine._blast_counts_join`` through ``abom_blast_counts_indexed``
and ``abom_blast_counts_indexed_sized``; which rows overflow and what the
two counters hold is computed from the edge list.  Every comparison is exact.
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
G, C = 16, 64                      # sizes around which the cases are built
SRV_CAP, AG_CAP, CR_CAP, TL_CAP = 64, 256, 256, 512   # caps of csrc/blast.hip
GRID_ROUND = 2048 * 4              # waves of one full grid of the wave kernel
OUTSIDE = 8                        # servers left out of the sliced index
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def toggles(monkeypatch):
    for name in ("AGENT_BOM_BLAST_INDEX",):
        monkeypatch.delenv(name, raising=False)


# ── hand-built edge lists ──────────────────────────────────────────────────


class Builder:
    def __init__(self):
        self.base = generate_estate(n_agents=300, n_servers=800, n_packages=128,
                                    name_catalog=8, seed=3)
        self.edges = []
        self.next_server = 0
        self.next_nbr = {ET_USES: 0, ET_HAS_CRED: 0, ET_PROVIDES_TOOL: 0}
        self.names = {}

    def _nbr(self, et, i):
        b = self.base
        if et == ET_USES:
            return b.agent_base + i % b.n_agents
        if et == ET_HAS_CRED:
            return b.cred_base + i % b.n_creds
        return b.tool_base + i % b.n_tools

    def server(self, n_ag=1, n_cr=1, n_tl=1, fixed=None):
        """A fresh server with that many distinct agents, creds and tools:
        the next unused ones, or ``fixed[et]`` = explicit indices."""
        b = self.base
        assert self.next_server < b.n_servers - OUTSIDE
        s = b.server_base + self.next_server
        self.next_server += 1
        for et, n in ((ET_USES, n_ag), (ET_HAS_CRED, n_cr), (ET_PROVIDES_TOOL, n_tl)):
            ids = fixed[et] if fixed else range(self.next_nbr[et], self.next_nbr[et] + n)
            if not fixed:
                self.next_nbr[et] += n
            for i in ids:
                o = self._nbr(et, i)
                self.edges.append((o, s, et) if et == ET_USES else (s, o, et))
        return s

    def outside_server(self, k):
        b = self.base
        s = b.server_base + b.n_servers - OUTSIDE + k
        self.edges.append((b.agent_base, s, ET_USES))
        return s

    def package(self, name, servers):
        p = self.base.pkg_base + len(self.names)
        assert len(self.names) < self.base.n_packages
        self.names[name] = p
        for s in servers:
            self.edges.append((s, p, ET_CONTAINS))
        return p

    def spread(self, name, n_srv, kind, total):
        """n_srv servers whose `kind` segments add up to `total` before dedup."""
        per, extra = divmod(total, n_srv)
        servers = []
        for i in range(n_srv):
            n = per + (1 if i < extra else 0)
            sizes = {ET_USES: 1, ET_HAS_CRED: 1, ET_PROVIDES_TOOL: 1}
            sizes[kind] = n
            servers.append(self.server(sizes[ET_USES], sizes[ET_HAS_CRED],
                                       sizes[ET_PROVIDES_TOOL]))
        return self.package(name, servers)

    def estate(self):
        src, dst, et = (np.array(col) for col in zip(*self.edges))
        return dataclasses.replace(self.base, edge_src=src.astype(np.int64),
                                   edge_dst=dst.astype(np.int64),
                                   edge_type=et.astype(np.uint8))


def _build():
    b = Builder()
    b.package("none", [])
    b.package("single", [b.server(2, 3, 4)])
    for k in (2, G - 1, G, G + 1, 63, 64, 65):
        b.package(f"srv{k}", [b.server() for _ in range(k)])
    same = {ET_USES: [290, 291, 292, 293], ET_HAS_CRED: [390, 391, 392, 393],
            ET_PROVIDES_TOOL: [790, 791, 792, 793]}
    b.package("share_all", [b.server(fixed=same) for _ in range(3)])
    b.package("share_none", [b.server(3, 3, 3) for _ in range(3)])
    s1, s2 = b.server(2, 2, 2), b.server(2, 2, 2)
    b.package("twice", [s1, s2, s1])
    # two servers with the same k tools: entry i repeats entry i - k, so the
    # repeat sits at every offset of the scan's groups of four and in its tail
    for k in range(1, 10):
        same_k = {ET_USES: [280], ET_HAS_CRED: [380], ET_PROVIDES_TOOL: range(700, 700 + k)}
        b.package(f"repeat{k}", [b.server(fixed=same_k), b.server(fixed=same_k)])
    # 70 edges: whatever order the CSR keeps, one server sits on both sides
    # of the row's 64th edge (and of every 16th)
    ten = [b.server(1, 2, 3) for _ in range(10)]
    b.package("chunks", ten * 7)
    b.package("outside_second", [b.server(), b.outside_server(0)])
    b.package("outside_single", [b.outside_server(1)])
    for kind, tag in ((ET_USES, "ag"), (ET_HAS_CRED, "cr"), (ET_PROVIDES_TOOL, "tl")):
        for total in (C - 1, C, C + 1):
            b.spread(f"{tag}{total}", 8, kind, total)
    for kind, tag, cap in ((ET_USES, "ag", AG_CAP), (ET_HAS_CRED, "cr", CR_CAP),
                           (ET_PROVIDES_TOOL, "tl", TL_CAP)):
        b.spread(f"{tag}{cap}", 64, kind, cap)
        b.spread(f"{tag}{cap + 1}", 64, kind, cap + 1)
    return b.estate(), b.names


def _spec(est, index, rows):
    """Per package of the estate, from the edge list alone: distinct servers,
    multi-server and must-overflow."""
    P, S = est.pkg_base, est.server_base
    m = est.edge_type == ET_CONTAINS
    ps = np.unique(np.stack([est.edge_dst[m] - P, est.edge_src[m]], 1), axis=0)

    def per_server(et, server_is_dst):
        mm = est.edge_type == et
        srv, other = ((est.edge_dst[mm], est.edge_src[mm]) if server_is_dst
                      else (est.edge_src[mm], est.edge_dst[mm]))
        u = np.unique(np.stack([srv, other], 1), axis=0)
        return np.bincount(u[:, 0] - S, minlength=est.n_servers)

    n = est.n_packages
    nsrv = np.bincount(ps[:, 0], minlength=n)
    outside = np.bincount(ps[:, 0], weights=(ps[:, 1] - index["row_base"] >= rows),
                          minlength=n) > 0
    tot = [np.bincount(ps[:, 0], weights=seg[ps[:, 1] - S], minlength=n)
           for seg in (per_server(ET_USES, True), per_server(ET_HAS_CRED, False),
                       per_server(ET_PROVIDES_TOOL, False))]
    multi = nsrv > 1
    over_cap = (tot[0] > AG_CAP) | (tot[1] > CR_CAP) | (tot[2] > TL_CAP)
    overflow = outside | (nsrv > SRV_CAP) | (multi & over_cap)
    return {"nsrv": nsrv, "multi": multi, "overflow": overflow}


class Hand:
    def __init__(self, dev):
        from agentbom_amd.graph.gpu_engine import EstateEngine

        self.est, self.names = _build()
        self.eng = EstateEngine(self.est, device=str(dev))
        full = self.eng.reach_index
        self.rows = full["reach_off"].shape[0] - OUTSIDE
        assert full["row_base"] == self.est.server_base
        assert full["reach_off"].shape[0] == self.est.n_servers
        # the last OUTSIDE servers have no row
        self.index = dict(full, reach_off=full["reach_off"][:self.rows].contiguous(),
                          reach_db=full["reach_db"][:self.rows].contiguous())
        self.spec = _spec(self.est, self.index, self.rows)
        all_pkgs = torch.arange(self.est.pkg_base, self.est.pkg_base + self.est.n_packages,
                                dtype=torch.int64, device=dev)
        join = self.eng._blast_counts_join(all_pkgs)
        self.want = torch.stack([join[k].to(torch.int32) for k in KEYS], 1)  # [P, 6]
        self.dev = dev

    def row(self, name):
        return self.names[name] - self.est.pkg_base


@pytest.fixture(scope="module")
def hand(dev):
    return Hand(dev)


def _run(h, rows, entry, n_dev=None, index=None, eng=None):
    """The kernels over the packages at ``rows`` (indices, repeats allowed).
    Returns counts [n, 6], flags [n], counters [2] and the queue, as numpy;
    ``n_dev`` (sized entry only) is the device count, the rest of the
    buffers starts as SENTINEL bytes."""
    from agentbom_amd.ops import native

    eng = eng or h.eng
    index = index or h.index
    dev = h.dev
    rows = np.asarray(rows, dtype=np.int64)
    n_cap = rows.size
    pkgs = torch.from_numpy(rows + h.est.pkg_base).to(torch.int32).to(dev)
    counts = torch.full((n_cap * 6,), SENTINEL, dtype=torch.int32, device=dev)
    flags = torch.full((n_cap,), SENTINEL, dtype=torch.uint8, device=dev)
    queue = torch.zeros(max(n_cap, 1), dtype=torch.int32, device=dev)
    counters = torch.full((2,), -1, dtype=torch.int32, device=dev)
    lib = native.load()
    p = native._ptr
    common = (p(eng.rev["row_off"]), p(eng.rev["col"]), p(eng.rev["etype"]), ET_CONTAINS,
              p(index["reach_off"]), p(index["reach_col"]), p(index["reach_db"]),
              index["row_base"], index["reach_off"].shape[0],
              p(eng.node_is_db_cred), p(eng.node_is_db_tool))
    if entry == "plain":
        assert n_dev is None
        rc = lib.abom_blast_counts_indexed(
            p(pkgs), n_cap, *common, p(queue), p(counters), p(counts), p(flags),
            native._stream())
        host = None
    else:
        n = n_cap if n_dev is None else n_dev
        word = torch.tensor([n], dtype=torch.int64, device=dev)
        host = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        rc = lib.abom_blast_counts_indexed_sized(
            p(pkgs), p(word), n_cap, *common, p(queue), p(counters), p(host), p(counts),
            p(flags), native._stream())
    native._check(rc, entry)
    torch.cuda.synchronize()
    if host is not None:
        assert host.tolist() == counters.tolist()
    return (counts.view(n_cap, 6).cpu().numpy(), flags.cpu().numpy(),
            counters.cpu().numpy(), queue.cpu().numpy())


def _check(h, rows, got, n=None):
    """Everything the kernels left behind for the first ``n`` input rows."""
    rows = np.asarray(rows, dtype=np.int64)
    n = rows.size if n is None else n
    counts, flags, counters, queue = got
    want = h.want.cpu().numpy()
    head = rows[:n]
    over = h.spec["overflow"][head]
    assert np.array_equal(flags[:n], over.astype(np.uint8))
    assert np.array_equal(counts[:n][~over], want[head][~over])
    assert not counts[:n][over].any()           # an overflowed row carries six zeros
    # rows at or beyond the device count are not touched
    assert (flags[n:] == SENTINEL).all() and (counts[n:] == SENTINEL).all()
    n_queued = int(h.spec["multi"][head].sum())
    assert counters.tolist() == [n_queued, int(over.sum())]
    # every multi-server input position is queued exactly once
    position = queue[:n_queued].astype(np.int64)
    assert np.array_equal(np.sort(position), np.nonzero(h.spec["multi"][head])[0])


ENTRIES = ("plain", "sized")


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_hand_built_package(hand, entry):
    h = hand
    rows = np.arange(h.est.n_packages)
    got = _run(h, rows, entry)
    _check(h, rows, got)
    counts, flags = got[0], got[1]
    # the cases are what their names say
    spec = h.spec
    for k in (2, G - 1, G, G + 1, 63, 64, 65):
        r = h.row(f"srv{k}")
        assert spec["nsrv"][r] == k
        assert bool(flags[r]) == (k > SRV_CAP)
        if k <= SRV_CAP:
            assert counts[r].tolist()[:3] == [k, k, k] and counts[r][4] == k
    assert counts[h.row("share_all")].tolist()[:3] == [3, 4, 4]
    assert counts[h.row("share_all")][4] == 4
    assert counts[h.row("share_none")].tolist()[:3] == [3, 9, 9]
    assert counts[h.row("twice")].tolist()[:3] == [2, 4, 4]
    for k in range(1, 10):
        assert counts[h.row(f"repeat{k}")].tolist()[:3] == [2, 1, 1]
        assert counts[h.row(f"repeat{k}")][4] == k
    assert counts[h.row("chunks")].tolist()[:3] == [10, 10, 20]
    assert counts[h.row("chunks")][4] == 30
    assert flags[h.row("outside_second")] == 1 and flags[h.row("outside_single")] == 1
    for tag, col in (("ag", 1), ("cr", 2), ("tl", 4)):
        for total in (C - 1, C, C + 1):
            r = h.row(f"{tag}{total}")
            assert flags[r] == 0 and counts[r][col] == total
    for tag, cap in (("ag", AG_CAP), ("cr", CR_CAP), ("tl", TL_CAP)):
        assert flags[h.row(f"{tag}{cap}")] == 0 and flags[h.row(f"{tag}{cap + 1}")] == 1
    # db and non-db entries are mixed: the db counts differ from the totals
    want = h.want.cpu().numpy()
    live = ~spec["overflow"] & spec["multi"]
    assert (want[live][:, 3] < want[live][:, 2]).any() and (want[live][:, 3] > 0).any()
    assert (want[live][:, 5] < want[live][:, 4]).any() and (want[live][:, 5] > 0).any()


def test_fused_path_with_the_fallback_equals_the_join(hand, dev):
    h = hand
    pkgs = torch.arange(h.est.pkg_base, h.est.pkg_base + h.est.n_packages,
                        dtype=torch.int64, device=dev)
    got = h.eng._blast_counts_fused(pkgs)
    for k, key in enumerate(KEYS):
        assert torch.equal(got[key], h.want[:, k]), key


def _queue_rows(h, length):
    """`length` multi-server packages, light and heavy ones mixed."""
    multi = np.nonzero(h.spec["multi"])[0]
    return multi[np.arange(length) % multi.size]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("length", [1, 3, 4, 5, 255, 256, 257, GRID_ROUND + 1])
def test_queue_lengths(hand, entry, length):
    rows = _queue_rows(hand, length)
    _check(hand, rows, _run(hand, rows, entry))


@pytest.mark.parametrize("entry", ENTRIES)
def test_light_and_heavy_packages_side_by_side(hand, entry):
    h = hand
    rows = np.array([h.row("srv2"), h.row("srv64"), h.row("srv2"), h.row("srv64"),
                     h.row("srv16"), h.row("tl512"), h.row("chunks")])
    _check(h, rows, _run(h, rows, entry))


@pytest.mark.parametrize("n_dev", [0, 1, 40, 300])
def test_sized_entry_reads_the_device_count(hand, n_dev):
    rows = np.arange(300) % hand.est.n_packages
    _check(hand, rows, _run(hand, rows, "sized", n_dev=n_dev), n=n_dev)


# ── the seed-7 estate of tests/test_blast_index_gpu.py ─────────────────────


def test_seed7_estate_rows_the_kernels_answer_equal_the_join(dev):
    from agentbom_amd.graph.gpu_engine import EstateEngine

    est = generate_estate(n_agents=50, n_servers=200, n_packages=3000,
                          name_catalog=500, extra_pkg_share=2.0, seed=7)
    eng = EstateEngine(est, device=str(dev))

    class Seed7:
        pass

    h = Seed7()
    h.est, h.eng, h.dev, h.index = est, eng, dev, eng.reach_index
    rows = np.arange(est.n_packages)
    pkgs = torch.arange(est.pkg_base, est.pkg_base + est.n_packages,
                        dtype=torch.int64, device=dev)
    join = eng._blast_counts_join(pkgs)
    want = torch.stack([join[k].to(torch.int32) for k in KEYS], 1).cpu().numpy()
    for entry in ENTRIES:
        counts, flags, counters, _queue = _run(h, rows, entry)
        keep = flags == 0
        assert set(np.unique(flags)) <= {0, 1}
        assert np.array_equal(counts[keep], want[keep]), entry
        assert not counts[~keep].any()
        assert counters[0] > 100 and counters[1] == int((~keep).sum()) >= 1
