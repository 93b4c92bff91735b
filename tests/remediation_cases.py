"""Hand-built inputs for the remediation plan (``cpu_ref.remediation_plan``,
``native.remediation_items``): a few agents, servers, creds, tools and
packages given as edge lists, laid out like an estate (agents first, then
servers, creds, tools, packages), a handful of advisory windows and a list of
findings.  ``item_of`` is given per package; the installs of one item carry
the same windows, as a step's findings do.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from agentbom_amd.ops import cpu_ref
from agentbom_amd.scan.synth import ET_CONTAINS, ET_HAS_CRED, ET_PROVIDES_TOOL, ET_USES

FIXED = cpu_ref.WF_HAS_FIXED
TOP = 1 << 63  # a word with bit 63 set: larger than any small word, unsigned


@dataclass
class RemedCase:
    name: str
    n_agents: int
    n_servers: int
    n_creds: int
    n_tools: int
    n_pkgs: int
    uses: list        # (agent, server), local indices
    has_cred: list    # (server, cred)
    provides: list    # (server, tool)
    contains: list    # (server, package)
    item_of: list     # per package
    windows: list     # (flags, fixed_hi, fixed_lo, severity, kev)
    findings: list    # (package, window, score), packages ascending
    expected: dict = field(default_factory=dict)   # key -> per matched item
    expected_order: list = field(default_factory=list)

    @property
    def server_base(self) -> int:
        return self.n_agents

    @property
    def cred_base(self) -> int:
        return self.server_base + self.n_servers

    @property
    def tool_base(self) -> int:
        return self.cred_base + self.n_creds

    @property
    def pkg_base(self) -> int:
        return self.tool_base + self.n_tools

    @property
    def num_nodes(self) -> int:
        return self.pkg_base + self.n_pkgs

    def edges(self):
        """(src, dst, etype) in global node ids."""
        src, dst, et = [], [], []
        for a, s in self.uses:
            src.append(a), dst.append(s + self.server_base), et.append(ET_USES)
        for s, c in self.has_cred:
            src.append(s + self.server_base), dst.append(c + self.cred_base), et.append(ET_HAS_CRED)
        for s, t in self.provides:
            src.append(s + self.server_base), dst.append(t + self.tool_base)
            et.append(ET_PROVIDES_TOOL)
        for s, p in self.contains:
            src.append(s + self.server_base), dst.append(p + self.pkg_base), et.append(ET_CONTAINS)
        return (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64),
                np.asarray(et, dtype=np.uint8))

    def finding_arrays(self):
        f = self.findings
        return (np.asarray([x[0] for x in f], dtype=np.int64),
                np.asarray([x[1] for x in f], dtype=np.int64),
                np.asarray([x[2] for x in f], dtype=np.float32))

    def window_arrays(self):
        """(flags u8, fixed_hi i64, fixed_lo i64, severity u8, kev u8)"""
        w = self.windows
        return (np.asarray([x[0] for x in w], dtype=np.uint8),
                np.asarray([x[1] for x in w], dtype=np.uint64).view(np.int64),
                np.asarray([x[2] for x in w], dtype=np.uint64).view(np.int64),
                np.asarray([x[3] for x in w], dtype=np.uint8),
                np.asarray([x[4] for x in w], dtype=np.uint8))


def csr(src, dst, et, num_nodes: int):
    """(row_off int64 [N+1], col int32 [E], etype uint8 [E]), rows by ``src``."""
    order = np.argsort(src, kind="stable")
    row_off = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=num_nodes), out=row_off[1:])
    return row_off, dst[order].astype(np.int32), et[order]


def oracle(c: RemedCase) -> dict:
    """``cpu_ref.remediation_plan`` on the case."""
    src, dst, et = c.edges()
    flags, fhi, flo, sev, kev = c.window_arrays()
    return cpu_ref.remediation_plan(
        *c.finding_arrays(), np.asarray(c.item_of, dtype=np.int32),
        *csr(dst, src, et, c.num_nodes), *csr(src, dst, et, c.num_nodes),
        ET_CONTAINS, ET_USES, ET_HAS_CRED, ET_PROVIDES_TOOL, c.pkg_base,
        flags, fhi, flo, sev, kev, c.n_agents)


def device_inputs(c: RemedCase, device: str = "cuda") -> dict:
    """Keyword arguments of ``native.remediation_items`` (less workspace and
    pool size), the reach index built by the engine's own builder."""
    import torch

    from agentbom_amd.graph.gpu_engine import build_reach_index

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    src, dst, et = c.edges()
    off, col, etype = csr(dst, src, et, c.num_nodes)
    flag = torch.zeros(c.num_nodes, dtype=torch.uint8, device=device)
    index = build_reach_index(torch, dev(src), dev(dst), dev(et), c.server_base, c.n_servers,
                              flag, flag)
    pkg_idx, win_idx, scores = c.finding_arrays()
    flags, fhi, flo, sev, kev = c.window_arrays()
    return dict(
        pkg_idx=dev(pkg_idx), win_idx=dev(win_idx), scores=dev(scores),
        item_of=dev(np.asarray(c.item_of, dtype=np.int32)),
        n_items=max(c.item_of) + 1 if c.item_of else 0,
        arena={"windows": {"flags": dev(flags), "fixed_hi": dev(fhi), "fixed_lo": dev(flo)},
               "severity": dev(sev), "kev": dev(kev)},
        rev={"row_off": dev(off), "col": dev(col), "etype": dev(etype)},
        index=index, et_contains=ET_CONTAINS, pkg_base=c.pkg_base)


# ── hand-computed cases ─────────────────────────────────────────────────────

WINDOWS = [
    (FIXED, 1, 5, 3, 0),        # w0
    (FIXED, 1, 9, 2, 1),        # w1: KEV
    (0, 0, 0, 4, 0),            # w2: no fix
    (0, 7, 7, 1, 0),            # w3: no fix; its key words are not a fixed key
    (FIXED, 1, TOP + 1, 1, 0),  # w4: same hi as w0 and w1, the largest lo unsigned
]


def three_items() -> RemedCase:
    """Six packages, three items.

    a0{s0}; a1{s0,s1}; a2{s2}; a3{s2}; no agent uses s3.
    creds: s0{c0}; s1{c0,c1}; s2{c2}.  tools: s0{t0}; s1{t0,t1}; s2{t2,t3}; s3{t3}.
    item 0 = p0 (in s0), p1 (in s1), windows w0 w1 w4: fixed keys that differ
      in lo only.  Servers {s0,s1}, agents {a0,a1}, creds {c0,c1}, tools {t0,t1}.
    item 1 = p2 (in s0, the CONTAINS edge twice), p5 (in no server), windows
      w2 w3: all unfixed.  Shares s0 with item 0.  Servers {s0}.
    item 2 = p3 (in s2), p4 (in s2 and s3), windows w1 w2: two installs on one
      server; s3 has no agents.  Servers {s2,s3}, tools {t2,t3}.
    """
    findings = []
    for p, wins, scores in (
            (0, (0, 1, 4), (0.5, 0.25, 0.75)), (1, (0, 1, 4), (0.5, 0.25, 0.625)),
            (2, (2, 3), (0.75, 0.125)), (3, (1, 2), (0.25, 0.875)), (4, (1, 2), (0.5, 0.5)),
            (5, (2, 3), (0.25, 0.25))):
        findings += [(p, w, s) for w, s in zip(wins, scores)]
    return RemedCase(
        "three_items", n_agents=4, n_servers=4, n_creds=3, n_tools=4, n_pkgs=6,
        uses=[(0, 0), (1, 0), (1, 1), (2, 2), (3, 2)],
        has_cred=[(0, 0), (1, 0), (1, 1), (2, 2)],
        provides=[(0, 0), (1, 0), (1, 1), (2, 2), (2, 3), (3, 3)],
        contains=[(0, 0), (1, 1), (0, 2), (0, 2), (2, 3), (2, 4), (3, 4)],
        item_of=[0, 0, 1, 2, 2, 1], windows=WINDOWS, findings=findings,
        expected={
            "item": [0, 1, 2], "rep_pkg": [0, 2, 3], "installs": [2, 2, 2],
            "n_findings": [6, 4, 4], "n_vulns": [3, 2, 2],
            "max_score": [0.75, 0.75, 0.875], "worst_sev": [3, 4, 4], "kev": [1, 0, 1],
            "fix_hi": [1, 0, 1], "fix_lo": [TOP + 1, 0, 9], "n_unfixed": [0, 2, 1],
            "n_servers": [2, 1, 2], "n_agents": [2, 2, 2], "n_creds": [2, 1, 1],
            "n_tools": [2, 1, 2], "agents_pct": [50.0, 50.0, 50.0]},
        # item 2 by score; items 0 and 1 tie on score and agents: item index
        expected_order=[2, 0, 1])


def order_ties() -> RemedCase:
    """Four one-package items.  s0{a0,a1,a2}; s1{a0}; s2{a0}; s3{a0,a1}.
    Scores 0.5, 0.5, 0.5, 0.75: item 3 first, then item 0 (three agents), then
    items 1 and 2 (one agent each) by index."""
    return RemedCase(
        "order_ties", n_agents=3, n_servers=4, n_creds=1, n_tools=1, n_pkgs=4,
        uses=[(0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (0, 3), (1, 3)],
        has_cred=[(0, 0)], provides=[(1, 0)],
        contains=[(0, 0), (1, 1), (2, 2), (3, 3)],
        item_of=[0, 1, 2, 3], windows=WINDOWS,
        findings=[(0, 0, 0.5), (1, 0, 0.5), (2, 0, 0.5), (3, 0, 0.75)],
        expected={"item": [0, 1, 2, 3], "n_agents": [3, 1, 1, 2], "n_servers": [1, 1, 1, 1],
                  "n_creds": [1, 0, 0, 0], "n_tools": [0, 1, 0, 0]},
        expected_order=[3, 0, 1, 2])


def empty_findings() -> RemedCase:
    c = three_items()
    c.name, c.findings, c.expected, c.expected_order = "empty_findings", [], {}, []
    return c


HAND_CASES = (three_items, order_ties, empty_findings)


# ── generated cases (checked against the oracle) ────────────────────────────


def spread(name: str, n_findings: int, n_items: int = 5, n_servers: int = 7,
           per_pkg: int = 1, matched_items=None) -> RemedCase:
    """``n_findings`` findings, ``per_pkg`` per package on windows
    0..per_pkg-1: package p is item ``p % n_items`` (or cycles through
    ``matched_items``) and sits in servers p % n_servers and
    (3p + 1) % n_servers.  One more package, of the last item, is unmatched."""
    assert n_findings % per_pkg == 0 and per_pkg <= len(WINDOWS)
    n_pkgs = n_findings // per_pkg
    pick = matched_items or list(range(n_items))
    item_of = [pick[p % len(pick)] for p in range(n_pkgs)] + [n_items - 1]
    findings = [(p, w, ((p * 7 + w * 3) % 16) / 16.0)
                for p in range(n_pkgs) for w in range(per_pkg)]
    return RemedCase(
        name, n_agents=6, n_servers=n_servers, n_creds=5, n_tools=9, n_pkgs=n_pkgs + 1,
        uses=[(a, s) for s in range(n_servers) for a in range(6) if (a + s) % 3 == 0],
        has_cred=[(s, c) for s in range(n_servers) for c in range(5) if (s * c) % 4 == 1],
        provides=[(s, t) for s in range(n_servers) for t in range(9) if (s + 2 * t) % 5 == 0],
        contains=[(p % n_servers, p) for p in range(n_pkgs)]
        + [((3 * p + 1) % n_servers, p) for p in range(n_pkgs)],
        item_of=item_of, windows=WINDOWS, findings=findings)


def one_item_two_waves() -> RemedCase:
    """128 findings, all of one item: 64 packages with two windows each."""
    return spread("one_item_two_waves", 128, n_items=1, per_pkg=2)


def first_and_last_item() -> RemedCase:
    """Ten items; only item 0 and item 9 are matched."""
    return spread("first_and_last_item", 12, n_items=10, matched_items=[0, 9])


def wide_union(which: str, size: int) -> RemedCase:
    """One item whose set ``which`` (servers, agents, creds, tools) has exactly
    ``size`` members, beside a small second item.

    servers: ``size`` installs, one per server of its own.  The others: two
    installs on two servers whose segments overlap in six members and cover
    ``size`` together."""
    n = {"servers": 3, "agents": 2, "creds": 2, "tools": 2}
    n[which] = size
    if which == "servers":
        hold = size
        pairs = []
    else:
        hold = 2
        half = size // 2
        pairs = [(0, x) for x in range(half + 3)] + [(1, x) for x in range(half - 3, size)]
    n_servers = max(n["servers"], hold) + 1
    small = n_servers - 1   # the server of the second item
    uses = [(0, small)] + ([(x, s) for s, x in pairs] if which == "agents" else [(1, 0)])
    has_cred = [(small, 0)] + (pairs if which == "creds" else [(0, 1)])
    provides = [(small, 1)] + (pairs if which == "tools" else [(0, 0)])
    findings = [(p, 0, 0.5) for p in range(hold)] + [(hold, 2, 0.25)]
    return RemedCase(
        f"wide_{which}_{size}", n_agents=n["agents"], n_servers=n_servers, n_creds=n["creds"],
        n_tools=n["tools"], n_pkgs=hold + 1, uses=uses, has_cred=has_cred, provides=provides,
        contains=[(p, p) for p in range(hold)] + [(small, hold)],
        item_of=[0] * hold + [1], windows=WINDOWS, findings=findings)


def many_wide(n_wide: int, size: int) -> RemedCase:
    """``n_wide`` items of ``size`` installs each, every install on a server
    of its own; the servers of neighbouring items overlap by half, and server
    s has agent s % 5, cred s % 3 and tools s % 7, s % 11."""
    n_pkgs = n_wide * size
    n_servers = (n_wide + 1) * size // 2 + 1
    contains = [((p // size) * (size // 2) + p % size, p) for p in range(n_pkgs)]
    return RemedCase(
        f"many_wide_{n_wide}x{size}", n_agents=5, n_servers=n_servers, n_creds=3, n_tools=11,
        n_pkgs=n_pkgs, uses=[(s % 5, s) for s in range(n_servers)],
        has_cred=[(s, s % 3) for s in range(n_servers)],
        provides=[(s, s % 7) for s in range(n_servers)] + [(s, s % 11) for s in range(n_servers)],
        contains=contains, item_of=[p // size for p in range(n_pkgs)], windows=WINDOWS,
        findings=[(p, 1, 0.5) for p in range(n_pkgs)])


def many_installs(n_installs: int, servers_each: int, n_servers: int) -> RemedCase:
    """One item of ``n_installs`` installs, install p in ``servers_each``
    servers starting at p * servers_each (mod n_servers)."""
    contains = [((p * servers_each + k) % n_servers, p)
                for p in range(n_installs) for k in range(servers_each)]
    return RemedCase(
        f"many_installs_{n_installs}x{servers_each}", n_agents=7, n_servers=n_servers,
        n_creds=4, n_tools=6, n_pkgs=n_installs,
        uses=[(s % 7, s) for s in range(n_servers)],
        has_cred=[(s, s % 4) for s in range(0, n_servers, 2)],
        provides=[(s, s % 6) for s in range(n_servers)],
        contains=contains, item_of=[0] * n_installs, windows=WINDOWS,
        findings=[(p, 0, 0.5) for p in range(n_installs)])


# a few thousand findings on 78 matched items of up to 47 installs each
ESTATE_ARGS = dict(n_agents=40, n_servers=150, n_packages=4000, name_catalog=300,
                   arena_windows=6000, seed=11)
