"""Hand-built inputs for the toxic combinations (``cpu_ref.toxic_combinations``,
``native.toxic_combinations``): a few agents, servers, tools and packages
given as edge lists, laid out like an estate (agents first, then servers,
tools, packages), a handful of advisory windows and a list of findings with
the step's ``n_creds`` and ``n_tools`` written next to them.  The hand cases
carry their expected values, worked out on paper from the definitions.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from remediation_cases import csr

from agentbom_amd.graph.gpu_engine import _DB_TOOL, _FULL_TOOL, _impact_lut
from agentbom_amd.ops import cpu_ref
from agentbom_amd.scan.synth import ET_CONTAINS, ET_PROVIDES_TOOL, ET_USES

EXEC, WRITE, DELETE = cpu_ref.TC_EXEC, cpu_ref.TC_WRITE, cpu_ref.TC_DELETE
READ, RETRIEVAL = cpu_ref.TC_READ, cpu_ref.TC_RETRIEVAL

TOOL_LUT = _impact_lut(_FULL_TOOL, _DB_TOOL)
FULL = min(_FULL_TOOL)                          # an impact code of class 2
DB = min(_DB_TOOL)                              # class 1: db tools only
NONE = int(np.flatnonzero(TOOL_LUT == 0)[0])    # class 0: no tools

f32 = np.float32


@dataclass
class ToxicCase:
    name: str
    n_agents: int
    n_servers: int
    n_tools: int
    n_pkgs: int
    uses: list        # (agent, server), local indices
    provides: list    # (server, tool)
    contains: list    # (server, package)
    tool_caps: list   # per tool
    tool_is_db: list  # per tool
    windows: list     # (severity, kev, impact code)
    findings: list    # (package, window, score, n_creds, n_tools), packages ascending
    vuln_of: list | None = None
    expected: dict = field(default_factory=dict)

    @property
    def server_base(self) -> int:
        return self.n_agents

    @property
    def tool_base(self) -> int:
        return self.server_base + self.n_servers

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
        for s, t in self.provides:
            src.append(s + self.server_base), dst.append(t + self.tool_base)
            et.append(ET_PROVIDES_TOOL)
        for s, p in self.contains:
            src.append(s + self.server_base), dst.append(p + self.pkg_base), et.append(ET_CONTAINS)
        return (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64),
                np.asarray(et, dtype=np.uint8))

    def finding_arrays(self):
        """(pkg_idx i64, win_idx i64, scores f32, n_creds i32, n_tools i32)"""
        f = self.findings
        return (np.asarray([x[0] for x in f], dtype=np.int64),
                np.asarray([x[1] for x in f], dtype=np.int64),
                np.asarray([x[2] for x in f], dtype=np.float32),
                np.asarray([x[3] for x in f], dtype=np.int32),
                np.asarray([x[4] for x in f], dtype=np.int32))

    def window_arrays(self):
        """(severity u8, kev u8, impact u8)"""
        return tuple(np.asarray([x[k] for x in self.windows], dtype=np.uint8) for k in range(3))

    def vuln_map(self):
        return None if self.vuln_of is None else np.asarray(self.vuln_of, dtype=np.int32)


def oracle(c: ToxicCase, vuln_of="case") -> dict:
    """``cpu_ref.toxic_combinations`` on the case (``vuln_of``: another map)."""
    src, dst, et = c.edges()
    pkg_idx, win_idx, scores, n_creds, n_tools = c.finding_arrays()
    sev, kev, impact = c.window_arrays()
    return cpu_ref.toxic_combinations(
        pkg_idx, win_idx, scores, n_creds, n_tools,
        *csr(dst, src, et, c.num_nodes), *csr(src, dst, et, c.num_nodes),
        ET_CONTAINS, ET_USES, ET_PROVIDES_TOOL, c.pkg_base, sev, kev, impact, TOOL_LUT,
        c.tool_base, np.asarray(c.tool_is_db, dtype=np.uint8),
        np.asarray(c.tool_caps, dtype=np.uint8),
        c.vuln_map() if isinstance(vuln_of, str) else vuln_of)


def device_inputs(c: ToxicCase, device: str = "cuda") -> dict:
    """Keyword arguments of ``native.toxic_combinations`` (less workspace and
    pool size): the reach index built by the engine's own builder, the server
    table by ``native.toxic_server_table``."""
    import torch

    from agentbom_amd.graph.gpu_engine import build_reach_index
    from agentbom_amd.ops import native

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    src, dst, et = c.edges()
    off, col, etype = csr(dst, src, et, c.num_nodes)
    flag = torch.zeros(c.num_nodes, dtype=torch.uint8, device=device)
    index = build_reach_index(torch, dev(src), dev(dst), dev(et), c.server_base, c.n_servers,
                              flag, flag)
    table = native.toxic_server_table(
        index, dev(np.asarray(c.tool_caps, dtype=np.uint8)),
        dev(np.asarray(c.tool_is_db, dtype=np.uint8)), c.tool_base)
    pkg_idx, win_idx, scores, n_creds, _n_tools = c.finding_arrays()
    sev, kev, impact = c.window_arrays()
    vmap = c.vuln_map()
    return dict(
        pkg_idx=dev(pkg_idx), win_idx=dev(win_idx), scores=dev(scores), n_creds=dev(n_creds),
        arena={"severity": dev(sev), "kev": dev(kev), "impact": dev(impact)},
        tool_lut=dev(TOOL_LUT), table=table,
        rev={"row_off": dev(off), "col": dev(col), "etype": dev(etype)},
        index=index, et_contains=ET_CONTAINS, pkg_base=c.pkg_base,
        vuln_of=None if vmap is None else dev(vmap),
        n_vulns=None if vmap is None else int(vmap.max()) + 1)


# ── engine level ────────────────────────────────────────────────────────────


def engine_reference(eng, res, caps, vuln_of):
    """The oracle on an engine's host tensors and a step result on the host."""
    est = eng.estate
    return cpu_ref.toxic_combinations(
        res["pkg_idx"].numpy(), res["win_idx"].numpy(), res["scores"].numpy(),
        res["n_creds"].numpy(), res["n_tools"].numpy(),
        eng.rev["row_off"].numpy(), eng.rev["col"].numpy(), eng.rev["etype"].numpy(),
        eng.fwd["row_off"].numpy(), eng.fwd["col"].numpy(), eng.fwd["etype"].numpy(),
        ET_CONTAINS, ET_USES, ET_PROVIDES_TOOL, est.pkg_base,
        eng.arena["severity"].numpy(), eng.arena["kev"].numpy(), eng.arena["impact"].numpy(),
        eng.tool_lut.numpy(), est.tool_base, est.tool_is_db, caps, vuln_of)


def assert_engine_equals_oracle(got, ref, k=None):
    """Every key of an ``EstateEngine.toxic_combinations`` result against the
    oracle's: exact, fp32 as bit patterns."""
    import torch

    def same(g, w, key):
        g, w = g.cpu(), torch.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == w.dtype and g.shape == w.shape, key
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), key

    flagged = np.flatnonzero(ref["patterns"])
    order = flagged[np.argsort(-ref["combo_score"][flagged], kind="stable")]
    v_order = ref["vulns"]["order"]
    if k is not None:
        order, v_order = order[:k], v_order[:k]
    same(got["patterns"], ref["patterns"], "patterns")
    same(got["combo_score"], ref["combo_score"], "combo_score")
    same(got["order"], order.astype(np.int64), "order")
    for key in cpu_ref.TOXIC_VULN_KEYS:
        same(got["vulns"][key], ref["vulns"][key][v_order], "vulns." + key)
    same(got["poison_servers"], ref["poison_servers"], "poison_servers")
    same(got["n_by_pattern"], ref["n_by_pattern"], "n_by_pattern")
    assert got["n_vulns"] == len(ref["vulns"]["vuln"])
    assert got["n_multi_agent"] == ref["n_multi_agent"]


# ── hand-computed cases ─────────────────────────────────────────────────────


def rules() -> ToxicCase:
    """Eleven findings, one rule at a time.

    a0{s0,s4}; a1{s1, the USES edge twice}; a2{s1}; a3{s2}; no agent uses s3.
    So s1 is the one shared server (a1, a2).
    t0 exec; t1 exec, a db tool; t2 retrieval; t3 read.
    s0{t0}; s1{t1,t2}; s2{t3}; s3 no tools; s4{t0}.
    p0 in s0 (the CONTAINS edge twice); p1 in s1; p2 in s2; p3 in no server;
    p4 in s3; p5 in s4 and s0.
    w0 high; w1 medium; w2 medium KEV; w3 critical, db tools only; w4
    critical, no tools; w5 high.

    f0  p0 w0 score 4, creds: high + creds -> CRED; t0 exec -> EXEC.  4 * 1.5 = 6.
    f1  p0 w1: medium, nothing.
    f2  p0 w2 score 0, creds: KEV + creds -> KEV at medium, CRED not.  10.
    f3  p0 w3 score 8, no creds: db class and t0 is no db tool -> no EXEC.
    f4  p1 w0 score 0, no creds: t1 exec, t2 retrieval, s1 shared -> EXEC,
        CACHE, LATERAL; score 0 takes the defaults, the largest is 9.5.
    f5  p1 w3 score 7, creds: CRED; db class: t1 -> EXEC, t2 is no db tool ->
        no CACHE; LATERAL.  7 * 1.5 = 10.5 -> 10.
    f6  p1 w4 score 2: no tools at class 0; LATERAL alone, 2 * 1.4.
    f7  p2 w1: medium, nothing.
    f8  p3 w0: no server, nothing of its own.
    f9  p4 w0: s3 has no tools and no agents, nothing of its own.
    f10 p5 w5 score 1: s4 and s0 have one agent each (the same) -> no LATERAL;
        t0 -> EXEC, 1 * 1.3.

    Advisories: w0 = {f0,f4,f8,f9}, packages p0 p1 p3 p4, servers s0 s1 s3,
    agents a0 a1 a2 -> multi-agent, on all four, largest score 4 -> 4.8.
    w1 = {f1,f7}: s0, s2 -> a0, a3: two agents, not multi.  w3 = {f3,f5}: s0,
    s1 -> three agents -> multi, largest score 8 -> 9.6.  w2, w4, w5 single.
    """
    hi_multi, crit_multi = f32(4.0) * f32(1.2), f32(8.0) * f32(1.2)
    return ToxicCase(
        "rules", n_agents=4, n_servers=5, n_tools=4, n_pkgs=6,
        uses=[(0, 0), (1, 1), (2, 1), (1, 1), (3, 2), (0, 4)],
        provides=[(0, 0), (1, 1), (1, 2), (2, 3), (4, 0)],
        contains=[(0, 0), (0, 0), (1, 1), (2, 2), (3, 4), (4, 5), (0, 5)],
        tool_caps=[EXEC, EXEC, RETRIEVAL, READ], tool_is_db=[0, 1, 0, 0],
        windows=[(4, 0, FULL), (3, 0, FULL), (3, 1, FULL), (5, 0, DB), (5, 0, NONE),
                 (4, 0, FULL)],
        findings=[(0, 0, 4.0, 1, 1), (0, 1, 4.0, 1, 1), (0, 2, 0.0, 2, 1), (0, 3, 8.0, 0, 0),
                  (1, 0, 0.0, 0, 2), (1, 3, 7.0, 1, 1), (1, 4, 2.0, 0, 0), (2, 1, 1.0, 1, 1),
                  (3, 0, 3.0, 0, 0), (4, 0, 3.0, 0, 0), (5, 5, 1.0, 0, 1)],
        expected={
            "patterns": [1 | 4 | 32, 0, 2, 32, 4 | 8 | 16 | 32, 1 | 4 | 16 | 32, 16, 0, 32, 32, 4],
            "combo_score": [f32(6.0), f32(0.0), f32(10.0), crit_multi, f32(9.5), f32(10.0),
                            f32(2.0) * f32(1.4), f32(0.0), hi_multi, hi_multi, f32(1.3)],
            "vulns": {
                "vuln": [0, 1, 2, 3, 4, 5], "n_findings": [4, 2, 1, 2, 1, 1],
                "n_packages": [4, 2, 1, 2, 1, 1], "n_servers": [3, 2, 1, 2, 1, 2],
                "n_agents": [3, 2, 1, 3, 2, 1], "max_score": [4.0, 4.0, 0.0, 8.0, 2.0, 1.0],
                "worst_sev": [4, 3, 3, 5, 5, 4], "kev": [0, 0, 1, 0, 0, 0],
                "patterns": [61, 0, 2, 53, 16, 4],
                # w3 by score; w0 and w1 tie at 4: three agents before two
                "order": [3, 0, 1, 4, 5, 2]},
            "poison_servers": [], "n_by_pattern": [2, 1, 4, 1, 3, 6], "n_multi_agent": 2})


def two_windows_one_advisory() -> ToxicCase:
    """s0 used by a0, a1, a2; p0 and p1 in s0; windows w0 and w1 are advisory
    0, w2 is advisory 1.  p0 matches w0 and w1: advisory 0 has two findings on
    ONE package.  Both advisories reach three agents with all scores 0: the
    multi-agent default, 7.5."""
    return ToxicCase(
        "two_windows_one_advisory", n_agents=3, n_servers=1, n_tools=1, n_pkgs=2,
        uses=[(0, 0), (1, 0), (2, 0)], provides=[], contains=[(0, 0), (0, 1)],
        tool_caps=[0], tool_is_db=[0],
        windows=[(2, 0, FULL), (2, 0, FULL), (1, 0, FULL)],
        findings=[(0, 0, 0.0, 0, 0), (0, 1, 0.0, 0, 0), (1, 2, 0.0, 0, 0)],
        vuln_of=[0, 0, 1],
        expected={
            "patterns": [32, 32, 32], "combo_score": [f32(7.5)] * 3,
            "vulns": {"vuln": [0, 1], "n_findings": [2, 1], "n_packages": [1, 1],
                      "n_servers": [1, 1], "n_agents": [3, 3], "max_score": [0.0, 0.0],
                      "worst_sev": [2, 1], "kev": [0, 0], "patterns": [32, 32],
                      "order": [0, 1]},
            "poison_servers": [], "n_by_pattern": [0, 0, 0, 0, 0, 3], "n_multi_agent": 2})


def poison() -> ToxicCase:
    """No findings.  t0 write, t1 read, t2 retrieval.  s0: a0 a1, write + read
    -> poison.  s1: a0 a1, write only -> not.  s2: a2 alone, write + read ->
    not.  s3: a1 a2, write + retrieval -> poison.  Servers start at node 3."""
    return ToxicCase(
        "poison", n_agents=3, n_servers=4, n_tools=3, n_pkgs=1,
        uses=[(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (1, 3), (2, 3)],
        provides=[(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (3, 0), (3, 2)],
        contains=[(0, 0)], tool_caps=[WRITE, READ, RETRIEVAL], tool_is_db=[0, 0, 0],
        windows=[(5, 1, FULL)], findings=[],
        expected={
            "patterns": [], "combo_score": [],
            "vulns": {key: [] for key in cpu_ref.TOXIC_VULN_KEYS + ("order",)},
            "poison_servers": [3, 6], "n_by_pattern": [0] * 6, "n_multi_agent": 0})


HAND_CASES = (rules, two_windows_one_advisory, poison)


# ── generated cases (checked against the oracle) ────────────────────────────


def with_counts(c: ToxicCase) -> ToxicCase:
    """The case with every finding's ``n_tools`` set to what the step's filter
    gives: the distinct tools (db tools at class 1, none at class 0) of the
    package's servers.  ``n_creds`` stays as written."""
    tools_of: dict = {}
    for s, t in c.provides:
        tools_of.setdefault(s, set()).add(t)
    servers_of: dict = {}
    for s, p in c.contains:
        servers_of.setdefault(p, set()).add(s)
    out = []
    for p, w, score, n_creds, _ in c.findings:
        cls = int(TOOL_LUT[c.windows[w][2]])
        tools = set().union(*(tools_of.get(s, set()) for s in servers_of.get(p, ())))
        if cls == 1:
            tools = {t for t in tools if c.tool_is_db[t]}
        out.append((p, w, score, n_creds, len(tools) if cls else 0))
    c.findings = out
    return c


WINDOWS = [(4, 0, FULL), (3, 1, FULL), (5, 0, DB), (5, 1, NONE), (2, 0, FULL), (4, 1, DB),
           (1, 0, FULL)]
TOOL_CAPS = [EXEC, WRITE | READ, RETRIEVAL, READ, DELETE, 0, WRITE, EXEC | RETRIEVAL, READ]
TOOL_IS_DB = [0, 1, 0, 1, 0, 0, 1, 1, 0]


def runs(name: str, run_lengths, n_servers: int = 7, vuln_of=None) -> ToxicCase:
    """Package p has ``run_lengths[p]`` findings, on windows (3p + j) % 7, and
    sits in servers p % n_servers and (3p + 1) % n_servers; every fifth
    package sits in none.  Scores and n_creds cycle, with zeros among them."""
    findings = [(p, (3 * p + j) % len(WINDOWS), ((p * 7 + j * 3) % 16) / 2.0, (p + j) % 3, 0)
                for p, n in enumerate(run_lengths) for j in range(n)]
    n_pkgs = len(run_lengths)
    return with_counts(ToxicCase(
        name, n_agents=6, n_servers=n_servers, n_tools=len(TOOL_CAPS), n_pkgs=n_pkgs + 1,
        uses=[(a, s) for s in range(n_servers) for a in range(6) if (a + 2 * s) % 5 == 0],
        provides=[(s, t) for s in range(n_servers) for t in range(len(TOOL_CAPS))
                  if (s + 2 * t) % 5 == 0],
        contains=[(p % n_servers, p) for p in range(n_pkgs) if p % 5 != 4]
        + [((3 * p + 1) % n_servers, p) for p in range(n_pkgs) if p % 5 != 4],
        tool_caps=TOOL_CAPS, tool_is_db=TOOL_IS_DB, windows=WINDOWS, findings=findings,
        vuln_of=vuln_of))


def spread(n_findings: int) -> ToxicCase:
    return runs(f"spread_{n_findings}", [1] * n_findings)


def run_at_lane_62() -> ToxicCase:
    """62 packages with one finding each, then a package with four: its run
    takes lanes 62 and 63 of the first wave and 0 and 1 of the second; the
    windows of the run map to two advisories, two findings each."""
    return runs("run_at_lane_62", [1] * 62 + [4, 1, 1], vuln_of=[1, 1, 0, 1, 2, 1, 2])


def one_advisory_two_waves() -> ToxicCase:
    """128 packages with one finding each, all on window 0, 30 servers."""
    c = runs("one_advisory_two_waves", [1] * 128, n_servers=30)
    c.findings = [(p, 0, score, n_creds, n_tools) for p, _w, score, n_creds, n_tools in c.findings]
    return with_counts(c)


def wide_union(which: str, size: int) -> ToxicCase:
    """Advisory 0 with exactly ``size`` distinct servers (``size`` packages,
    one per server of its own, each server used by agent s % 5) or agents (two
    packages on two servers whose agents overlap in six and cover ``size``),
    beside a small second advisory."""
    if which == "servers":
        hold, n_agents = size, 5
        uses = [(s % 5, s) for s in range(size)]
    else:
        hold, n_agents, half = 2, size, size // 2
        uses = [(x, 0) for x in range(half + 3)] + [(x, 1) for x in range(half - 3, size)]
    small = hold  # the server and the package of the second advisory
    return with_counts(ToxicCase(
        f"wide_{which}_{size}", n_agents=n_agents, n_servers=hold + 1, n_tools=2, n_pkgs=hold + 1,
        uses=uses + [(0, small)], provides=[(0, 0), (small, 1)],
        contains=[(p, p) for p in range(hold)] + [(small, hold)],
        tool_caps=[EXEC, RETRIEVAL], tool_is_db=[0, 1],
        windows=WINDOWS,
        findings=[(p, 0, 2.5, 1, 0) for p in range(hold)] + [(hold, 2, 0.5, 0, 0)]))


def many_packages(n_pkgs: int, n_servers: int) -> ToxicCase:
    """One advisory of ``n_pkgs`` packages on ``n_servers`` servers."""
    return with_counts(ToxicCase(
        f"many_packages_{n_pkgs}", n_agents=7, n_servers=n_servers, n_tools=2, n_pkgs=n_pkgs,
        uses=[(s % 7, s) for s in range(n_servers)], provides=[(0, 0), (1, 1)],
        contains=[(p % n_servers, p) for p in range(n_pkgs)],
        tool_caps=[WRITE, READ], tool_is_db=[0, 0], windows=WINDOWS,
        findings=[(p, 0, 0.5, 0, 0) for p in range(n_pkgs)]))


def full_server_list() -> ToxicCase:
    """One advisory of 256 packages, one chunk of the block tier, package p
    alone on servers 5p .. 5p + 4: 1280 distinct servers, more than the 1024
    a block lists per chunk, so the threads that find the list full visit
    their servers' rows alone.  Server s is used by agent s % 320 and, every
    fourth one, by agent (s // 4 + 1) % 320 as well: 320 distinct agents, each
    on four servers or more."""
    n_pkgs, per, n_agents = 256, 5, 320
    n_servers = n_pkgs * per
    return with_counts(ToxicCase(
        "full_server_list", n_agents=n_agents, n_servers=n_servers, n_tools=1, n_pkgs=n_pkgs,
        uses=[(s % n_agents, s) for s in range(n_servers)]
        + [((s // 4 + 1) % n_agents, s) for s in range(0, n_servers, 4)],
        provides=[(0, 0)], contains=[(per * p + k, p) for p in range(n_pkgs) for k in range(per)],
        tool_caps=[EXEC], tool_is_db=[0], windows=WINDOWS,
        findings=[(p, 0, 1.0 + p % 4, p % 2, 0) for p in range(n_pkgs)]))


def many_wide(n_wide: int, size: int) -> ToxicCase:
    """``n_wide`` advisories of ``size`` packages each, every package on a
    server of its own; the servers of neighbouring advisories overlap by half."""
    n_pkgs = n_wide * size
    n_servers = (n_wide + 1) * size // 2 + 1
    return with_counts(ToxicCase(
        f"many_wide_{n_wide}x{size}", n_agents=5, n_servers=n_servers, n_tools=1, n_pkgs=n_pkgs,
        uses=[(s % 5, s) for s in range(n_servers)], provides=[(0, 0)],
        contains=[((p // size) * (size // 2) + p % size, p) for p in range(n_pkgs)],
        tool_caps=[EXEC], tool_is_db=[0], windows=WINDOWS,
        findings=[(p, p // size, 1.0, 1, 0) for p in range(n_pkgs)]))
