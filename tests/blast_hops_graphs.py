"""Hand-built graphs for the multi-hop delegation expansion (blast_hops).

Each graph is a few agents, servers, credentials and packages given as edge
lists, laid out like an estate (agent ids first, then servers, credentials,
packages), with the expected outputs written by hand.  The builders return
the CSR arrays ``cpu_ref.blast_hops`` takes, the device inputs
``native.blast_hops`` takes, and ``Agent`` / ``MCPServer`` / ``BlastRadius``
objects for ``models.blast.expand_blast_radius_hops``; no arena is involved.

The agent sets A_h for h <= D do not depend on D, so one row of level sizes
per package, cut at D, is the expected ``hop_agents`` at every depth; the
credential count is written per depth.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from agentbom_amd.ops import native
from agentbom_amd.scan.synth import ET_CONTAINS, ET_HAS_CRED, ET_USES

DEPTHS = (1, 2, 3, 4, 5)


@dataclass
class HopGraph:
    name: str
    n_agents: int
    n_servers: int
    n_creds: int
    n_pkgs: int
    uses: list            # (agent, server), local indices
    has_cred: list        # (server, cred)
    contains: list        # (server, package)
    # per package: |A_2|..|A_5| at depth 5, and t_creds at depth 1..5
    levels: list = field(default_factory=list)
    creds_by_depth: list = field(default_factory=list)

    @property
    def server_base(self) -> int:
        return self.n_agents

    @property
    def cred_base(self) -> int:
        return self.n_agents + self.n_servers

    @property
    def pkg_base(self) -> int:
        return self.cred_base + self.n_creds

    @property
    def num_nodes(self) -> int:
        return self.pkg_base + self.n_pkgs

    @property
    def pkgs(self) -> np.ndarray:
        return np.arange(self.n_pkgs, dtype=np.int64) + self.pkg_base

    def edges(self):
        """(src, dst, etype) in global node ids."""
        src, dst, et = [], [], []
        for a, s in self.uses:
            src.append(a), dst.append(s + self.server_base), et.append(ET_USES)
        for s, c in self.has_cred:
            src.append(s + self.server_base), dst.append(c + self.cred_base), et.append(ET_HAS_CRED)
        for s, p in self.contains:
            src.append(s + self.server_base), dst.append(p + self.pkg_base), et.append(ET_CONTAINS)
        return (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64),
                np.asarray(et, dtype=np.uint8))

    def expected(self, depth: int):
        """(hop_agents int32 [U,4], t_creds int32 [U], hop_depth uint8 [U])."""
        d = max(1, min(depth, 5))
        hop = np.asarray(self.levels, dtype=np.int32).reshape(self.n_pkgs, 4).copy()
        hop[:, max(d - 1, 0):] = 0
        creds = np.asarray([row[d - 1] for row in self.creds_by_depth], dtype=np.int32)
        hop_depth = (1 + (hop > 0).sum(axis=1)).astype(np.uint8)
        return hop, creds, hop_depth


def csr(src, dst, et, num_nodes: int):
    """(row_off int64 [N+1], col int32 [E], etype uint8 [E]), rows by ``src``."""
    order = np.argsort(src, kind="stable")
    row_off = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=num_nodes), out=row_off[1:])
    return row_off, dst[order].astype(np.int32), et[order]


def cpu_args(g: HopGraph, depth: int) -> tuple:
    """Positional arguments of ``cpu_ref.blast_hops`` for graph ``g``."""
    src, dst, et = g.edges()
    fwd = csr(src, dst, et, g.num_nodes)
    rev = csr(dst, src, et, g.num_nodes)
    return (g.pkgs, *rev, ET_CONTAINS, ET_USES, ET_HAS_CRED, *fwd, depth)


def device_inputs(g: HopGraph, device: str = "cuda") -> dict:
    """pkgs32, rev CSR, reach index and agent index on ``device``, built by
    the engine's own index builders."""
    import torch

    from agentbom_amd.graph.gpu_engine import build_agent_index, build_reach_index

    src, dst, et = (torch.from_numpy(x).to(device) for x in g.edges())
    off, col, etype = csr(*(x.cpu().numpy() for x in (dst, src, et)), g.num_nodes)
    rev = {"row_off": torch.from_numpy(off).to(device),
           "col": torch.from_numpy(col).to(device),
           "etype": torch.from_numpy(etype).to(device)}
    flag = torch.zeros(g.num_nodes, dtype=torch.uint8, device=device)
    index = build_reach_index(torch, src, dst, et, g.server_base, g.n_servers, flag, flag)
    agent_index = build_agent_index(torch, src, dst, et, g.n_agents, index)
    return {"pkgs32": torch.from_numpy(g.pkgs.astype(np.int32)).to(device), "rev": rev,
            "index": index, "agent_index": agent_index}


def model_objects(src, dst, et, n_agents: int, pkgs):
    """(agents, blast radii) for ``expand_blast_radius_hops``: one ``Agent``
    per agent id with its servers in edge order, one ``BlastRadius`` per
    package of ``pkgs`` with its holders and their agents as the direct sets.
    Credential c becomes the env key ``C<c>_TOKEN`` of its servers."""
    from agentbom_amd.models import (
        Agent, AgentType, BlastRadius, MCPServer, Package, Severity, Vulnerability,
    )

    uses = et == ET_USES
    server_ids = sorted(set(dst[uses].tolist()) | set(src[et == ET_CONTAINS].tolist())
                        | set(src[et == ET_HAS_CRED].tolist()))
    env: dict = {s: {} for s in server_ids}
    for s, c in zip(src[et == ET_HAS_CRED].tolist(), dst[et == ET_HAS_CRED].tolist()):
        env[s][f"C{c}_TOKEN"] = "x"
    servers = {s: MCPServer(name=f"s{s}", command="npx", env=env[s]) for s in server_ids}
    agent_servers: dict = {a: [] for a in range(n_agents)}
    for a, s in zip(src[uses].tolist(), dst[uses].tolist()):
        agent_servers[a].append(servers[s])
    agents = [Agent(name=f"a{a}", agent_type=AgentType.CURSOR, config_path=f"/a{a}",
                    mcp_servers=agent_servers[a]) for a in range(n_agents)]
    holders: dict = {int(p): [] for p in pkgs}
    for s, p in zip(src[et == ET_CONTAINS].tolist(), dst[et == ET_CONTAINS].tolist()):
        if p in holders and s not in holders[p]:
            holders[p].append(s)
    radii = []
    for p in pkgs:
        held = holders[int(p)]
        direct = [a for a in agents if any(srv.name in {f"s{s}" for s in held}
                                           for srv in a.mcp_servers)]
        vuln = Vulnerability(id="CVE-2024-0001", summary="test vuln", severity=Severity.HIGH)
        radii.append(BlastRadius(vuln, Package(f"p{int(p)}", "1", "npm"),
                                 [servers[s] for s in held], direct, [], []))
    return agents, radii


def expansion_counts(agents, br, depth: int):
    """(hop_agents [4], t_creds, hop_depth) of ``expand_blast_radius_hops`` on
    one fresh blast radius."""
    from agentbom_amd.models.blast import expand_blast_radius_hops

    expand_blast_radius_hops([br], agents, max_depth=depth)
    hop = [0, 0, 0, 0]
    names = [t["name"] for t in br.transitive_agents]
    assert len(names) == len(set(names))
    for t in br.transitive_agents:
        hop[t["hop"] - 2] += 1
    return hop, len(set(br.transitive_credentials)), br.hop_depth


# ── the graphs ──────────────────────────────────────────────────────────────


def chain() -> HopGraph:
    # p0 in s0; a_i uses s_i and s_{i+1}; c_i on s_i.  One agent per hop:
    # A_h = {a_{h-1}}, cut at D; the servers of a_1..a_{D-1} are s_1..s_D.
    return HopGraph(
        "chain", n_agents=6, n_servers=7, n_creds=7, n_pkgs=1,
        uses=[(i, i) for i in range(6)] + [(i, i + 1) for i in range(6)],
        has_cred=[(i, i) for i in range(7)], contains=[(0, 0)],
        levels=[[1, 1, 1, 1]], creds_by_depth=[[0, 2, 3, 4, 5]])


def diamond() -> HopGraph:
    # a0{s0,s1}; a1{s1,s2}; a2{s1,s2}; a3{s2,s3}.  a2 is reachable at hop 2
    # (through s1) and again at hop 3 (through s2): counted once, at hop 2.
    # c0 on s2, c1 on s3.
    return HopGraph(
        "diamond", n_agents=4, n_servers=4, n_creds=2, n_pkgs=1,
        uses=[(0, 0), (0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (3, 3)],
        has_cred=[(2, 0), (3, 1)], contains=[(0, 0)],
        levels=[[2, 1, 0, 0]], creds_by_depth=[[0, 1, 2, 2, 2]])


def dup_edges() -> HopGraph:
    # a0{s0,s1}; a1{s1,s2}; a2{s2}; c0 on s1 and s2, c1 on s2; every edge twice
    uses = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)]
    has_cred = [(1, 0), (2, 0), (2, 1)]
    return HopGraph(
        "dup_edges", n_agents=3, n_servers=3, n_creds=2, n_pkgs=1,
        uses=uses + uses, has_cred=has_cred + has_cred, contains=[(0, 0), (0, 0)],
        levels=[[1, 1, 0, 0]], creds_by_depth=[[0, 2, 2, 2, 2]])


def loop_back() -> HopGraph:
    # a0{s0,s1}; a1{s0,s1,s2}: the other servers s1, s2 lead back to a0, a1
    return HopGraph(
        "loop_back", n_agents=2, n_servers=3, n_creds=1, n_pkgs=1,
        uses=[(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)],
        has_cred=[(1, 0)], contains=[(0, 0)],
        levels=[[0, 0, 0, 0]], creds_by_depth=[[0, 0, 0, 0, 0]])


def two_holders() -> HopGraph:
    # p0 in s0 and s1; a0{s0,s2}; a1{s1,s2}: from s0 alone a1 would be a hop-2
    # agent, with both holders it is direct.  a2{s2,s3}; a3{s3}.
    # c0 on s1, c1 on s3, c2 on s2.
    return HopGraph(
        "two_holders", n_agents=4, n_servers=4, n_creds=3, n_pkgs=1,
        uses=[(0, 0), (0, 2), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3)],
        has_cred=[(1, 0), (3, 1), (2, 2)], contains=[(0, 0), (1, 0)],
        levels=[[1, 1, 0, 0]], creds_by_depth=[[0, 2, 2, 2, 2]])


def orphans() -> HopGraph:
    # p0 has no holder; p1 is in s0, which no agent uses; p2 is in s1, whose
    # one agent a0 uses nothing else.  a1{s2} is unrelated.
    return HopGraph(
        "orphans", n_agents=2, n_servers=3, n_creds=1, n_pkgs=3,
        uses=[(0, 1), (1, 2)], has_cred=[(2, 0)], contains=[(0, 1), (1, 2)],
        levels=[[0, 0, 0, 0]] * 3, creds_by_depth=[[0, 0, 0, 0, 0]] * 3)


def creds() -> HopGraph:
    # a0{s0,s1}; a1{s1,s2}; a2{s2,s3}; a3{s3,s4}.
    # c0 only on S0 (never counted); c1 on s1 and s2 (shared by the servers of
    # a1 and a2, counted once); c4 on s2, which at D = 2 belongs to the
    # last-level agent a1 and is never enqueued; c2 on s3; c3 on s4.
    return HopGraph(
        "creds", n_agents=4, n_servers=5, n_creds=5, n_pkgs=1,
        uses=[(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4)],
        has_cred=[(0, 0), (1, 1), (2, 1), (2, 4), (3, 2), (4, 3)], contains=[(0, 0)],
        levels=[[1, 1, 1, 0]], creds_by_depth=[[0, 2, 3, 4, 4]])


def fat() -> HopGraph:
    """Three packages; sizes follow the kernel's LDS caps (native.BLAST_HOPS_*).

    p0 in s0: a0 uses s0 and ``wide`` = server cap + 53 further servers, more
    than the visited-server array holds; each of the first 200 of them has one
    agent of its own (A_2 = 200 agents), the first 10 one credential each.
    p1 in t0: e0 uses t0 and t1, and ``crowd`` = agent cap + 8 agents use t1
    alone: a frontier whose agents pass the agent cap.  One credential on t1.
    p2 in u0: h0{u0,u1}, h1{u1}: small, beside the two that overflow."""
    wide = native.BLAST_HOPS_SRV_CAP + 53
    crowd = native.BLAST_HOPS_AG_CAP + 8
    own, with_cred = 200, 10
    # servers: s0, s1..s_wide, t0, t1, u0, u1
    t0 = wide + 1
    t1, u0, u1 = t0 + 1, t0 + 2, t0 + 3
    # agents: a0, b_1..b_own, e0, g_1..g_crowd, h0, h1
    e0 = own + 1
    g0 = e0 + 1
    h0 = g0 + crowd
    uses = [(0, s) for s in range(wide + 1)]
    uses += [(i, i) for i in range(1, own + 1)]
    uses += [(e0, t0), (e0, t1)] + [(g0 + i, t1) for i in range(crowd)]
    uses += [(h0, u0), (h0, u1), (h0 + 1, u1)]
    has_cred = [(s, s - 1) for s in range(1, with_cred + 1)] + [(t1, with_cred)]
    return HopGraph(
        "fat", n_agents=h0 + 2, n_servers=u1 + 1, n_creds=with_cred + 1, n_pkgs=3,
        uses=uses, has_cred=has_cred, contains=[(0, 0), (t0, 1), (u0, 2)],
        levels=[[own, 0, 0, 0], [crowd, 0, 0, 0], [1, 0, 0, 0]],
        creds_by_depth=[[0] + [with_cred] * 4, [0, 1, 1, 1, 1], [0, 0, 0, 0, 0]])


GRAPHS = (chain, diamond, dup_edges, loop_back, two_holders, orphans, creds, fat)

ESTATE_ARGS = dict(n_agents=300, n_servers=1500, n_packages=20000, name_catalog=4000, seed=7)
HOP_KEYS = ("hop_depth", "transitive_agents", "transitive_creds", "transitive_scores")
