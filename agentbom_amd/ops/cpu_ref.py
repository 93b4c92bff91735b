"""CPU (numpy) reference implementations of the engine ops.

These are the numerics oracle for the HIP kernels (tests/test_ops_gpu.py
compares device results bit-for-bit / set-for-set against these) and the
engine used on GPU-less development machines.  Semantics mirror
ops/csrc/{match,bfs,query,score}.hip exactly.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

UNVISITED = np.uint32(0xFFFFFFFF)

# Window flag bits (contract with csrc/abom_common.h and db/arena.py)
WF_HAS_INTRO = 1
WF_HAS_FIXED = 2
WF_HAS_LAST = 4
WF_CPU_FALLBACK = 8
WF_UNFIXED_SUPPRESSED = 16
PF_ENCODABLE = 1


def _key_lt(ahi, alo, bhi, blo):
    return (ahi < bhi) | ((ahi == bhi) & (alo < blo))


def match(pkg_group_key, pkg_key_hi, pkg_key_lo, pkg_flags,
          group_keys, group_off, windows: dict):
    """Vectorized reference of the match kernel.

    Returns (pkg_idx, win_idx) int64 arrays sorted by (pkg, window).
    """
    P = len(pkg_group_key)
    enc = (pkg_flags & PF_ENCODABLE) != 0
    gidx = np.searchsorted(group_keys, pkg_group_key)
    in_range = gidx < len(group_keys)
    gidx_c = np.clip(gidx, 0, max(len(group_keys) - 1, 0))
    hit = enc & in_range & (group_keys[gidx_c] == pkg_group_key) if len(group_keys) else np.zeros(P, bool)

    pkg_out = []
    win_out = []
    wf = windows["flags"]
    ihi, ilo = windows["intro_hi"], windows["intro_lo"]
    fhi, flo = windows["fixed_hi"], windows["fixed_lo"]
    lhi, llo = windows["last_hi"], windows["last_lo"]
    for p in np.nonzero(hit)[0]:
        g = gidx[p]
        khi, klo = pkg_key_hi[p], pkg_key_lo[p]
        for w in range(group_off[g], group_off[g + 1]):
            f = wf[w]
            if f & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED):
                continue
            if (f & WF_HAS_INTRO) and _key_lt(khi, klo, ihi[w], ilo[w]):
                continue
            if (f & WF_HAS_FIXED) and not _key_lt(khi, klo, fhi[w], flo[w]):
                continue
            if (f & WF_HAS_LAST) and _key_lt(lhi[w], llo[w], khi, klo):
                continue
            pkg_out.append(p)
            win_out.append(w)
    pkg_arr = np.asarray(pkg_out, dtype=np.int64)
    win_arr = np.asarray(win_out, dtype=np.int64)
    order = np.lexsort((win_arr, pkg_arr)) if len(pkg_arr) else np.array([], dtype=np.int64)
    return pkg_arr[order], win_arr[order]


def bfs(row_off, col, sources, num_nodes: int,
        etype: Optional[np.ndarray] = None, allowed_mask: int = 0xFFFFFFFF,
        max_levels: int = 64):
    """Level-synchronous multi-source BFS; u32 dist, UNVISITED sentinel."""
    dist = np.full(num_nodes, UNVISITED, dtype=np.uint32)
    frontier = np.unique(np.asarray(sources, dtype=np.int64))
    dist[frontier] = 0
    level = 0
    while len(frontier) and level < max_levels:
        level += 1
        nxt = []
        for u in frontier:
            beg, end = row_off[u], row_off[u + 1]
            for e in range(beg, end):
                if etype is not None and not ((allowed_mask >> int(etype[e])) & 1):
                    continue
                v = col[e]
                if dist[v] == UNVISITED:
                    dist[v] = level
                    nxt.append(v)
        frontier = np.asarray(nxt, dtype=np.int64)
    return dist


def bfs_level(row_off, col, frontier, dist, level: int,
              etype: Optional[np.ndarray] = None, allowed_mask: int = 0xFFFFFFFF):
    """Expand ONE BFS level (claim semantics identical to the HIP kernel).

    ``dist`` may exceed the local node count (distributed sent-markers)."""
    nxt = []
    for u in frontier:
        for e in range(row_off[u], row_off[u + 1]):
            if etype is not None and not ((allowed_mask >> int(etype[e])) & 1):
                continue
            v = int(col[e])
            if dist[v] == UNVISITED:
                dist[v] = level
                nxt.append(v)
    return np.asarray(nxt, dtype=np.int64)


def reach_hops(row_off, col, sources, targets, num_nodes: int,
               etype: Optional[np.ndarray] = None, allowed_mask: int = 0xFFFFFFFF,
               max_depth: int = 16):
    """Per-source reach, from the definition: one queue BFS per source.

    Returns u8 ``hops[t, s]`` = distance from ``sources[s]`` to ``targets[t]``
    when it is at most ``max_depth`` (clamped to [0, 254]), else 255.  A node
    at distance ``max_depth`` is recorded but not expanded, as in
    ``UnifiedGraph.bfs``; duplicate sources each keep their column."""
    from collections import deque

    sources = np.asarray(sources, dtype=np.int64)
    targets = np.asarray(targets, dtype=np.int64)
    depth = max(0, min(int(max_depth), 254))
    hops = np.full((len(targets), len(sources)), 255, dtype=np.uint8)
    for s, src in enumerate(sources):
        dist = np.full(num_nodes, -1, dtype=np.int64)
        dist[src] = 0
        queue = deque([int(src)])
        while queue:
            u = queue.popleft()
            if dist[u] >= depth:
                continue
            for e in range(int(row_off[u]), int(row_off[u + 1])):
                if etype is not None and not ((allowed_mask >> int(etype[e])) & 1):
                    continue
                v = int(col[e])
                if dist[v] < 0:
                    dist[v] = dist[u] + 1
                    queue.append(v)
        d = dist[targets]
        hops[d >= 0, s] = d[d >= 0]
    return hops


def impact_query(row_off, col, query_sources, etype=None, allowed_mask: int = 0xFFFFFFFF,
                 max_hops: int = 4, max_nodes: int = 4096):
    """Reference bounded blast-radius query.  Returns list of {node: hop}."""
    results = []
    for s in query_sources:
        hops = {int(s): 0}
        frontier = [int(s)]
        truncated = False
        for hop in range(1, max_hops + 1):
            nxt = []
            for u in frontier:
                for e in range(row_off[u], row_off[u + 1]):
                    if etype is not None and not ((allowed_mask >> int(etype[e])) & 1):
                        continue
                    v = int(col[e])
                    if v not in hops:
                        if len(hops) >= max_nodes:
                            truncated = True
                            continue
                        hops[v] = hop
                        nxt.append(v)
            frontier = nxt
        results.append((hops, truncated))
    return results


def risk_score(severity, n_agents, n_creds, n_tools, flags, epss, scorecard, reach,
               weights: Optional[np.ndarray] = None):
    """Vectorized reference of the risk-score kernel (f32 arithmetic)."""
    if weights is None:
        from agentbom_amd.ops.native import risk_weights_array

        weights = risk_weights_array()
    w = weights.astype(np.float32)
    sev = np.asarray(severity)
    base = np.zeros(len(sev), dtype=np.float32)
    base[sev == 5] = w[0]
    base[sev == 4] = w[1]
    base[sev == 3] = w[2]
    base[sev == 2] = w[3]
    af = np.minimum(n_agents.astype(np.float32) * w[4], w[5])
    cf = np.minimum(n_creds.astype(np.float32) * w[6], w[7])
    tf = np.minimum(n_tools.astype(np.float32) * w[8], w[9])
    ai_signals = (flags & 1).astype(np.int32) + (n_creds > 0) + (n_tools > 0)
    ai = np.where(ai_signals >= 2, w[10], 0.0).astype(np.float32)
    kev = np.where((flags & 2) != 0, w[11], 0.0).astype(np.float32)
    ep = np.where(epss >= w[13], w[12], 0.0).astype(np.float32)
    sc = np.zeros(len(sev), dtype=np.float32)
    has_sc = scorecard >= 0
    sc = np.where(has_sc & (scorecard < w[14]), w[15], sc)
    sc = np.where(has_sc & (scorecard >= w[14]) & (scorecard < w[16]), w[17], sc)
    sc = np.where(has_sc & (scorecard >= w[16]) & (scorecard < w[18]), w[19], sc)
    ra = np.where(reach == 1, w[20], np.where(reach == 0, -w[21], 0.0)).astype(np.float32)
    total = base + af + cf + tf + ai + kev + ep + sc + ra
    out = np.clip(total, 0.0, 10.0).astype(np.float32)
    out[(flags & 4) != 0] = 0.0
    return out


def severity_histogram(owner, severity, num_containers: int):
    hist = np.zeros((num_containers, 6), dtype=np.uint32)
    np.add.at(hist, (np.asarray(owner, dtype=np.int64), np.asarray(severity, dtype=np.int64)), 1)
    return hist


# ── attack/exposure path DP (oracle for csrc/paths.hip) ─────────────────────

PATH_NO_EDGE = np.uint64(0xFFFFFFFF)


def _ordered_f32(f):
    """Order-preserving u32 image of non-negative float32 scores."""
    u = np.asarray(f, dtype=np.float32).view(np.uint32)
    return (u | np.uint32(0x80000000)).astype(np.uint64)


def path_unordered_f32(u):
    """Inverse of _ordered_f32 for valid (non-negative-score) labels."""
    raw = (np.asarray(u, dtype=np.uint64) & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    return raw.view(np.float32)


def path_pack(score, edge):
    return (_ordered_f32(score) << np.uint64(32)) | np.asarray(edge, dtype=np.uint64)


def path_relax(edge_src, col, etype, edge_weight, cur, node_boost,
               etype_boost, etype_trav, etype_gate, node_gate):
    """One hop of the max-score path DP; exact mirror of abom_path_relax.

    ``cur``/returned ``nxt`` are u64 [N*2] packed labels
    ((ordered_f32(score) << 32) | winner_edge); slot 0 = ungated path,
    slot 1 = path that used a gate edge or touched a gated node.  The
    kernel's atomicMax == np.maximum.at (both order-independent).
    """
    nxt = np.zeros_like(cur)
    et = np.asarray(etype)
    keep = etype_trav[et].astype(bool)
    e_idx = np.nonzero(keep)[0]
    if not len(e_idx):
        return nxt
    u = np.asarray(edge_src, dtype=np.int64)[e_idx]
    v = np.asarray(col, dtype=np.int64)[e_idx]
    step = etype_boost[et[e_idx]].astype(np.float32) + node_boost[v].astype(np.float32)
    if edge_weight is not None:
        step = step + edge_weight[e_idx].astype(np.float32) * np.float32(0.3)
    gate = etype_gate[et[e_idx]].astype(bool)
    if node_gate is not None:
        gate = gate | node_gate[v].astype(bool)

    esrc_all = np.asarray(edge_src, dtype=np.int64)

    def not_backtrack(labels):
        # predecessor-avoidance: block relaxing straight back to the node
        # the label came from (matches the kernel's 2-cycle guard)
        pe = (labels & np.uint64(0xFFFFFFFF)).astype(np.int64)
        no_edge = pe == 0xFFFFFFFF
        pred = np.where(no_edge, -1, esrc_all[np.where(no_edge, 0, pe)])
        return no_edge | (pred != v)

    lu0 = cur[u * 2]
    m = (lu0 != 0) & not_backtrack(lu0)
    if m.any():
        s = path_unordered_f32(lu0[m] >> np.uint64(32)) + step[m]
        cand = path_pack(s, e_idx[m])
        np.maximum.at(nxt, v[m] * 2 + gate[m], cand)
    lu1 = cur[u * 2 + 1]
    m = (lu1 != 0) & not_backtrack(lu1)
    if m.any():
        s = path_unordered_f32(lu1[m] >> np.uint64(32)) + step[m]
        cand = path_pack(s, e_idx[m])
        np.maximum.at(nxt, v[m] * 2 + 1, cand)
    return nxt


# ── centrality (oracle for csrc/centrality.hip) ─────────────────────────────

PAGERANK_TOLERANCE = 1e-10


def _row_ids(row_off, num_nodes: int):
    """Owning row of every CSR slot, in CSR order."""
    deg = np.diff(np.asarray(row_off, dtype=np.int64))
    return np.repeat(np.arange(num_nodes, dtype=np.int64), deg)


def pagerank(rev_off, rev_col, out_degree, num_nodes: int, damping: float = 0.85,
             iterations: int = 50):
    """Pull power iteration over the reverse CSR; fp64 [N].

    new[v] = (1-d)/n + d * sum_{u in in(v)} rank[u]/outdeg[u] + d * dangling/n,
    with the in-neighbour sum taken in CSR order.  Stops after ``iterations``
    passes or after the first pass whose L1 change is below 1e-10.
    """
    n = int(num_nodes)
    if n == 0:
        return np.zeros(0, dtype=np.float64)
    dst = _row_ids(rev_off, n)
    src = np.asarray(rev_col, dtype=np.int64)
    out_deg = np.asarray(out_degree, dtype=np.float64)
    dangling_nodes = out_deg == 0
    rank = np.full(n, 1.0 / n)
    teleport = (1.0 - damping) / n
    for _ in range(iterations):
        contrib = np.where(dangling_nodes, 0.0, rank / np.maximum(out_deg, 1.0))
        pulled = np.zeros(n, dtype=np.float64)
        if len(src):
            np.add.at(pulled, dst, contrib[src])
        new = teleport + damping * pulled + damping * rank[dangling_nodes].sum() / n
        change = np.abs(new - rank).sum()
        rank = new
        if change < PAGERANK_TOLERANCE:
            break
    return rank


def _expand_rows(row_off, rows):
    """(slot index, owning row) for every CSR slot of ``rows``, row by row."""
    beg = row_off[rows]
    cnt = row_off[rows + 1] - beg
    total = int(cnt.sum())
    if total == 0:
        empty = np.zeros(0, dtype=np.int64)
        return empty, empty
    ends = np.cumsum(cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(ends - cnt, cnt)
    return np.repeat(beg, cnt) + within, np.repeat(rows, cnt)


def betweenness(fwd_off, fwd_col, num_nodes: int, sources,
                etype: Optional[np.ndarray] = None, allowed_mask: int = 0xFFFFFFFF):
    """Un-normalised Brandes betweenness (unweighted) over the forward CSR;
    fp64 [N].  Level-synchronous per source: sigma flows down the BFS levels,
    delta back up, and every reached node except the source adds its delta.
    Parallel edges count once each; ``etype``/``allowed_mask`` filter edges as
    in :func:`bfs`.
    """
    n = int(num_nodes)
    bc = np.zeros(n, dtype=np.float64)
    off = np.asarray(fwd_off, dtype=np.int64)
    col = np.asarray(fwd_col, dtype=np.int64)
    keep = None
    if etype is not None:
        keep = ((np.uint32(allowed_mask) >> np.asarray(etype, dtype=np.uint32)) & 1).astype(bool)
    for s in np.asarray(sources, dtype=np.int64):
        dist = np.full(n, -1, dtype=np.int64)
        sigma = np.zeros(n, dtype=np.float64)
        dist[s], sigma[s] = 0, 1.0
        frontier = np.array([s], dtype=np.int64)
        dag = []  # per level: (u, w) edges with dist[w] == dist[u] + 1
        level = 0
        while len(frontier):
            level += 1
            slots, u = _expand_rows(off, frontier)
            if keep is not None:
                sel = keep[slots]
                slots, u = slots[sel], u[sel]
            w = col[slots]
            fresh = np.unique(w[dist[w] < 0])
            dist[fresh] = level
            down = dist[w] == level
            u, w = u[down], w[down]
            np.add.at(sigma, w, sigma[u])
            dag.append((u, w))
            frontier = fresh
        delta = np.zeros(n, dtype=np.float64)
        for u, w in reversed(dag):
            np.add.at(delta, u, sigma[u] / sigma[w] * (1.0 + delta[w]))
        reached = dist >= 0
        reached[s] = False
        bc[reached] += delta[reached]
    return bc


# ── connected components (oracle for csrc/components.hip) ───────────────────


def connected_components(edge_src, col, num_nodes: int,
                         etype: Optional[np.ndarray] = None, allowed_mask: int = 0xFFFFFFFF):
    """Weakly connected components of an edge list; int32 labels [N], each the
    smallest node id of the node's component (the kernel's contract).

    Min-label propagation to a fixed point: every edge whose endpoints carry
    different labels pulls the larger label's entry down to the smaller
    (``np.minimum.at``), then pointer jumping flattens ``labels[labels]``;
    repeated until no edge disagrees.  ``etype``/``allowed_mask`` filter
    edges as in :func:`bfs`.
    """
    n = int(num_nodes)
    labels = np.arange(n, dtype=np.int64)
    u = np.asarray(edge_src, dtype=np.int64)
    v = np.asarray(col, dtype=np.int64)
    if etype is not None:
        keep = ((np.uint32(allowed_mask) >> np.asarray(etype, dtype=np.uint32)) & 1).astype(bool)
        u, v = u[keep], v[keep]
    while len(u):
        lu, lv = labels[u], labels[v]
        differ = lu != lv
        if not differ.any():
            break
        lo = np.minimum(lu, lv)[differ]
        hi = np.maximum(lu, lv)[differ]
        np.minimum.at(labels, hi, lo)
        while True:
            jumped = labels[labels]
            if np.array_equal(jumped, labels):
                break
            labels = jumped
    return labels.astype(np.int32)


def component_stats(comp, kind, num_components: int, num_kinds: int,
                    weight: Optional[np.ndarray] = None, worst: Optional[np.ndarray] = None):
    """Per-component roll-up, the mirror of abom_component_stats: returns
    ``(kind_counts int32 [C, num_kinds], weight_sum int64 [C], worst_min
    int32 [C])``.  ``comp`` is a dense component index per node, ``kind`` the
    node class, ``weight`` an int32 column summed in 64 bits, ``worst`` a
    severity column where lower is worse.  Without ``weight`` the sums are 0;
    without ``worst`` worst_min is -1 (the kernel's 0xFFFFFFFF fill)."""
    C, K = int(num_components), int(num_kinds)
    comp = np.asarray(comp, dtype=np.int64)
    kind_counts = np.bincount(comp * K + np.asarray(kind, dtype=np.int64),
                              minlength=C * K).astype(np.int32).reshape(C, K)
    weight_sum = np.zeros(C, dtype=np.int64)
    if weight is not None:
        np.add.at(weight_sum, comp, np.asarray(weight, dtype=np.int64))
    worst_min = np.full(C, 0xFFFFFFFF, dtype=np.uint32)
    if worst is not None:
        np.minimum.at(worst_min, comp, np.asarray(worst, dtype=np.uint32))
    return kind_counts, weight_sum, worst_min.view(np.int32)


# ── multi-hop delegation expansion (oracle for csrc/blast_hops.hip) ─────────

BLAST_HOPS_MAX_DEPTH = 5


def blast_hops(pkgs, rev_off, rev_col, rev_et, et_contains, et_uses, et_has_cred,
               fwd_off, fwd_col, fwd_et, max_depth: int):
    """Multi-hop delegation blast radius per package node, as plain sets.

    With srv(a) the distinct USES targets of agent a, ag(s) the distinct USES
    sources of server s, cr(s) the distinct HAS_CRED targets of s and
    D = clamp(max_depth, 1, 5): S0 = holders of p (reverse CONTAINS),
    A_1 = ag(S0), F_1 = srv(A_1) \\ S0, then for h = 1..D-1
    A_{h+1} = ag(F_h) \\ visited agents and, while h+1 < D,
    F_{h+1} = srv(A_{h+1}) \\ visited servers; the walk stops at an empty
    level.  The level BFS of models/blast.py expand_blast_radius_hops.

    Returns ``(hop_agents int32 [U,4], t_creds int32 [U], hop_depth uint8
    [U])``: |A_h| for h = 2..5, the distinct credentials on every server of
    every transitive agent (h >= 2), and the largest h with |A_h| > 0, else 1.
    """
    depth = max(1, min(int(max_depth), BLAST_HOPS_MAX_DEPTH))
    pkgs = np.asarray(pkgs, dtype=np.int64)
    U = len(pkgs)
    hop_agents = np.zeros((U, 4), dtype=np.int32)
    t_creds = np.zeros(U, dtype=np.int32)
    hop_depth = np.ones(U, dtype=np.uint8)

    def neighbours(off, col, et, want):
        cache: dict = {}

        def of(node):
            got = cache.get(node)
            if got is None:
                beg, end = int(off[node]), int(off[node + 1])
                got = cache[node] = frozenset(
                    int(col[e]) for e in range(beg, end) if et[e] == want)
            return got
        return of

    holders = neighbours(rev_off, rev_col, rev_et, et_contains)
    ag = neighbours(rev_off, rev_col, rev_et, et_uses)
    srv = neighbours(fwd_off, fwd_col, fwd_et, et_uses)
    cr = neighbours(fwd_off, fwd_col, fwd_et, et_has_cred)

    def union(fn, nodes):
        out: set = set()
        for v in nodes:
            out |= fn(v)
        return out

    for i, p in enumerate(pkgs):
        s0 = set(holders(int(p)))
        a1 = union(ag, s0)
        seen_s, seen_a = set(s0), set(a1)
        frontier = union(srv, a1) - s0
        seen_s |= frontier
        transitive: set = set()
        for h in range(1, depth):
            level = union(ag, frontier) - seen_a
            if not level:
                break
            seen_a |= level
            transitive |= level
            hop_agents[i, h - 1] = len(level)
            hop_depth[i] = h + 1
            if h + 1 < depth:
                frontier = union(srv, level) - seen_s
                seen_s |= frontier
        t_creds[i] = len(union(cr, union(srv, transitive)))
    return hop_agents, t_creds, hop_depth


# the per-item arrays of the remediation plan, in the order they are documented
REMEDIATION_KEYS = (
    "item", "rep_pkg", "installs", "n_findings", "n_vulns", "max_score", "worst_sev", "kev",
    "fix_hi", "fix_lo", "n_unfixed", "n_servers", "n_agents", "n_creds", "n_tools")


def remediation_item_of(pkg_group_key, pkg_key_hi, pkg_key_lo):
    """``item_of`` int32 [P]: the index of every package's (group key, key hi,
    key lo) triple among the distinct triples in ascending unsigned
    lexicographic order."""
    triples = list(zip(np.asarray(pkg_group_key).view(np.uint64).tolist(),
                       np.asarray(pkg_key_hi).view(np.uint64).tolist(),
                       np.asarray(pkg_key_lo).view(np.uint64).tolist()))
    rank = {t: i for i, t in enumerate(sorted(set(triples)))}
    return np.asarray([rank[t] for t in triples], dtype=np.int32)


def remediation_plan(pkg_idx, win_idx, scores, item_of,
                     rev_off, rev_col, rev_et, fwd_off, fwd_col, fwd_et,
                     et_contains: int, et_uses: int, et_has_cred: int, et_tool: int,
                     pkg_base: int, w_flags, w_fixed_hi, w_fixed_lo, a_severity, a_kev,
                     n_agents_total: int) -> dict:
    """Fix-first remediation plan of a step's findings, from the definitions.

    An item is a distinct (name, version); ``item_of`` maps a package index to
    its item.  Per item with at least one finding, in ascending item index
    (the keys of ``REMEDIATION_KEYS``): ``rep_pkg`` its smallest matched
    package, ``installs`` its distinct matched packages, ``n_findings``,
    ``n_vulns`` distinct windows, ``max_score`` fp32, ``worst_sev`` and ``kev``
    uint8 over its windows, (``fix_hi``, ``fix_lo``) int64 bit patterns of the
    largest fixed key -- unsigned 128-bit order -- over its windows with
    WF_HAS_FIXED (0, 0 without one), ``n_unfixed`` distinct windows without
    it, ``n_servers`` distinct sources of CONTAINS edges into a matched
    install and ``n_agents`` / ``n_creds`` / ``n_tools`` the distinct agents
    (USES sources), creds (HAS_CRED targets) and tools (PROVIDES_TOOL targets)
    of those servers, unfiltered.  On top: ``agents_pct`` fp32 = (100 *
    n_agents) / n_agents_total and ``order`` int64, the positions sorted by
    max_score descending, n_agents descending, item ascending."""
    pkg_idx = np.asarray(pkg_idx, dtype=np.int64)
    win_idx = np.asarray(win_idx, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    fhi, flo = np.asarray(w_fixed_hi).view(np.uint64), np.asarray(w_fixed_lo).view(np.uint64)

    def row(off, col, et, node, want):
        return {int(col[e]) for e in range(int(off[node]), int(off[node + 1])) if et[e] == want}

    groups: dict = {}
    for f in range(len(pkg_idx)):
        groups.setdefault(int(item_of[pkg_idx[f]]), []).append(f)
    out = {k: [] for k in REMEDIATION_KEYS}
    for item in sorted(groups):
        fs = groups[item]
        pkgs = {int(pkg_idx[f]) for f in fs}
        wins = {int(win_idx[f]) for f in fs}
        fixed = [(int(fhi[w]), int(flo[w])) for w in wins if w_flags[w] & WF_HAS_FIXED]
        best = max(fixed) if fixed else (0, 0)
        servers: set = set()
        for p in pkgs:
            servers |= row(rev_off, rev_col, rev_et, p + pkg_base, et_contains)
        agents, creds, tools = set(), set(), set()
        for s in servers:
            agents |= row(rev_off, rev_col, rev_et, s, et_uses)
            creds |= row(fwd_off, fwd_col, fwd_et, s, et_has_cred)
            tools |= row(fwd_off, fwd_col, fwd_et, s, et_tool)
        for key, value in zip(REMEDIATION_KEYS, (
                item, min(pkgs), len(pkgs), len(fs), len(wins),
                max(scores[f] for f in fs), max(int(a_severity[w]) for w in wins),
                int(any(a_kev[w] for w in wins)), best[0], best[1],
                len(wins) - len(fixed), len(servers), len(agents), len(creds), len(tools))):
            out[key].append(value)
    dtypes = dict.fromkeys(REMEDIATION_KEYS, np.int32)
    dtypes.update(max_score=np.float32, worst_sev=np.uint8, kev=np.uint8)
    res = {k: np.asarray(out[k], dtype=dtypes[k]) for k in REMEDIATION_KEYS
           if k not in ("fix_hi", "fix_lo")}
    for k in ("fix_hi", "fix_lo"):
        res[k] = np.asarray(out[k], dtype=np.uint64).view(np.int64)
    res["agents_pct"] = (np.float32(100.0) * res["n_agents"].astype(np.float32)
                         / np.float32(n_agents_total))
    M = len(res["item"])
    res["order"] = np.asarray(
        sorted(range(M), key=lambda m: (-float(res["max_score"][m]), -int(res["n_agents"][m]),
                                        int(res["item"][m]))), dtype=np.int64)
    return res


# ── toxic combinations (oracle for csrc/toxic.hip) ──────────────────────────

# tool capability bits of ``tool_caps``
TC_EXEC, TC_WRITE, TC_DELETE, TC_READ, TC_RETRIEVAL = 1, 2, 4, 8, 16
TC_DANGEROUS = TC_EXEC | TC_WRITE | TC_DELETE
# pattern bits of a finding, in the order of ``n_by_pattern``
TP_CRED_BLAST, TP_KEV_WITH_CREDS, TP_EXECUTE_EXPLOIT = 1, 2, 4
TP_CACHE_POISON, TP_LATERAL_CHAIN, TP_MULTI_AGENT_CVE = 8, 16, 32
TOXIC_PATTERN_NAMES = ("cred_blast", "kev_with_credentials", "execute_exploit",
                       "cache_poison", "lateral_chain", "multi_agent_cve")
# per pattern bit: (fp32 multiplier of the score, default without a score)
TOXIC_SCORING = ((1.5, 9.0), (None, 10.0), (1.3, 8.5), (1.5, 9.5), (1.4, 9.0), (1.2, 7.5))
TOXIC_HOT_SEVERITY = 4      # high; 5 is critical
TOXIC_MULTI_AGENTS = 3      # agents of one advisory from which it is multi-agent
# the per-advisory arrays, in the order they are documented
TOXIC_VULN_KEYS = ("vuln", "n_findings", "n_packages", "n_servers", "n_agents", "max_score",
                   "worst_sev", "kev", "patterns")


def _toxic_score(bit_index: int, s) -> np.float32:
    """One fp32 multiply by an fp32 constant, then a min: nothing to fuse."""
    mult, default = TOXIC_SCORING[bit_index]
    if mult is None or not s > 0:
        return np.float32(default)
    return min(np.float32(s) * np.float32(mult), np.float32(10.0))


def toxic_combinations(pkg_idx, win_idx, scores, n_creds, n_tools,
                       rev_off, rev_col, rev_et, fwd_off, fwd_col, fwd_et,
                       et_contains: int, et_uses: int, et_tool: int, pkg_base: int,
                       a_severity, a_kev, a_impact, tool_lut, tool_base: int,
                       tool_is_db, tool_caps, vuln_of=None) -> dict:
    """Toxic combinations of a step's findings, from the definitions: risks
    that are tolerable alone and critical together (the reference's
    ``toxic_combos.py``, per finding and per advisory).

    For finding f with package p, window w, ``hot`` = a_severity[w] >= 4 and
    advisory v = vuln_of[w] (w itself without a map): the servers of p are the
    distinct CONTAINS sources of node p + pkg_base, the agents of a server its
    distinct USES sources, and ``exposed`` the OR of ``tool_caps`` (u8
    [n_tools], indexed by node - tool_base) over the PROVIDES_TOOL targets of
    those servers -- all of them at tool_lut[a_impact[w]] == 2, those with
    ``tool_is_db`` at 1, none at 0, the filter of the step's ``n_tools``
    (a finding that exposes a capability with n_tools[f] == 0 is refused).
    ``patterns`` u8 [F]: TP_CRED_BLAST hot and n_creds[f] > 0;
    TP_KEV_WITH_CREDS a_kev[w] and n_creds[f] > 0; TP_EXECUTE_EXPLOIT hot and
    exposed & TC_DANGEROUS; TP_CACHE_POISON hot and exposed & TC_RETRIEVAL;
    TP_LATERAL_CHAIN hot and a server of p has >= 2 agents;
    TP_MULTI_AGENT_CVE, at any severity, v has >= 3 distinct agents over the
    servers of all packages of all its findings.  ``combo_score`` fp32 [F]:
    the largest of the set bits' scores (``TOXIC_SCORING``: min(s * mult, 10)
    with s = scores[f], for the multi-agent bit s = the advisory's largest
    score; the default where s is not > 0), 0.0 without a bit.  The reference
    scales the first blast radius it met; the advisory's maximum is used here
    because it does not depend on order.

    Returns ``patterns`` and ``combo_score`` per finding and, under ``vulns``,
    per advisory with a finding, ascending (``TOXIC_VULN_KEYS``): ``vuln``,
    ``n_findings``, ``n_packages``, ``n_servers``, ``n_agents`` int32,
    ``max_score`` fp32, ``worst_sev``, ``kev`` and ``patterns`` (OR over its
    findings) u8; ``order`` int64, the positions by max_score descending,
    n_agents descending, vuln ascending.  On top: ``poison_servers`` int32: the nodes
    with >= 2 agents whose unfiltered tool caps hold TC_WRITE and TC_READ or
    TC_RETRIEVAL (the reference's cross-agent poison), ascending.
    ``n_by_pattern`` int64 [6] findings per bit, ``n_multi_agent`` the number
    of multi-agent advisories.

    Out of scope: TRANSITIVE_CRITICAL (the estate has no direct/transitive
    flag), the keyword text of titles, deduplication by title."""
    pkg_idx = np.asarray(pkg_idx, dtype=np.int64)
    win_idx = np.asarray(win_idx, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    F = len(pkg_idx)
    num_nodes = len(rev_off) - 1
    n_tool_nodes = len(tool_caps)

    def row(off, col, et, node, want):
        return {int(col[e]) for e in range(int(off[node]), int(off[node + 1])) if et[e] == want}

    def caps_of(server, db_only=False):
        caps = 0
        for t in row(fwd_off, fwd_col, fwd_et, server, et_tool):
            k = t - tool_base
            if 0 <= k < n_tool_nodes and (not db_only or tool_is_db[k]):
                caps |= int(tool_caps[k])
        return caps

    patterns = np.zeros(F, dtype=np.uint8)
    by_vuln: dict = {}
    for f in range(F):
        p, w = int(pkg_idx[f]), int(win_idx[f])
        servers = row(rev_off, rev_col, rev_et, p + pkg_base, et_contains)
        cls = int(tool_lut[a_impact[w]])
        exposed = 0
        for s in servers:
            exposed |= caps_of(s, db_only=cls == 1) if cls else 0
        if exposed and not n_tools[f] > 0:
            raise ValueError(f"finding {f} exposes a tool capability with n_tools == 0")
        hot = int(a_severity[w]) >= TOXIC_HOT_SEVERITY
        creds = n_creds[f] > 0
        shared = any(len(row(rev_off, rev_col, rev_et, s, et_uses)) >= 2 for s in servers)
        bits = 0
        if hot and creds:
            bits |= TP_CRED_BLAST
        if a_kev[w] and creds:
            bits |= TP_KEV_WITH_CREDS
        if hot and exposed & TC_DANGEROUS:
            bits |= TP_EXECUTE_EXPLOIT
        if hot and exposed & TC_RETRIEVAL:
            bits |= TP_CACHE_POISON
        if hot and shared:
            bits |= TP_LATERAL_CHAIN
        patterns[f] = bits
        by_vuln.setdefault(w if vuln_of is None else int(vuln_of[w]), []).append(f)

    per = {k: [] for k in TOXIC_VULN_KEYS}
    for v in sorted(by_vuln):
        fs = by_vuln[v]
        pkgs = {int(pkg_idx[f]) for f in fs}
        servers: set = set()
        for p in pkgs:
            servers |= row(rev_off, rev_col, rev_et, p + pkg_base, et_contains)
        agents: set = set()
        for s in servers:
            agents |= row(rev_off, rev_col, rev_et, s, et_uses)
        if len(agents) >= TOXIC_MULTI_AGENTS:
            for f in fs:
                patterns[f] |= TP_MULTI_AGENT_CVE
        bits = 0
        for f in fs:
            bits |= int(patterns[f])
        for key, value in zip(TOXIC_VULN_KEYS, (
                v, len(fs), len(pkgs), len(servers), len(agents), max(scores[f] for f in fs),
                max(int(a_severity[win_idx[f]]) for f in fs),
                int(any(a_kev[win_idx[f]] for f in fs)), bits)):
            per[key].append(value)
    dtypes = dict.fromkeys(TOXIC_VULN_KEYS, np.int32)
    dtypes.update(max_score=np.float32, worst_sev=np.uint8, kev=np.uint8, patterns=np.uint8)
    vulns = {k: np.asarray(per[k], dtype=dtypes[k]) for k in TOXIC_VULN_KEYS}
    vuln_max = dict(zip(vulns["vuln"].tolist(), vulns["max_score"]))

    combo = np.zeros(F, dtype=np.float32)
    for f in range(F):
        v = int(win_idx[f]) if vuln_of is None else int(vuln_of[win_idx[f]])
        for b in range(6):
            if patterns[f] >> b & 1:
                s = vuln_max[v] if 1 << b == TP_MULTI_AGENT_CVE else scores[f]
                combo[f] = max(combo[f], _toxic_score(b, s))
    M = len(vulns["vuln"])
    vulns["order"] = np.asarray(
        sorted(range(M), key=lambda m: (-float(vulns["max_score"][m]),
                                        -int(vulns["n_agents"][m]), int(vulns["vuln"][m]))),
        dtype=np.int64)
    poison = []
    for s in range(num_nodes):
        if len(row(rev_off, rev_col, rev_et, s, et_uses)) >= 2:
            caps = caps_of(s)
            if caps & TC_WRITE and caps & (TC_READ | TC_RETRIEVAL):
                poison.append(s)
    return {
        "patterns": patterns, "combo_score": combo, "vulns": vulns,
        "poison_servers": np.asarray(poison, dtype=np.int32),
        "n_by_pattern": np.asarray(
            [int(np.count_nonzero(patterns >> b & 1)) for b in range(6)], dtype=np.int64),
        "n_multi_agent": int(np.count_nonzero(vulns["n_agents"] >= TOXIC_MULTI_AGENTS)),
    }
