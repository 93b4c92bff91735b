"""Inputs and oracles for the score, score-gather, rank and histogram tests
(ops/csrc/score.hip, ops/csrc/rank.hip).  numpy only, apart from the rank
oracle, which is the torch key sort that the kernel replaces.

Weights: with the default config six of the 22 weight fields are 0.5, so two
of them could trade places between ``native.risk_weights_array()``, the
kernel's ``RiskWeights`` and ``cpu_ref.risk_score`` unnoticed.  ``DYADIC``
gives each field its own value, a multiple of 1/64, so every term and every
partial sum of the formula is exact in f32 and in f64 alike and the three
sides can be compared with ``==``.
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from agentbom_amd.ops import cpu_ref

UNVISITED = 0xFFFFFFFF

# config name -> value, in the order of models/blast.py's formula, which is
# the order of native.risk_weights_array() and of RiskWeights in score.hip
DYADIC = {
    "RISK_BASE_CRITICAL": 8.25,
    "RISK_BASE_HIGH": 6.125,
    "RISK_BASE_MEDIUM": 4.0625,
    "RISK_BASE_LOW": 2.03125,
    "RISK_AGENT_WEIGHT": 0.4375,      # cap reached at exactly 4 agents
    "RISK_AGENT_CAP": 1.75,
    "RISK_CRED_WEIGHT": 0.28125,      # ... at exactly 5 credentials
    "RISK_CRED_CAP": 1.40625,
    "RISK_TOOL_WEIGHT": 0.109375,     # ... at exactly 9 tools
    "RISK_TOOL_CAP": 0.984375,
    "RISK_AI_BOOST": 0.515625,
    "RISK_KEV_BOOST": 1.015625,
    "RISK_EPSS_BOOST": 0.546875,
    "EPSS_CRITICAL_THRESHOLD": 0.6875,
    "RISK_SCORECARD_TIER1_THRESHOLD": 3.25,
    "RISK_SCORECARD_TIER1_BOOST": 0.765625,
    "RISK_SCORECARD_TIER2_THRESHOLD": 5.5,
    "RISK_SCORECARD_TIER2_BOOST": 0.484375,
    "RISK_SCORECARD_TIER3_THRESHOLD": 7.75,
    "RISK_SCORECARD_TIER3_BOOST": 0.265625,
    "RISK_REACHABLE_BOOST": 0.578125,
    "RISK_UNREACHABLE_PENALTY": 0.640625,
}
WEIGHT_NAMES = tuple(DYADIC)


def default_weights() -> dict:
    """The config's own values, by name (read before anything patches them)."""
    from agentbom_amd.utils import config as cfg

    return {name: getattr(cfg, name) for name in WEIGHT_NAMES}


def set_weights(monkeypatch, weights: dict) -> None:
    """Both risk_weights_array() and risk_score_from_counts read cfg live."""
    from agentbom_amd.utils import config as cfg

    for name, value in weights.items():
        monkeypatch.setattr(cfg, name, value)


# ── the risk-score grid ─────────────────────────────────────────────────────

SEVERITIES = (5, 4, 3, 2, 0, 1, 6, 255)       # the last four have base 0
REACH = (-1, 0, 1)
BIG_COUNT = 2**31 + 5


def _count_values(weight: float, cap: float) -> tuple:
    at_cap = round(cap / weight)
    return (0, 1, at_cap, at_cap + 1, BIG_COUNT)


def risk_grid(weights: dict) -> dict:
    """Columns of the grid, as decimal (python float / int) lists under
    ``spec_*`` for models/blast.py and as the kernel's arrays otherwise.

    Two blocks: severity x flags x epss x scorecard x reach in full, with the
    count triples cycling under them; then count triples x flags x reach in
    full, with the rest cycling."""
    thr = weights["EPSS_CRITICAL_THRESHOLD"]
    # None, 0.0, just below / at / above the threshold
    epss = (None, 0.0, thr - 1e-4, thr, thr + 1e-4)
    scorecard = [None, 0.0]
    for t in ("RISK_SCORECARD_TIER1_THRESHOLD", "RISK_SCORECARD_TIER2_THRESHOLD",
              "RISK_SCORECARD_TIER3_THRESHOLD"):
        scorecard += [weights[t] - 1e-3, weights[t], weights[t] + 1e-3]
    agents = _count_values(weights["RISK_AGENT_WEIGHT"], weights["RISK_AGENT_CAP"])
    creds = _count_values(weights["RISK_CRED_WEIGHT"], weights["RISK_CRED_CAP"])
    tools = _count_values(weights["RISK_TOOL_WEIGHT"], weights["RISK_TOOL_CAP"])
    triples = [(a, c, t) for a in agents for c in creds for t in tools]

    rows = []
    i = 0
    for sev in SEVERITIES:
        for fl in range(8):
            for ep in epss:
                for sc in scorecard:
                    for rc in REACH:
                        rows.append((sev, *triples[i % len(triples)], fl, ep, sc, rc))
                        i += 1
    for tr in triples:
        for fl in range(8):
            for rc in REACH:
                rows.append((SEVERITIES[i % 8], *tr, fl, epss[i % 5],
                             scorecard[i % 11], rc))
                i += 1
    cols = list(zip(*rows))
    return {
        "spec_epss": cols[5], "spec_scorecard": cols[6],
        "severity": np.array(cols[0], dtype=np.uint8),
        "n_agents": np.array(cols[1], dtype=np.uint32),
        "n_creds": np.array(cols[2], dtype=np.uint32),
        "n_tools": np.array(cols[3], dtype=np.uint32),
        "flags": np.array(cols[4], dtype=np.uint8),   # bit0 ai_ctx, bit1 kev, bit2 suppressed
        "epss": np.array([-1.0 if v is None else v for v in cols[5]], dtype=np.float32),
        "scorecard": np.array([-1.0 if v is None else v for v in cols[6]], dtype=np.float32),
        "reach": np.array(cols[7], dtype=np.int8),
    }


KERNEL_COLUMNS = ("severity", "n_agents", "n_creds", "n_tools", "flags", "epss",
                  "scorecard", "reach")


def tile(grid: dict, n: int) -> dict:
    return {k: np.resize(grid[k], n) for k in KERNEL_COLUMNS}


def reference_scores(cols: dict) -> np.ndarray:
    """cpu_ref.risk_score under the weights currently in the config."""
    return cpu_ref.risk_score(*(cols[k] for k in KERNEL_COLUMNS))


def spec_scores(grid: dict) -> np.ndarray:
    """models/blast.py, row by row, in f64 on the decimal values.  A
    suppressed finding scores 0.0 (BlastRadius.calculate_risk_score)."""
    from agentbom_amd.models import SEVERITY_FROM_CODE, Severity, risk_score_from_counts

    out = np.empty(len(grid["severity"]), dtype=np.float64)
    for i in range(len(out)):
        fl = int(grid["flags"][i])
        rc = int(grid["reach"][i])
        if fl & 4:
            out[i] = 0.0
            continue
        out[i] = risk_score_from_counts(
            severity=SEVERITY_FROM_CODE.get(int(grid["severity"][i]), Severity.UNKNOWN),
            n_agents=int(grid["n_agents"][i]), n_creds=int(grid["n_creds"][i]),
            n_tools=int(grid["n_tools"][i]), has_ai_context=bool(fl & 1),
            is_kev=bool(fl & 2), epss_score=grid["spec_epss"][i],
            scorecard_score=grid["spec_scorecard"][i],
            graph_reachable=None if rc < 0 else bool(rc))
    return out


# ── score_gather ────────────────────────────────────────────────────────────

GATHER_N = 600_001


def _primes(count: int) -> np.ndarray:
    sieve = np.ones(count * 20, dtype=bool)
    sieve[:2] = False
    for p in range(2, int(len(sieve) ** 0.5) + 1):
        if sieve[p]:
            sieve[p * p::p] = False
    return np.flatnonzero(sieve)[:count]


def gather_case(weights: dict, n: int = GATHER_N) -> dict:
    """Arena columns of 60 windows, a counts table of six distinct primes per
    row, and ``n`` findings that cycle through windows x count rows x nodes
    with pairwise coprime periods."""
    thr = np.float32(weights["EPSS_CRITICAL_THRESHOLD"])
    w = 60
    k = np.arange(w)
    a_sev = np.array(SEVERITIES, dtype=np.uint8)[k % 8]
    a_kev = np.array([0, 1, 2, 255], dtype=np.uint8)[(k // 2) % 4]
    a_epss = np.array([-1.0, 0.0, np.nextafter(thr, np.float32(0)), thr,
                       np.nextafter(thr, np.float32(1)), 1.0], dtype=np.float32)[(k // 3) % 6]
    a_impact = (k % 9).astype(np.uint8)
    # full (2) / db-only (1) / none (0), different for creds and tools
    cred_lut = np.array([2, 1, 0, 2, 1, 0, 1, 2, 0], dtype=np.uint8)
    tool_lut = np.array([0, 2, 1, 1, 0, 2, 2, 0, 1], dtype=np.uint8)
    rows = 7
    counts2d = _primes(rows * 6).reshape(rows, 6).astype(np.int32)
    # three rows that primes cannot give: counts at the dyadic caps with zero
    # db counts, counts that need the unsigned cast, and counts below every cap
    counts2d[3] = [3, 4, 5, 0, 9, 0]
    counts2d[5] = [17, 2**31 - 1, 1, 2**31 - 2, 2, 2**31 - 3]
    counts2d[6] = [5, 2, 3, 1, 4, 6]
    nodes = 11
    dist = np.array([UNVISITED, 0, 7, UNVISITED, 1, 0x7FFFFFFF, 0xFFFFFFFE, UNVISITED, 2, 0, 3],
                    dtype=np.uint32)
    i = np.arange(n, dtype=np.int64)
    # 60 x 7 x 11 = 4620 combinations, all met since the periods are coprime
    win_idx = (i * 7) % w                 # a permutation of the windows, not sorted
    pos = (i * 3 + 2) % rows              # not monotonic
    pkg_nodes = (i * 5 + 1) % nodes
    return {"win_idx": win_idx, "pkg_nodes": pkg_nodes, "pos": pos, "a_sev": a_sev,
            "a_kev": a_kev, "a_epss": a_epss, "a_impact": a_impact, "cred_lut": cred_lut,
            "tool_lut": tool_lut, "counts2d": counts2d, "dist": dist}


GATHER_ARGS = ("win_idx", "pkg_nodes", "pos", "a_sev", "a_kev", "a_epss", "a_impact",
               "cred_lut", "tool_lut", "counts2d", "dist")


def gather_oracle(c: dict):
    """Plain gathers, then cpu_ref.risk_score under the config's weights.
    Returns (scores f32, n_agents, n_creds, n_tools int32)."""
    win = c["win_idx"]
    rows = c["counts2d"][c["pos"]]
    impact = c["a_impact"][win]
    ccls = c["cred_lut"][impact]
    tcls = c["tool_lut"][impact]
    zero = np.zeros(len(win), dtype=np.int32)
    n_agents = rows[:, 1] if len(win) else zero
    n_creds = np.where(ccls == 2, rows[:, 2], np.where(ccls == 1, rows[:, 3], zero))
    n_tools = np.where(tcls == 2, rows[:, 4], np.where(tcls == 1, rows[:, 5], zero))
    flags = np.where(c["a_kev"][win] != 0, 2, 0).astype(np.uint8)
    reach = (c["dist"][c["pkg_nodes"]] != UNVISITED).astype(np.int8)
    scores = cpu_ref.risk_score(
        c["a_sev"][win], n_agents.astype(np.uint32), n_creds.astype(np.uint32),
        n_tools.astype(np.uint32), flags, c["a_epss"][win],
        np.full(len(win), -1.0, dtype=np.float32), reach)
    return (scores, n_agents.astype(np.int32), n_creds.astype(np.int32),
            n_tools.astype(np.int32))


# ── rank ────────────────────────────────────────────────────────────────────

def rank_oracle(scores_cpu):
    """The quantized key sort that rank.hip replaces: bucket asc (score
    desc, 0.01 steps, round-half-even, clamped to 0..10), index asc."""
    import torch

    n = scores_cpu.numel()
    q = (scores_cpu * 100).round().clamp(0, 1000).to(torch.int64)
    bits = max(1, (n - 1).bit_length())
    key = ((1000 - q) << bits) | torch.arange(n)
    skey, _ = torch.sort(key)
    return skey & ((1 << bits) - 1)


def half_scores() -> np.ndarray:
    """Every f32 s in [0, 10] with s * 100 == k + 0.5 exactly in f32, found
    by rounding (k + 0.5) / 100 to f32 and keeping the hits, plus their two
    f32 neighbours."""
    k = np.arange(1000, dtype=np.float64)
    s = ((k + 0.5) / 100.0).astype(np.float32)
    hit = (s * np.float32(100.0)) == (k + 0.5).astype(np.float32)
    s = s[hit]
    return np.concatenate([s, np.nextafter(s, np.float32(-1)), np.nextafter(s, np.float32(11))])


@lru_cache(maxsize=None)
def rounding_scores() -> np.ndarray:
    """k / 100 for k = 0..1000, the exact halves, and the ends of the clamp.
    No NaN: the oracle's NaN -> int64 conversion is undefined."""
    grid = (np.arange(1001, dtype=np.float64) / 100.0).astype(np.float32)
    ten = np.float32(10.0)
    ends = np.array([-0.0, 0.0, np.inf, -np.inf, ten, np.nextafter(ten, np.float32(np.inf)),
                     np.nextafter(ten, np.float32(0)), -1e-3, 0.005, 0.015, 0.025, 1e30],
                    dtype=np.float32)
    out = np.concatenate([grid, half_scores(), ends])
    rng = np.random.default_rng(5)
    return out[rng.permutation(len(out))]


def bins_to_scores(bins) -> np.ndarray:
    """A score in the middle of each bin (bin = 1000 - round(score * 100))."""
    return ((1000 - np.asarray(bins, dtype=np.int64)) / 100.0).astype(np.float32)
