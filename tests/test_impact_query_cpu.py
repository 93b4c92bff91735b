"""Preconditions of the impact-query cases (impact_query_cases.py), from the
oracle alone: which queries the kernel may not truncate, which it must, the
hash-slot facts of the probe-limit case, and the checker itself.  No GPU."""

from __future__ import annotations

import numpy as np
import pytest

import impact_query_cases as iq
from impact_query_cases import (
    IQ_FRONTIER,
    IQ_HASH,
    IQ_PROBES,
    check_case,
    check_query,
    fits,
    max_probes,
    slot,
)


def _all_cases():
    return (iq.mask_cases() + iq.hop_cases() + iq.max_nodes_cases()
            + iq.frontier_cases() + iq.probe_cases() + iq.batch_cases() + iq.seed_cases())


def _oracle_output(case):
    """The oracle's answer in the kernel's output layout (exact queries only;
    a truncating query gets an empty row)."""
    q = len(case.sources)
    width = max(len(o) for o in case.oracle)
    nodes = np.zeros((q, width), dtype=np.int32)
    hops = np.zeros((q, width), dtype=np.uint8)
    counts = np.zeros(q, dtype=np.int32)
    for i in case.exact():
        items = list(case.oracle[i].items())
        nodes[i, :len(items)] = [n for n, _ in items]
        hops[i, :len(items)] = [h for _, h in items]
        counts[i] = len(items)
    return nodes, hops, counts


def test_slot_is_a_bijection_below_8192():
    s = slot(np.arange(IQ_HASH))
    assert s.dtype == np.uint32
    assert np.array_equal(np.sort(s), np.arange(IQ_HASH))
    assert np.all(slot(np.arange(IQ_HASH) + 5 * IQ_HASH) == s)
    # the multiply wraps in uint32, as on the device
    assert int(slot(3_000_000_000)[0]) == (3_000_000_000 * 2654435761) % (1 << 32) % IQ_HASH


def test_max_probes_bound():
    assert max_probes([5]) == 1
    assert max_probes(range(100)) == 1
    same = [7 + IQ_HASH * k for k in range(10)]
    assert max_probes(same) == 10
    # a neighbour one slot down the chain lengthens it for the home slot
    nxt = int(np.flatnonzero(slot(np.arange(IQ_HASH)) == slot(7)[0] + 1)[0])
    assert max_probes(same + [nxt]) == 11


@pytest.mark.parametrize("case", _all_cases(), ids=lambda c: c.name)
def test_exact_queries_cannot_truncate(case):
    """Every query a case compares exactly fits all three caps; every query
    it expects truncated misses at least one."""
    seen = {}   # queries of one source share one oracle dict
    for q, hops in enumerate(case.oracle):
        assert int(case.sources[q]) in hops and hops[int(case.sources[q])] == 0
        if id(hops) not in seen:
            seen[id(hops)] = fits(hops, case.max_nodes)
        assert seen[id(hops)] == (case.expected_trunc[q] == 0), f"{case.name} query {q}"
        assert max(hops.values()) <= case.max_hops


def test_share_of_exact_queries():
    """Cases 1-4 compare every query exactly; 5 and 6 each have their "fits"
    halves; case 7 truncates only the 37 star queries."""
    for case in iq.mask_cases() + iq.hop_cases():
        assert len(case.exact()) == len(case.sources) == len(case.oracle)
    assert [len(c.exact()) for c in iq.max_nodes_cases()] == [1, 0, 2]
    assert [len(c.exact()) for c in iq.frontier_cases()] == [1, 0, 0]
    assert iq.probe_cases()[0].exact().tolist() == [0, 2]
    for case in iq.batch_cases():
        assert len(case.sources) == iq.BATCH_Q == iq.IQ_GRID + 37
        assert len(case.exact()) == iq.IQ_GRID
    first, second = iq.batch_cases()
    # q and q + 2048 share a block: star before isolated, then the reverse
    assert np.all(first.sources[:37] == iq.BATCH_STAR)
    assert np.all(first.sources[iq.IQ_GRID:] >= iq.BATCH_ISOLATED)
    assert np.all(second.sources[:37] >= iq.BATCH_ISOLATED)
    assert np.all(second.sources[iq.IQ_GRID:] == iq.BATCH_STAR)
    for q in range(iq.IQ_GRID, iq.BATCH_Q):
        assert first.oracle[q] == {int(first.sources[q]): 0}


def test_mask_case_graph():
    g = iq.random_graph()
    assert g.n == 1000 and 5800 <= len(g.col) <= 6200
    pairs = g.src * g.n + g.dst
    assert len(np.unique(pairs)) < len(pairs), "no parallel edges"
    assert np.any((g.src == g.dst) & (g.src != iq.RAND_SELF)), "no self-loops"
    assert g.row_off[iq.RAND_SINK + 1] == g.row_off[iq.RAND_SINK]
    row = g.col[g.row_off[iq.RAND_SELF]:g.row_off[iq.RAND_SELF + 1]]
    assert row.tolist() == [iq.RAND_SELF]
    assert sorted(set(g.etype.tolist())) == [0, 1, 2]
    full, m101, m010, none, ignored = iq.mask_cases()
    assert full.oracle[0][1] == 1 and full.oracle[0][2] == 2   # the cycle 0 -> 1 -> 2 -> 0
    for q in range(16):
        assert none.oracle[q] == {int(none.sources[q]): 0}
        assert ignored.oracle[q] == full.oracle[q]
        assert set(m101.oracle[q]) <= set(full.oracle[q])
        assert set(m010.oracle[q]) <= set(full.oracle[q])
    # the masks cut real edges, and differently
    assert len(m101.oracle[3]) < len(full.oracle[3])
    assert m010.oracle[3] != m101.oracle[3]
    # masked-out types equal deleted edges
    keep = (np.arange(len(g.src)) % 3) != 1
    cut = iq.Graph(g.src[keep], g.dst[keep], g.n)
    assert cut.oracle(iq.RAND_SOURCES, masked=False, mask=0, max_hops=4) == m101.oracle


def test_hop_cases():
    zero, one, chain = iq.hop_cases()
    g = iq.random_graph()
    for q, s in enumerate(iq.RAND_SOURCES.tolist()):
        assert zero.oracle[q] == {s: 0}
        nbrs = set(g.col[g.row_off[s]:g.row_off[s + 1]].tolist()) - {s}
        assert one.oracle[q] == {s: 0, **{v: 1 for v in nbrs}}
    assert chain.oracle[0] == {v: v for v in range(256)}
    assert chain.oracle[1] == {44 + v: v for v in range(256)}
    assert chain.oracle[2] == {iq.CHAIN_N - 1: 0}


def test_max_hops_above_255_is_refused():
    """out_hops is uint8: native.impact_query refuses what would wrap,
    before it loads the library or touches a tensor."""
    import torch

    from agentbom_amd.ops import native

    g = iq.hop_cases()[2].graph
    args = (torch.from_numpy(g.row_off), torch.from_numpy(g.col),
            torch.zeros(1, dtype=torch.int32))
    for bad in (256, 1000):
        with pytest.raises(ValueError, match="max_hops"):
            native.impact_query(*args, max_hops=bad)


def test_max_nodes_cases():
    at, below, one = iq.max_nodes_cases()
    size = len(at.oracle[0])
    assert 64 < size <= IQ_FRONTIER
    assert (at.max_nodes, below.max_nodes, one.max_nodes) == (size, size - 1, 1)
    g = iq.random_graph()
    for q, s in enumerate(one.sources.tolist()):
        other = set(g.col[g.row_off[s]:g.row_off[s + 1]].tolist()) - {s}
        assert bool(other) == bool(one.expected_trunc[q])
    # source 0 has a self-loop as well as other neighbours
    assert 0 in g.col[g.row_off[0]:g.row_off[1]]


def test_frontier_cases():
    full, over, sink = iq.frontier_cases()
    for case in (full, over, sink):
        assert case.graph.n <= IQ_HASH and case.max_nodes == 8192
    levels = lambda c: np.bincount(list(c.oracle[0].values())).tolist()  # noqa: E731
    assert levels(full) == [1, IQ_FRONTIER, IQ_FRONTIER]
    assert levels(over) == [1, IQ_FRONTIER + 1, IQ_FRONTIER + 1]
    assert levels(sink) == [1, IQ_FRONTIER + 1, 1]
    assert over.expected_count[0] == 1 + 2049 + 2048
    assert sink.expected_count[0] == 1 + 2049 + 1
    assert sink.must_report[0][IQ_FRONTIER + 2] == 2


def test_probe_case_slots():
    """The slot facts of the probe-limit case, by the hash in numpy uint32."""
    (case,) = iq.probe_cases()
    home = int(slot(iq.PROBE_R)[0])
    assert home == iq.PROBE_HOME and IQ_HASH - 10 <= home <= IQ_HASH - 1
    assert np.all(slot(iq.probe_neighbours(65)) == home)
    chain = {(home + i) & (IQ_HASH - 1) for i in range(IQ_PROBES + 1)}
    assert 0 in chain and IQ_HASH - 1 in chain, "the chain does not wrap"
    free_fit, free_over, shared_fit, shared_over = case.sources.tolist()
    assert int(slot(free_fit)[0]) not in chain and int(slot(free_over)[0]) not in chain
    assert int(slot(shared_fit)[0]) == home and int(slot(shared_over)[0]) == home
    assert case.graph.n == 68 * IQ_HASH and case.graph.row_off.nbytes > 4_000_000
    assert [len(o) for o in case.oracle] == [65, 66, 64, 65]
    assert [max_probes(o) for o in case.oracle] == [64, 65, 64, 65]
    # one neighbour is dropped in each truncating half
    assert case.expected_count == {1: 65, 3: 64}


def test_engine_case_cannot_truncate():
    import torch

    from agentbom_amd.graph.gpu_engine import EstateEngine

    eng = EstateEngine(iq.engine_estate(), device="cpu")
    case = iq.engine_case(eng.rev["row_off"].numpy(), eng.rev["col"].numpy())
    assert all(fits(o, case.max_nodes) for o in case.oracle)
    assert max(len(o) for o in case.oracle) > 1
    out = eng.blast_radius_query(torch.from_numpy(case.sources),
                                 max_hops=case.max_hops, max_nodes=case.max_nodes)
    nodes, hops, counts, trunc = (t.numpy() for t in out)
    assert not trunc.any()
    check_case(case, nodes, hops, counts, trunc)


# ── the checker notices what it is there to notice ──────────────────────────

def _one(case, q=0):
    nodes, hops, counts = _oracle_output(case)
    return dict(nodes_row=nodes[q].copy(), hops_row=hops[q].copy(), count=int(counts[q]),
                trunc=0, source=int(case.sources[q]), oracle=case.oracle[q],
                max_hops=case.max_hops, max_nodes=case.max_nodes, expected_trunc=0)


def test_checker_accepts_the_oracle():
    for case in iq.mask_cases():
        nodes, hops, counts = _oracle_output(case)
        check_case(case, nodes, hops, counts, np.zeros(len(counts), dtype=np.uint8))


def test_checker_never_skips_a_flagged_query():
    """A kernel that flags every query truncated fails at once."""
    kw = _one(iq.mask_cases()[0])
    kw["trunc"] = 1
    with pytest.raises(AssertionError, match="truncated 1, expected 0"):
        check_query(**kw)


def test_checker_rejects_wrong_answers():
    base = _one(iq.mask_cases()[0])
    assert base["count"] > 10

    def broken(**change):
        kw = dict(base, nodes_row=base["nodes_row"].copy(), hops_row=base["hops_row"].copy())
        kw.update(change)
        return kw

    check_query(**base)
    with pytest.raises(AssertionError, match="count"):
        check_query(**broken(count=base["count"] - 1))
    kw = broken()
    kw["hops_row"][5] += 1
    with pytest.raises(AssertionError, match="differs"):
        check_query(**kw)
    kw = broken()
    kw["nodes_row"][5] = kw["nodes_row"][6]
    with pytest.raises(AssertionError, match="duplicate"):
        check_query(**kw)
    kw = broken()
    kw["nodes_row"][[0, 1]] = kw["nodes_row"][[1, 0]]
    with pytest.raises(AssertionError, match="entry 0"):
        check_query(**kw)
    with pytest.raises(AssertionError, match="count"):
        check_query(**broken(max_nodes=base["count"] - 1))
    # truncated: exact count, subset, hop bounds
    trunc = broken(trunc=1, expected_trunc=1, expected_count=base["count"])
    check_query(**trunc)
    with pytest.raises(AssertionError, match="derived"):
        check_query(**dict(trunc, expected_count=base["count"] + 1))
    with pytest.raises(AssertionError, match="derives"):
        check_query(**dict(trunc, expected_count=None))
    kw = dict(trunc, hops_row=base["hops_row"].copy())
    kw["hops_row"][5] = 0
    with pytest.raises(AssertionError, match="oracle"):
        check_query(**kw)
    kw = dict(trunc, nodes_row=base["nodes_row"].copy())
    kw["nodes_row"][5] = 5000
    with pytest.raises(AssertionError, match="outside"):
        check_query(**kw)
    with pytest.raises(AssertionError, match="not 1"):
        check_query(**dict(trunc, must_report={5000: 1}))
