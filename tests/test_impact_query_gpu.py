"""``native.impact_query`` (ops/csrc/query.hip) against ``cpu_ref.impact_query``
on the cases of impact_query_cases.py: the edge-type mask, the hop bound, the
three caps at their edges, a reused output tuple, and batches in which one
block serves two queries.  One checker (``check_case``) judges every query;
it is told which queries may be truncated and skips none.
test_impact_query_cpu.py proves, from the oracle alone, that the queries
compared exactly cannot truncate."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import impact_query_cases as iq
from impact_query_cases import check_case

from agentbom_amd.ops import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


_DEVICE_GRAPHS: dict = {}


def _on_device(graph, dev):
    g = _DEVICE_GRAPHS.get(id(graph))
    if g is None:
        g = _DEVICE_GRAPHS[id(graph)] = {
            "keep": graph,
            "row_off": torch.from_numpy(graph.row_off).to(dev),
            "col": torch.from_numpy(graph.col).to(dev),
            "etype": None if graph.etype is None else torch.from_numpy(graph.etype).to(dev),
        }
    return g


def _run(case, dev, out=None):
    g = _on_device(case.graph, dev)
    q = torch.from_numpy(case.sources.astype(np.int32)).to(dev)
    return native.impact_query(
        g["row_off"], g["col"], q, etype=g["etype"] if case.masked else None,
        allowed_mask=case.mask, max_hops=case.max_hops, max_nodes=case.max_nodes, out=out)


def _host(out, width=None):
    nodes, hops, counts, trunc = out
    counts = counts.cpu().numpy()
    width = int(counts.max(initial=1)) if width is None else width
    return (nodes[:, :width].cpu().numpy(), hops[:, :width].cpu().numpy(),
            counts, trunc.cpu().numpy())


def _check(case, dev):
    out = _run(case, dev)
    assert out[0].shape == out[1].shape == (len(case.sources), case.max_nodes)
    check_case(case, *_host(out))


@pytest.mark.parametrize("case", iq.mask_cases(), ids=lambda c: c.name)
def test_edge_type_mask(case, dev):
    """Masks 0b111, 0b101, 0b010 and 0 with etype; mask 0 without etype is
    ignored.  16 sources, one without out-edges, one with only a self-loop."""
    _check(case, dev)
    if case.masked and case.mask == 0:
        _nodes, _hops, counts, trunc = _host(_run(case, dev))
        assert counts.tolist() == [1] * 16 and not trunc.any()


@pytest.mark.parametrize("case", iq.hop_cases(), ids=lambda c: c.name)
def test_hop_bound(case, dev):
    """max_hops 0 and 1, and hop 255 at the end of a 300-node chain."""
    _check(case, dev)
    if case.max_hops == 255:
        nodes, hops, counts, _trunc = _host(_run(case, dev))
        assert counts[0] == 256
        assert sorted(hops[0, :256].tolist()) == list(range(256))


def test_max_hops_above_255_is_refused(dev):
    case = iq.hop_cases()[2]
    g = _on_device(case.graph, dev)
    q = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="max_hops"):
        native.impact_query(g["row_off"], g["col"], q, max_hops=256, max_nodes=512)


@pytest.mark.parametrize("case", iq.max_nodes_cases(), ids=lambda c: c.name)
def test_max_nodes_edges(case, dev):
    """max_nodes at the neighbourhood size (exact), one below it (flag,
    count = max_nodes) and 1 (flag iff a neighbour other than the source)."""
    _check(case, dev)


def test_reused_output_is_rewritten(dev):
    """A large neighbourhood, then a source without out-edges into the same
    preallocated tuple: count and flag of the first call must not survive
    (the hipGraph replay path relies on that)."""
    g = iq.random_graph()
    size = iq.max_nodes_cases()[0].max_nodes
    big = iq.Case("reuse, truncating", g, np.array([iq.CAP_SOURCE]), 4, size - 1,
                  np.ones(1, dtype=np.uint8), expected_count={0: size - 1})
    small = iq.Case("reuse, sink", g, np.array([iq.RAND_SINK]), 4, size - 1,
                    np.zeros(1, dtype=np.uint8))
    out = (torch.empty((1, size - 1), dtype=torch.int32, device=dev),
           torch.empty((1, size - 1), dtype=torch.uint8, device=dev),
           torch.zeros(1, dtype=torch.int32, device=dev),
           torch.zeros(1, dtype=torch.uint8, device=dev))
    first = _run(big, dev, out=out)
    assert all(a is b for a, b in zip(first, out))
    check_case(big, *_host(first))
    second = _run(small, dev, out=out)
    assert all(a is b for a, b in zip(second, out))
    _nodes, _hops, counts, trunc = _host(second)
    assert counts.tolist() == [1] and trunc.tolist() == [0]
    check_case(small, *_host(second))


@pytest.mark.parametrize("case", iq.frontier_cases(), ids=lambda c: c.name)
def test_frontier_cap(case, dev):
    """2048 new nodes in a level fit; the 2049th is reported, not expanded."""
    _check(case, dev)


def test_probe_limit(dev):
    """64 probes, wrapping past slot 8191: 64 colliding neighbours fit beside
    a source elsewhere, the 65th is dropped; with the source in the chain's
    slot 63 fit and the 64th is dropped."""
    (case,) = iq.probe_cases()
    _check(case, dev)


@pytest.mark.parametrize("case", iq.batch_cases(), ids=lambda c: c.name)
def test_two_queries_per_block(case, dev):
    """2048 + 37 queries on a grid capped at 2048: the hash, the frontier
    sizes, the cursor and the flag are reset between the queries of a block."""
    _check(case, dev)


def test_source_stays_in_the_visited_set(dev):
    """2048 blocks, each with a self-looping source whose hash slot the last
    wave clears last: the seed must come after the whole clear, or the
    self-loop reports the source twice."""
    (case,) = iq.seed_cases()
    _check(case, dev)


def test_empty_batch(dev):
    g = _on_device(iq.random_graph(), dev)
    q = torch.empty(0, dtype=torch.int32, device=dev)
    nodes, hops, counts, trunc = native.impact_query(g["row_off"], g["col"], q, max_nodes=16)
    torch.cuda.synchronize()
    assert nodes.shape == hops.shape == (0, 16)
    assert counts.numel() == 0 and trunc.numel() == 0


def test_engine_cpu_and_gpu_paths(dev):
    """EstateEngine.blast_radius_query on the CPU and on the GPU engine, 16
    queries that cannot truncate, both against the unbounded oracle."""
    from agentbom_amd.graph.gpu_engine import EstateEngine

    est = iq.engine_estate()
    cpu = EstateEngine(est, device="cpu")
    gpu = EstateEngine(est, device=dev)
    case = iq.engine_case(cpu.rev["row_off"].numpy(), cpu.rev["col"].numpy())
    assert np.array_equal(gpu.rev["row_off"].cpu().numpy(), case.graph.row_off)
    assert np.array_equal(gpu.rev["col"].cpu().numpy(), case.graph.col)
    q = torch.from_numpy(case.sources)
    for eng, queries in ((cpu, q), (gpu, q.to(dev))):
        out = eng.blast_radius_query(queries, max_hops=case.max_hops,
                                     max_nodes=case.max_nodes)
        nodes, hops, counts, trunc = _host(out)
        assert not trunc.any()
        check_case(case, nodes, hops, counts, trunc)
