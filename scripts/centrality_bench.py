#!/usr/bin/env python
"""Timing driver for the centrality kernels (profiles/centrality.md).

  backend  HipBackend against NativeBackend on a UnifiedGraph exported from a
           generated estate of about 20k nodes: wall time of
           betweenness(sample=64) and pagerank(), each once after a warm-up.
  engine   EstateEngine.betweenness(sample=64) and .pagerank() on the
           resident estate at the bench.py default size: ms per source, ms
           per iteration, and achieved bytes/s against the bytes the level
           passes must stream.

Prints one JSON line per measurement.  Needs a GPU; never falls back.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def _sync():
    import torch

    torch.cuda.synchronize()


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    out = fn()
    _sync()
    return out, time.perf_counter() - t0


def estate_to_unified(est):
    from agentbom_amd.graph.container import UnifiedEdge, UnifiedGraph, UnifiedNode
    from agentbom_amd.graph.types import EntityType, RelationshipType

    g = UnifiedGraph()
    for i in range(est.num_nodes):
        g.add_node(UnifiedNode(id=f"n{i:07d}", entity_type=EntityType.PACKAGE, label=str(i)))
    for u, v in zip(est.edge_src.tolist(), est.edge_dst.tolist()):
        g.add_edge(UnifiedEdge(f"n{u:07d}", f"n{v:07d}", RelationshipType.DEPENDS_ON))
    return g


def run_backend(args) -> None:
    from agentbom_amd.graph.backend import NativeBackend, get_backend
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=100, n_servers=600, n_packages=18_000,
                          name_catalog=5_000, seed=args.seed)
    g = estate_to_unified(est)
    hip = get_backend("hip")
    assert hip.name == "hip", "hip backend unavailable"
    hip.betweenness(g, sample=2)  # warm-up: code objects, allocator
    hip.pagerank(g, iterations=2)
    for what, call in (("betweenness_sample64", lambda b: b.betweenness(g, sample=64)),
                       ("pagerank", lambda b: b.pagerank(g))):
        got, hip_s = _timed(lambda: call(hip))
        want, native_s = _timed(lambda: call(NativeBackend()))
        worst = max(abs(got[k] - want[k]) for k in want)
        print(json.dumps({"measurement": f"backend_{what}", "nodes": g.node_count,
                          "edges": g.edge_count, "hip_s": round(hip_s, 6),
                          "native_s": round(native_s, 6),
                          "speedup": round(native_s / hip_s, 1),
                          "max_abs_diff": worst}), flush=True)


def run_engine(args) -> None:
    from agentbom_amd.graph.backend import brandes_sources
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=args.agents, n_servers=args.servers,
                          n_packages=args.packages, name_catalog=args.name_catalog,
                          seed=args.seed)
    eng = EstateEngine(est, device="cuda:0")
    n, e = eng.N, int(eng.fwd["col"].numel())
    eng.betweenness(sample=1)  # warm-up
    eng.pagerank(iterations=2)

    n_sources = len(brandes_sources(n, args.sample))
    _, bc_s = _timed(lambda: eng.betweenness(sample=args.sample))
    deepest = int(eng._centrality_ws()["bc_deepest"])
    # every level pass scans dist[N] and, for the rows it enters, their edges:
    # (deepest+1) forward and deepest backward passes per source; the sigma /
    # delta cells touched come on top and are not counted
    passes = 2 * deepest + 1
    bc_bytes = n_sources * passes * (4 * n + 4 * e)
    print(json.dumps({"measurement": "engine_betweenness", "nodes": n, "edges": e,
                      "sources": n_sources, "deepest_level": deepest,
                      "seconds": round(bc_s, 6),
                      "ms_per_source": round(1e3 * bc_s / n_sources, 4),
                      "model_bytes": bc_bytes,
                      "model_gb_per_s": round(bc_bytes / bc_s / 1e9, 1)}), flush=True)

    _, pr_s = _timed(lambda: eng.pagerank(iterations=args.iterations))
    iters = int(eng._centrality_ws()["pr_iterations"])  # it may stop early
    # per pass: row_off 8N + col 4E + contrib gathers 8E + rank/contrib in and out 32N
    pr_bytes = iters * (40 * n + 12 * e)
    print(json.dumps({"measurement": "engine_pagerank", "nodes": n, "edges": e,
                      "iterations_run": iters, "seconds": round(pr_s, 6),
                      "ms_per_iteration": round(1e3 * pr_s / iters, 4),
                      "model_bytes": pr_bytes,
                      "model_gb_per_s": round(pr_bytes / pr_s / 1e9, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["backend", "engine"])
    ap.add_argument("--packages", type=int, default=10_000_000)
    ap.add_argument("--agents", type=int, default=100_000)
    ap.add_argument("--servers", type=int, default=500_000)
    ap.add_argument("--name-catalog", type=int, default=1_000_000)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("centrality_bench needs a GPU")
    {"backend": run_backend, "engine": run_engine}[args.mode](args)


if __name__ == "__main__":
    main()
