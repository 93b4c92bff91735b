#!/usr/bin/env python
"""Timing driver for the per-source reach kernels (profiles/reach_sets.md).

``EstateEngine.agent_reach`` on the resident estate at the bench.py default
size, targets = the unique matched packages of one step, for each source count
of ``--sources``: a warm-up, then ``--repeats`` timed calls, host clock around
a device synchronise; min / median / max are printed with the words per node,
the passes and the levels of the call.  The yardstick is the only way to the
same matrix without these kernels: one single-source ``native.bfs`` per agent
plus a gather of the targets' distances into the agent's column; it is timed
the same way (fewer repeats at the larger counts) and its matrix is compared
with ``agent_reach``'s, cell for cell.

``--variant PATH`` names a second build of the library (for instance one
compiled with ``-DABOM_REACH_HEAVY_DEG=2147483647``, which never takes the
wave-per-row expand): every ``agent_reach`` timing is then taken with both
builds, alternating, and a star graph (``--star-leaves`` leaves under one hub,
64 sources on the hub) is timed with both too.

Prints one JSON line per measurement.  Needs a GPU; never falls back.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _summary(times) -> dict:
    times = sorted(times)
    return {"min_ms": round(1e3 * times[0], 4),
            "median_ms": round(1e3 * statistics.median(times), 4),
            "max_ms": round(1e3 * times[-1], 4), "repeats": len(times)}


def _load_variant(native, path: str):
    lib = ctypes.CDLL(path)
    for name, (argtypes, restype) in native._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    return lib


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--packages", type=int, default=10_000_000)
    ap.add_argument("--agents", type=int, default=100_000)
    ap.add_argument("--servers", type=int, default=500_000)
    ap.add_argument("--name-catalog", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sources", type=int, nargs="+", default=[64, 128, 256, 512, 1024])
    ap.add_argument("--yardstick-repeats", type=int, default=3)
    ap.add_argument("--variant", default=None, help="a second _abom_gpu.so to alternate with")
    ap.add_argument("--star-leaves", type=int, default=1_000_000)
    args = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("reach_sets_bench needs a GPU")
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.ops import native
    from agentbom_amd.scan.synth import (
        ET_CONTAINS, ET_HAS_CRED, ET_PROVIDES_TOOL, ET_USES, generate_estate,
    )

    builds = {"default": native.load()}
    if args.variant:
        builds["variant"] = _load_variant(native, args.variant)

    est = generate_estate(n_agents=args.agents, n_servers=args.servers,
                          n_packages=args.packages, name_catalog=args.name_catalog,
                          seed=args.seed)
    eng = EstateEngine(est, device="cuda:0")
    res = eng.step()
    targets = torch.unique_consecutive(res["pkg_idx"] + est.pkg_base).to(torch.int32)
    deg = (eng.fwd["row_off"][1:est.n_agents + 1] - eng.fwd["row_off"][:est.n_agents]).cpu().numpy()
    # the widest agents first (the heavy rows), then a seeded draw of the rest
    order = np.argsort(-deg, kind="stable")
    rest = np.random.default_rng(args.seed).permutation(order[8:])
    pool = np.concatenate([order[:8], rest]).astype(np.int32) + est.agent_base
    print(json.dumps({"what": "estate", "nodes": int(eng.N), "edges": int(eng.fwd["col"].numel()),
                      "targets": int(targets.numel()), "agent_degree_median": float(np.median(deg)),
                      "agent_degree_max": int(deg.max()),
                      "agents_at_heavy_degree": int((deg >= 64).sum())}), flush=True)
    mask = (1 << ET_USES) | (1 << ET_CONTAINS) | (1 << ET_HAS_CRED) | (1 << ET_PROVIDES_TOOL)

    for count in args.sources:
        agents = torch.from_numpy(pool[:count]).to("cuda:0")
        for name, lib in builds.items():  # warm-up of every build
            native._lib = lib
            out = eng.agent_reach(agents, targets=targets)
        times = {name: [] for name in builds}
        for _ in range(args.repeats):
            for name, lib in builds.items():
                native._lib = lib
                times[name].append(_timed(lambda: eng.agent_reach(agents, targets=targets))[1])
        native._lib = builds["default"]
        ws = eng._reach_ws
        for name in builds:
            s = _summary(times[name])
            print(json.dumps({"what": "agent_reach", "build": name, "sources": count,
                              "passes": ws["passes"], "levels": ws["levels"],
                              "words_first_pass": min(4, (count + 63) // 64),
                              "ms_per_pass": round(s["median_ms"] / ws["passes"], 4),
                              "reached_cells": int((out["hops"] != 255).sum()), **s}),
                  flush=True)

        # yardstick: one single-source BFS per agent, the targets gathered per column
        bfs_ws: dict = {}
        t64 = targets.to(torch.int64)

        def per_agent_bfs():
            cols = torch.empty((targets.numel(), count), dtype=torch.uint8, device="cuda:0")
            for j in range(count):
                dist = native.bfs(eng.fwd["row_off"], eng.fwd["col"], agents[j:j + 1], eng.N,
                                  etype=eng.fwd["etype"], allowed_mask=mask, max_levels=16,
                                  workspace=bfs_ws)
                cols[:, j] = dist[t64].clamp(min=-1, max=255).to(torch.uint8)
            return cols

        want = per_agent_bfs()  # warm-up; UNVISITED (-1 as int32) becomes 255
        reps = args.repeats if count <= 64 else args.yardstick_repeats
        y = _summary([_timed(per_agent_bfs)[1] for _ in range(reps)])
        same = bool(torch.equal(want, out["hops"]))
        print(json.dumps({"what": "per_agent_bfs", "sources": count, "equal_to_agent_reach": same,
                          **y}), flush=True)
        if not same:
            sys.exit("agent_reach differs from the per-agent BFS")

    if args.variant:
        n = args.star_leaves + 1
        row_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
        row_off[1:] = args.star_leaves
        col = torch.arange(1, n, dtype=torch.int32, device="cuda:0")
        hub = torch.zeros(64, dtype=torch.int32, device="cuda:0")
        leaves = torch.arange(1, n, dtype=torch.int32, device="cuda:0")
        ws = {}
        times = {name: [] for name in builds}
        for rep in range(args.repeats + 1):
            for name, lib in builds.items():
                native._lib = lib
                hops, t = _timed(lambda: native.reach_hops(row_off, col, hub, leaves, n,
                                                           max_depth=16, workspace=ws))
                if rep:
                    times[name].append(t)
                assert int((hops != 1).sum()) == 0
        native._lib = builds["default"]
        for name in builds:
            print(json.dumps({"what": "star", "build": name, "leaves": args.star_leaves,
                              "sources": 64, **_summary(times[name])}), flush=True)


if __name__ == "__main__":
    main()
