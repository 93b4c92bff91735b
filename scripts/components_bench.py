#!/usr/bin/env python
"""Timing driver for the component kernels (profiles/components.md).

EstateEngine.components() under the lateral mask and over every edge, and
EstateEngine.lateral_domains() given a step result, on the resident estate at
the bench.py default size (the estate of profiles/centrality.md): a warm-up,
then ``--repeats`` timed calls each, host clock around a device synchronise;
min / median / max are printed.  The rounds run, the bytes a round must move
and the achieved rate come with the component timings, and one run of the
numpy oracle on the same input for comparison.

Prints one JSON line per measurement.  Needs a GPU; never falls back.
"""

from __future__ import annotations

import argparse
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


def _spread(fn, repeats: int) -> dict:
    fn()  # warm-up: code objects, allocator
    times = sorted(_timed(fn)[1] for _ in range(repeats))
    return {"min_ms": round(1e3 * times[0], 4),
            "median_ms": round(1e3 * statistics.median(times), 4),
            "max_ms": round(1e3 * times[-1], 4), "repeats": repeats}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--packages", type=int, default=10_000_000)
    ap.add_argument("--agents", type=int, default=100_000)
    ap.add_argument("--servers", type=int, default=500_000)
    ap.add_argument("--name-catalog", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip-oracle", action="store_true",
                    help="leave out the numpy oracle runs (slow at full size)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("components_bench needs a GPU")
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.ops import cpu_ref
    from agentbom_amd.scan.synth import ET_HAS_CRED, ET_USES, generate_estate

    est = generate_estate(n_agents=args.agents, n_servers=args.servers,
                          n_packages=args.packages, name_catalog=args.name_catalog,
                          seed=args.seed)
    eng = EstateEngine(est, device="cuda:0")
    n, e = eng.N, int(eng.fwd["col"].numel())
    lateral = (1 << ET_USES) | (1 << ET_HAS_CRED)
    src, col, et = (eng.fwd[k].cpu().numpy() for k in ("src", "col", "etype"))

    for what, mask in (("lateral", lateral), ("all_edges", None)):
        timing = _spread(lambda: eng.components(mask), args.repeats)
        labels = eng.components(mask)
        rounds = int(eng._centrality_ws()["cc_rounds"])
        kept = e if mask is None else int(((mask >> eng.fwd["etype"].to(torch.int64)) & 1).sum())
        # hook: both endpoint ids of every edge (+ its type byte under a mask)
        # and two parent gathers per kept edge; compress (after every round
        # but the confirming one): parent and parent-of-parent per node; the
        # init pass writes the N labels once
        hook_bytes = e * (8 + (mask is not None)) + 8 * kept
        compress_bytes = 8 * n
        total = 4 * n + rounds * hook_bytes + (rounds - 1) * compress_bytes
        row = {"measurement": f"engine_components_{what}", "nodes": n, "edges": e,
               "edges_kept": kept, "rounds": rounds,
               "components": int(torch.unique(labels).numel()),
               "hook_bytes_per_round": hook_bytes, "compress_bytes_per_round": compress_bytes,
               "model_bytes": total,
               "model_gb_per_s": round(total / (timing["median_ms"] * 1e-3) / 1e9, 1)}
        row.update(timing)
        if not args.skip_oracle:
            t0 = time.perf_counter()
            want = cpu_ref.connected_components(
                src, col, n, etype=et if mask is not None else None,
                allowed_mask=mask if mask is not None else 0xFFFFFFFF)
            row["cpu_ref_s"] = round(time.perf_counter() - t0, 3)
            row["equal_to_cpu_ref"] = bool((labels.cpu().numpy() == want).all())
        print(json.dumps(row), flush=True)

    step = eng.step()
    timing = _spread(lambda: eng.lateral_domains(step), max(3, args.repeats // 4))
    dom = eng.lateral_domains(step)
    row = {"measurement": "engine_lateral_domains", "nodes": n, "edges": e,
           "n_domains": dom["n_domains"], "largest_agents": dom["largest_agents"],
           "top_findings": dom["findings"][:3].tolist()}
    row.update(timing)
    print(json.dumps(row), flush=True)
    # the part of lateral_domains that is not the labelling or the roll-up of
    # findings to servers: renumbering plus abom_component_stats
    roll = _spread(lambda: eng.rollup(step), max(3, args.repeats // 4))
    print(json.dumps(dict({"measurement": "engine_rollup_alone"}, **roll)), flush=True)


if __name__ == "__main__":
    main()
