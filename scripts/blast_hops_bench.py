#!/usr/bin/env python
"""Timing driver for the multi-hop delegation kernels (profiles/blast_hops.md).

EstateEngine.transitive_blast() given a step result, at ``max_depth`` 2, 3 and
5, on the resident estate at the bench.py default size: a warm-up, then
``--repeats`` timed calls each, host clock around a device synchronise; min /
median / max are printed with the share of the unique matched packages that
pass A finished, that were queued for the wave pass and that overflowed an LDS
cap into the exact join.  ``step()`` and ``step(blast_depth=1)`` are timed the
same way, interleaved, and ``cpu_ref.blast_hops`` runs once per depth on a
seeded subsample of the same packages, against which the device result is
also compared.

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


def _summary(times, repeats: int) -> dict:
    times = sorted(times)
    return {"min_ms": round(1e3 * times[0], 4),
            "median_ms": round(1e3 * statistics.median(times), 4),
            "max_ms": round(1e3 * times[-1], 4), "repeats": repeats}


def _spread(fn, repeats: int) -> dict:
    fn()  # warm-up: code objects, allocator
    return _summary([_timed(fn)[1] for _ in range(repeats)], repeats)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--packages", type=int, default=10_000_000)
    ap.add_argument("--agents", type=int, default=100_000)
    ap.add_argument("--servers", type=int, default=500_000)
    ap.add_argument("--name-catalog", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--oracle-sample", type=int, default=2000,
                    help="unique packages cpu_ref.blast_hops runs on (0 = skip)")
    args = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("blast_hops_bench needs a GPU")
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.ops import cpu_ref
    from agentbom_amd.scan.synth import ET_CONTAINS, ET_HAS_CRED, ET_USES, generate_estate

    est = generate_estate(n_agents=args.agents, n_servers=args.servers,
                          n_packages=args.packages, name_catalog=args.name_catalog,
                          seed=args.seed)
    eng = EstateEngine(est, device="cuda:0")

    # step() beside step(blast_depth=1): the same path, interleaved
    for _ in range(3):
        eng.step()
        eng.step(blast_depth=1)
    plain, one = [], []
    for _ in range(args.repeats):
        plain.append(_timed(eng.step)[1])
        one.append(_timed(lambda: eng.step(blast_depth=1))[1])
    print(json.dumps(dict({"measurement": "engine_step"}, **_summary(plain, args.repeats))),
          flush=True)
    print(json.dumps(dict({"measurement": "engine_step_blast_depth_1"},
                          **_summary(one, args.repeats))), flush=True)

    step = eng.step()
    host = None
    for depth in (2, 3, 5):
        timing = _spread(lambda: eng.transitive_blast(step, max_depth=depth), args.repeats)
        blast = eng.transitive_blast(step, max_depth=depth)
        n = int(blast["uniq_pkgs"].numel())
        queued, overflow = eng._hops_ws["hops_queued"], eng._hops_ws["hops_overflow"]
        row = {"measurement": f"engine_transitive_blast_depth_{depth}",
               "findings": step["n_findings"], "unique_packages": n,
               "finished_in_pass_a": n - queued, "queued": queued, "overflowed": overflow,
               "pass_a_share": round((n - queued) / max(n, 1), 4),
               "queued_share": round(queued / max(n, 1), 4),
               "overflow_share": round(overflow / max(n, 1), 4),
               "hop_depth_histogram": torch.bincount(
                   blast["hop_depth"].to(torch.int64), minlength=6).tolist(),
               "max_transitive_agents": int(blast["t_agents"].max()) if n else 0,
               "max_transitive_creds": int(blast["t_creds"].max()) if n else 0}
        row.update(timing)
        step_timing = _spread(lambda: eng.step(blast_depth=depth), max(3, args.repeats // 4))
        row["step_with_depth_median_ms"] = step_timing["median_ms"]
        if args.oracle_sample:
            if host is None:
                host = {k: eng.rev[k].cpu().numpy() for k in ("row_off", "col", "etype")}
                host.update({"f_" + k: eng.fwd[k].cpu().numpy()
                             for k in ("row_off", "col", "etype")})
            rng = np.random.default_rng(args.seed)
            pick = np.sort(rng.choice(n, min(n, args.oracle_sample), replace=False))
            uniq = blast["uniq_pkgs"].cpu().numpy()[pick]
            t0 = time.perf_counter()
            hop, creds, hop_depth = cpu_ref.blast_hops(
                uniq, host["row_off"], host["col"], host["etype"], ET_CONTAINS, ET_USES,
                ET_HAS_CRED, host["f_row_off"], host["f_col"], host["f_etype"], depth)
            row["cpu_ref_sample"] = int(len(pick))
            row["cpu_ref_s"] = round(time.perf_counter() - t0, 3)
            row["equal_to_cpu_ref"] = bool(
                (blast["hop_agents"].cpu().numpy()[pick] == hop).all()
                and (blast["t_creds"].cpu().numpy()[pick] == creds).all()
                and (blast["hop_depth"].cpu().numpy()[pick] == hop_depth).all())
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
