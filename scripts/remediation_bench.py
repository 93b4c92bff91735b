#!/usr/bin/env python
"""Timing driver for the remediation plan (profiles/r12_remediation_plan.md).

One ``EstateEngine.step()`` on the resident estate at the bench.py default
size, then ``EstateEngine.remediation_plan(step, k=None)`` with the native arm
(ops/csrc/remediation.hip) and the torch arm (AGENT_BOM_REMEDIATION_NATIVE=0)
alternating: a warm-up of each, then ``--repeats`` timed calls of each, host
clock around a device synchronise.  Every array of the two plans is compared,
and the tier-2 queue length and pool rounds of the native arm are printed.
``--split`` adds the native arm's per-call split, each of its four entry
points timed with a synchronise behind it.

Prints one JSON line per measurement.  Needs a GPU; never falls back.
"""

from __future__ import annotations

import argparse
import json
import os
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


def _split(eng, step, repeats: int) -> dict:
    """Median ms of each native entry point, a synchronise behind each: the
    library calls of ``native.remediation_items`` wrapped one by one."""
    import torch

    from agentbom_amd.ops import native

    lib = native.load()
    names = ("abom_remediation_fold", "abom_remediation_gather", "abom_remediation_scatter",
             "abom_remediation_union")
    spent = {n: [] for n in names}
    originals = {n: getattr(lib, n) for n in names}

    def wrap(name):
        def call(*a):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = originals[name](*a)
            torch.cuda.synchronize()
            spent[name].append(time.perf_counter() - t0)
            return rc
        return call

    # ctypes function objects cannot be replaced on the CDLL: shadow them on
    # the instance for the length of the measurement
    for n in names:
        lib.__dict__[n] = wrap(n)
    try:
        for _ in range(repeats):
            eng.remediation_plan(step, k=None)
    finally:
        for n in names:
            lib.__dict__[n] = originals[n]
    return {n: round(1e3 * statistics.median(t), 4) for n, t in spent.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--packages", type=int, default=10_000_000)
    ap.add_argument("--agents", type=int, default=100_000)
    ap.add_argument("--servers", type=int, default=500_000)
    ap.add_argument("--name-catalog", type=int, default=1_000_000)
    ap.add_argument("--arena-windows", type=int, default=2_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--split", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("remediation_bench needs a GPU")
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.ops.cpu_ref import REMEDIATION_KEYS
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=args.agents, n_servers=args.servers,
                          n_packages=args.packages, name_catalog=args.name_catalog,
                          arena_windows=args.arena_windows, seed=args.seed)
    eng = EstateEngine(est, device="cuda:0")
    eng.step()
    step = eng.step()
    _, t_items = _timed(eng.remediation_items)

    def arm(native_on: bool):
        os.environ["AGENT_BOM_REMEDIATION_NATIVE"] = "1" if native_on else "0"
        return eng.remediation_plan(step, k=None)

    plans = {True: arm(True), False: arm(False)}  # warm-up: code objects, allocator
    times = {True: [], False: []}
    for _ in range(args.repeats):
        for native_on in (True, False):
            times[native_on].append(_timed(lambda: arm(native_on))[1])
    equal = all(torch.equal(plans[True][k], plans[False][k])
                for k in REMEDIATION_KEYS + ("agents_pct",))
    os.environ["AGENT_BOM_REMEDIATION_NATIVE"] = "1"
    plan = plans[True]
    shape = {"findings": step["n_findings"], "items": eng.remediation_items()[1],
             "matched_items": plan["n_items"],
             "matched_installs": int(plan["installs"].sum()),
             "max_installs": int(plan["installs"].max()) if plan["n_items"] else 0,
             "max_servers": int(plan["n_servers"].max()) if plan["n_items"] else 0,
             "max_agents": int(plan["n_agents"].max()) if plan["n_items"] else 0,
             "max_tools": int(plan["n_tools"].max()) if plan["n_items"] else 0,
             "item_index_build_ms": round(1e3 * t_items, 2)}
    print(json.dumps(dict({"measurement": "remediation_plan_native",
                           "tier2_queued": eng._remed_ws["remed_queued"],
                           "pool_rounds": eng._remed_ws["remed_rounds"],
                           "equal_to_torch_arm": equal}, **shape,
                          **_summary(times[True], args.repeats))), flush=True)
    print(json.dumps(dict({"measurement": "remediation_plan_torch"},
                          **_summary(times[False], args.repeats))), flush=True)
    if args.split:
        print(json.dumps(dict({"measurement": "remediation_native_split_ms"},
                              **_split(eng, step, args.repeats))), flush=True)
    if not equal:
        sys.exit("the native and the torch arm differ")


if __name__ == "__main__":
    main()
