"""row_of, the package -> unique-row map of the dedup layout (CPU torch):
the inverse of perm2/run_off that ops/csrc/findings.hip reads."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from agentbom_amd.graph.gpu_engine import row_of_from_runs


def _random_layout(rng, P, U):
    row_of_pkg = torch.from_numpy(rng.integers(0, U, P)).to(torch.int64)
    perm2 = torch.argsort(row_of_pkg, stable=True)
    counts = torch.bincount(row_of_pkg[perm2], minlength=U)
    run_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    return run_off, perm2, row_of_pkg


@pytest.mark.parametrize("seed,P,U", [(0, 500, 60), (1, 500, 60), (2, 64, 200), (3, 1, 1)])
def test_row_of_inverts_the_runs(seed, P, U):
    run_off, perm2, row_of_pkg = _random_layout(np.random.default_rng(seed), P, U)
    row_of = row_of_from_runs(torch, run_off, perm2)
    assert row_of.dtype == torch.int32 and row_of.shape == (P,)
    for r in range(U):
        for k in range(int(run_off[r]), int(run_off[r + 1])):
            assert int(row_of[perm2[k]]) == r
    assert torch.equal(row_of.to(torch.int64), row_of_pkg)


def test_row_of_in_the_engine_layout():
    """build_dedup_match_layout carries row_of for the real estate layout."""
    from agentbom_amd.graph.gpu_engine import build_dedup_match_layout
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=50, n_servers=200, n_packages=5000,
                          name_catalog=800, seed=3, arena_windows=1600)
    arena = est.arena.to_torch(torch.device("cpu"))
    cols = [torch.from_numpy(a.view(np.int64)) for a in
            (est.pkg_name_id, est.pkg_key_hi, est.pkg_key_lo)]
    layout = build_dedup_match_layout(torch, arena, *cols, torch.from_numpy(est.pkg_flags))
    assert layout is not None
    run_off, perm2, row_of = layout["run_off"], layout["perm2"], layout["row_of"]
    rows = torch.repeat_interleave(torch.arange(run_off.numel() - 1), run_off[1:] - run_off[:-1])
    assert torch.equal(row_of[perm2].to(torch.int64), rows)
