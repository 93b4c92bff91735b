"""The multi-hop delegation expansion without a GPU: ``cpu_ref.blast_hops``
against hand-written results and against
``models.blast.expand_blast_radius_hops``, and the hop keys of the CPU
engine's ``step(blast_depth=k)``.  Every comparison is exact.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from blast_hops_graphs import (
    DEPTHS, ESTATE_ARGS, GRAPHS, HOP_KEYS, chain, cpu_args, expansion_counts, model_objects,
)

from agentbom_amd.graph.gpu_engine import EstateEngine
from agentbom_amd.models.blast import HOP_RISK_FACTORS
from agentbom_amd.ops import cpu_ref
from agentbom_amd.scan.synth import ET_CONTAINS, ET_HAS_CRED, ET_USES, generate_estate

STEP_KEYS = {"n_findings", "scores", "order", "pkg_idx", "win_idx", "n_agents", "n_creds",
             "n_tools", "reach_dist"}


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("make", GRAPHS, ids=lambda f: f.__name__)
def test_oracle_matches_hand_written(make, depth):
    g = make()
    hop, creds, hop_depth = cpu_ref.blast_hops(*cpu_args(g, depth))
    want_hop, want_creds, want_depth = g.expected(depth)
    assert hop.dtype == np.int32 and hop.shape == (g.n_pkgs, 4)
    assert creds.dtype == np.int32 and creds.shape == (g.n_pkgs,)
    assert hop_depth.dtype == np.uint8 and hop_depth.shape == (g.n_pkgs,)
    assert np.array_equal(hop, want_hop)
    assert np.array_equal(creds, want_creds)
    assert np.array_equal(hop_depth, want_depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_chain_has_one_agent_per_hop_cut_at_depth(depth):
    hop, _creds, hop_depth = cpu_ref.blast_hops(*cpu_args(chain(), depth))
    assert hop[0].tolist() == [1] * (depth - 1) + [0] * (5 - depth)
    assert int(hop_depth[0]) == depth


def test_depth_is_clamped():
    g = chain()
    for out_of_range, clamped in ((0, 1), (-3, 1), (6, 5), (9, 5)):
        got = cpu_ref.blast_hops(*cpu_args(g, out_of_range))
        want = cpu_ref.blast_hops(*cpu_args(g, clamped))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("make", GRAPHS, ids=lambda f: f.__name__)
def test_oracle_matches_host_model(make, depth):
    g = make()
    hop, creds, hop_depth = cpu_ref.blast_hops(*cpu_args(g, depth))
    src, dst, et = g.edges()
    agents, radii = model_objects(src, dst, et, g.n_agents, g.pkgs)
    for i, br in enumerate(radii):
        m_hop, m_creds, m_depth = expansion_counts(agents, br, depth)
        assert hop[i].tolist() == m_hop, (g.name, i)
        assert int(creds[i]) == m_creds, (g.name, i)
        assert int(hop_depth[i]) == m_depth, (g.name, i)


@pytest.fixture(scope="module")
def cpu_engine():
    return EstateEngine(generate_estate(**ESTATE_ARGS), device="cpu")


@pytest.fixture(scope="module")
def cpu_steps(cpu_engine):
    return {"default": cpu_engine.step(), 1: cpu_engine.step(blast_depth=1),
            3: cpu_engine.step(blast_depth=3)}


def test_estate_oracle_matches_host_model(cpu_engine, cpu_steps):
    est = cpu_engine.estate
    blast = cpu_engine.transitive_blast(cpu_steps["default"], max_depth=5)
    uniq = blast["uniq_pkgs"].numpy()
    depths = blast["hop_depth"].numpy()
    # one package per hop depth reached, and the heaviest: the host model is slow
    pick = sorted({int(np.flatnonzero(depths == d)[0]) for d in np.unique(depths)}
                  | {int(np.argmax(blast["t_agents"].numpy()))})
    agents, radii = model_objects(est.edge_src.astype(np.int64), est.edge_dst.astype(np.int64),
                                  est.edge_type, est.n_agents, uniq[pick])
    for i, br in zip(pick, radii):
        m_hop, m_creds, m_depth = expansion_counts(agents, br, 5)
        assert blast["hop_agents"][i].tolist() == m_hop
        assert int(blast["t_creds"][i]) == m_creds
        assert int(depths[i]) == m_depth


def test_transitive_blast_equals_oracle(cpu_engine, cpu_steps):
    blast = cpu_engine.transitive_blast(cpu_steps["default"], max_depth=3)
    uniq = blast["uniq_pkgs"]
    assert torch.equal(uniq, torch.unique(cpu_steps["default"]["pkg_idx"])
                       + cpu_engine.estate.pkg_base)
    hop, creds, hop_depth = cpu_ref.blast_hops(
        uniq.numpy(), cpu_engine.rev["row_off"].numpy(), cpu_engine.rev["col"].numpy(),
        cpu_engine.rev["etype"].numpy(), ET_CONTAINS, ET_USES, ET_HAS_CRED,
        cpu_engine.fwd["row_off"].numpy(), cpu_engine.fwd["col"].numpy(),
        cpu_engine.fwd["etype"].numpy(), 3)
    assert np.array_equal(blast["hop_agents"].numpy(), hop)
    assert np.array_equal(blast["t_creds"].numpy(), creds)
    assert np.array_equal(blast["hop_depth"].numpy(), hop_depth)
    assert np.array_equal(blast["t_agents"].numpy(), hop.sum(axis=1))
    assert blast["hop_agents"].dtype == torch.int32 and blast["hop_depth"].dtype == torch.uint8


def test_step_depth_one_is_todays_step(cpu_steps):
    assert set(cpu_steps["default"]) == STEP_KEYS
    assert set(cpu_steps[1]) == STEP_KEYS
    assert cpu_steps["default"]["n_findings"] == cpu_steps[1]["n_findings"]
    for key in STEP_KEYS - {"n_findings"}:
        assert torch.equal(cpu_steps["default"][key], cpu_steps[1][key]), key


def test_step_carries_hop_keys(cpu_engine, cpu_steps):
    res = cpu_steps[3]
    assert set(res) == STEP_KEYS | set(HOP_KEYS)
    n = res["n_findings"]
    assert n > 0
    assert res["hop_depth"].dtype == torch.uint8 and res["hop_depth"].shape == (n,)
    assert res["transitive_agents"].dtype == torch.int32 and res["transitive_agents"].shape == (n,)
    assert res["transitive_creds"].dtype == torch.int32 and res["transitive_creds"].shape == (n,)
    assert res["transitive_scores"].dtype == torch.float32
    assert res["transitive_scores"].shape == (n,)
    for key in STEP_KEYS - {"n_findings"}:
        assert torch.equal(res[key], cpu_steps["default"][key]), key
    # per finding = per unique package, gathered by package
    blast = cpu_engine.transitive_blast(cpu_steps["default"], max_depth=3)
    pos = torch.searchsorted(blast["uniq_pkgs"], res["pkg_idx"] + cpu_engine.estate.pkg_base)
    assert torch.equal(res["hop_depth"], blast["hop_depth"][pos])
    assert torch.equal(res["transitive_agents"], blast["t_agents"][pos])
    assert torch.equal(res["transitive_creds"], blast["t_creds"][pos])
    assert int(res["hop_depth"].max()) <= 3
    factor = torch.tensor([0.0] + [HOP_RISK_FACTORS[h] for h in range(1, 6)])
    want = torch.where(res["hop_depth"] > 1,
                       res["scores"] * factor[res["hop_depth"].long()], torch.zeros(n))
    assert torch.equal(res["transitive_scores"], want)
    assert bool((res["transitive_scores"][res["hop_depth"] == 1] == 0).all())


def test_step_depth_is_clamped_to_five(cpu_engine):
    nine, five = cpu_engine.step(blast_depth=9), cpu_engine.step(blast_depth=5)
    for key in HOP_KEYS:
        assert torch.equal(nine[key], five[key]), key
    assert set(torch.unique(five["hop_depth"]).tolist()) == {1, 2, 3, 4, 5}
