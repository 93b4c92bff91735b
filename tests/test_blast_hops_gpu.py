"""The multi-hop delegation kernels (ops/csrc/blast_hops.hip) against the
``cpu_ref.blast_hops`` oracle: hand-built graphs through ``native.blast_hops``
and a small estate through ``EstateEngine.step(blast_depth=k)``.  Every
comparison is exact.  The graphs that pass an LDS cap stay inside every
buffer: the kernel checks a cap before it stores.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from blast_hops_graphs import (
    ESTATE_ARGS, GRAPHS, HOP_KEYS, chain, cpu_args, device_inputs, fat, loop_back, orphans,
)

from agentbom_amd.graph.gpu_engine import EstateEngine
from agentbom_amd.ops import cpu_ref, native
from agentbom_amd.scan.synth import ET_CONTAINS, generate_estate

pytestmark = pytest.mark.gpu

GPU_DEPTHS = (2, 3, 5)


def _run(g, depth, ws=None):
    d = device_inputs(g)
    return native.blast_hops(d["pkgs32"], d["rev"], d["index"], d["agent_index"],
                             ET_CONTAINS, depth, ws)


def _assert_equal_to_oracle(g, depth, got):
    hop, creds, hop_depth = cpu_ref.blast_hops(*cpu_args(g, depth))
    assert got["hop_agents"].dtype == torch.int32 and got["hop_agents"].shape == (g.n_pkgs, 4)
    assert got["t_creds"].dtype == torch.int32 and got["t_creds"].shape == (g.n_pkgs,)
    assert got["hop_depth"].dtype == torch.uint8 and got["hop_depth"].shape == (g.n_pkgs,)
    assert np.array_equal(got["hop_agents"].cpu().numpy(), hop)
    assert np.array_equal(got["t_creds"].cpu().numpy(), creds)
    assert np.array_equal(got["hop_depth"].cpu().numpy(), hop_depth)


def test_caps_are_the_built_ones():
    lib = native.load()
    assert [lib.abom_blast_hops_cap(k) for k in range(4)] == [
        native.BLAST_HOPS_SRV_CAP, native.BLAST_HOPS_AG_CAP, native.BLAST_HOPS_CR_CAP, -1]


@pytest.mark.parametrize("depth", GPU_DEPTHS)
@pytest.mark.parametrize("make", GRAPHS, ids=lambda f: f.__name__)
def test_kernel_equals_oracle(make, depth):
    g = make()
    ws: dict = {}
    _assert_equal_to_oracle(g, depth, _run(g, depth, ws))
    assert isinstance(ws["hops_queued"], int) and isinstance(ws["hops_overflow"], int)
    assert 0 <= ws["hops_overflow"] <= ws["hops_queued"] <= g.n_pkgs


@pytest.mark.parametrize("depth", GPU_DEPTHS)
def test_fat_takes_the_exact_fallback(depth):
    g = fat()
    ws: dict = {}
    got = _run(g, depth, ws)
    # p0 passes the server cap, p1 the agent cap; p2 fits
    assert ws["hops_overflow"] == 2 and ws["hops_queued"] == 3
    _assert_equal_to_oracle(g, depth, got)


@pytest.mark.parametrize("make", (orphans, loop_back), ids=lambda f: f.__name__)
def test_nothing_to_walk_queues_nothing(make):
    ws: dict = {}
    _assert_equal_to_oracle(make(), 5, _run(make(), 5, ws))
    assert ws["hops_queued"] == 0 and ws["hops_overflow"] == 0


def test_sized_entry_reads_the_count_from_the_device():
    g = chain()
    d = device_inputs(g)
    # a buffer of 5 with one package that counts; the rest must stay untouched
    pkgs = torch.full((5,), int(g.pkgs[0]), dtype=torch.int32, device="cuda")
    n_dev = torch.tensor([1], dtype=torch.int64, device="cuda")
    hop, creds, hop_depth, overflow, queued, n_overflow = native.blast_hops_sized(
        pkgs, n_dev, d["rev"], d["index"], d["agent_index"], ET_CONTAINS, 3, {})
    want = g.expected(3)
    assert (queued, n_overflow) == (1, 0)
    assert hop[0].tolist() == want[0][0].tolist()
    assert int(creds[0]) == int(want[1][0]) and int(hop_depth[0]) == int(want[2][0])
    assert int(overflow[0]) == 0


def test_empty_package_list():
    d = device_inputs(chain())
    ws: dict = {}
    got = native.blast_hops(d["pkgs32"][:0], d["rev"], d["index"], d["agent_index"],
                            ET_CONTAINS, 3, ws)
    assert got["hop_agents"].shape == (0, 4) and got["hop_agents"].dtype == torch.int32
    assert got["t_creds"].shape == (0,) and got["hop_depth"].shape == (0,)
    # nothing was launched: no queue or counter buffer was ever allocated
    assert ws == {"hops_queued": 0, "hops_overflow": 0}


def test_arguments_are_checked():
    d = device_inputs(chain())
    with pytest.raises(TypeError):
        native.blast_hops(d["pkgs32"].to(torch.int64), d["rev"], d["index"], d["agent_index"],
                          ET_CONTAINS, 3)
    with pytest.raises(ValueError):
        native.blast_hops(d["pkgs32"].cpu(), d["rev"], d["index"], d["agent_index"],
                          ET_CONTAINS, 3)


@pytest.fixture(scope="module")
def engines():
    est = generate_estate(**ESTATE_ARGS)
    return EstateEngine(est, device="cuda"), EstateEngine(est, device="cpu")


@pytest.mark.parametrize("depth", GPU_DEPTHS)
def test_engine_step_equals_cpu_engine(engines, depth):
    gpu, cpu = engines
    got, want = gpu.step(blast_depth=depth), cpu.step(blast_depth=depth)
    if depth == 5:
        # the estate exercises every hop level; fail here if the generator changes
        assert set(torch.unique(want["hop_depth"]).tolist()) == {1, 2, 3, 4, 5}
    assert torch.equal(got["pkg_idx"].cpu(), want["pkg_idx"])
    for key in HOP_KEYS:
        assert got[key].dtype == want[key].dtype, key
        print(key, depth, "mismatches:", int((got[key].cpu() != want[key]).sum()),
              "of", want[key].numel())
    for key in HOP_KEYS:
        assert torch.equal(got[key].cpu(), want[key]), key


def test_engine_transitive_blast_equals_cpu_engine(engines):
    gpu, cpu = engines
    got, want = gpu.transitive_blast(max_depth=5), cpu.transitive_blast(max_depth=5)
    for key in ("uniq_pkgs", "hop_agents", "t_agents", "t_creds", "hop_depth"):
        assert torch.equal(got[key].cpu(), want[key]), key
    assert got["hop_agents"].is_cuda


def test_engine_depth_one_is_todays_step(engines):
    gpu, _cpu = engines
    base, one = gpu.step(), gpu.step(blast_depth=1)
    assert set(base) == set(one) and not set(HOP_KEYS) & set(one)
    for key in ("pkg_idx", "win_idx", "scores", "order"):
        assert torch.equal(base[key], one[key]), key
