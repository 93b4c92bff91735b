"""GPU parity of the component kernels (ops/csrc/components.hip).

``native.connected_components`` / ``native.component_stats`` are compared
with the numpy oracle ``cpu_ref.*``, which tests/test_components_cpu.py holds
against a plain breadth-first labelling.  Labels, counts and sums are
integers with one right answer: every comparison is exact equality.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from components_graphs import ALL_ZERO, GRAPHS, unified_80

from agentbom_amd.graph.backend import HipBackend, NativeBackend, get_backend
from agentbom_amd.graph.container import UnifiedGraph
from agentbom_amd.graph.types import RelationshipType
from agentbom_amd.ops import cpu_ref, native
from agentbom_amd.scan.synth import ET_HAS_CRED, ET_USES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu_labels(src, dst, n, **kw) -> np.ndarray:
    got = native.connected_components(_dev(src), _dev(dst), n, **kw)
    assert got.dtype == torch.int32 and got.shape == (n,)
    return got.cpu().numpy()


@pytest.fixture(scope="module")
def rand():
    return GRAPHS["sparse_random"]()


@pytest.fixture(scope="module")
def rand_ref(rand):
    return cpu_ref.connected_components(*rand)


# ── labelling ───────────────────────────────────────────────────────────────


@pytest.mark.parametrize("n", [130, 1])
def test_no_edges_labels_every_node_itself(n):
    src, dst, _ = GRAPHS["no_edges_130"]()
    ws: dict = {}
    assert np.array_equal(_gpu_labels(src, dst, n, workspace=ws), np.arange(n))
    assert ws["cc_rounds"] == 0  # the hook kernel was not launched


def test_all_masked_edges_label_every_node_itself(rand):
    src, dst, n = rand
    etype = np.full(len(src), 3, dtype=np.uint8)
    got = _gpu_labels(src, dst, n, etype=_dev(etype), allowed_mask=0b0111)
    assert np.array_equal(got, np.arange(n))


@pytest.mark.parametrize("name", ALL_ZERO)
def test_single_component_graphs_label_zero(name):
    """zig-zag chain (and its reverse), contended root, lost-union comb with
    the hub's edges first and last."""
    src, dst, n = GRAPHS[name]()
    got = _gpu_labels(src, dst, n)
    assert not got.any(), f"{np.count_nonzero(got)} nodes missed component 0"
    assert np.array_equal(got, cpu_ref.connected_components(src, dst, n))


def test_zigzag_reversed_edges_give_identical_labels():
    src, dst, n = GRAPHS["zigzag_4097"]()
    assert np.array_equal(_gpu_labels(src, dst, n), _gpu_labels(dst, src, n))


def test_sparse_random_graph(rand, rand_ref):
    # conditions on the input, checked on the oracle's labels
    _, sizes = np.unique(rand_ref, return_counts=True)
    assert len(sizes) >= 400
    assert (sizes > 2).sum() >= 20
    assert sizes.max() >= 100
    src, dst, n = rand
    assert (src == dst).sum() >= 20
    assert np.array_equal(_gpu_labels(src, dst, n), rand_ref)


def test_edge_type_mask_equals_deleted_edges(rand, rand_ref):
    src, dst, n = rand
    etype = (np.arange(len(src)) % 3).astype(np.uint8)
    got = _gpu_labels(src, dst, n, etype=_dev(etype), allowed_mask=0b101)
    keep = etype != 1
    want = cpu_ref.connected_components(src[keep], dst[keep], n)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, rand_ref)


def test_repeat_runs_and_workspace_reuse(rand, rand_ref):
    src, dst, n = rand
    s, d = _dev(src), _dev(dst)
    first = native.connected_components(s, d, n)
    assert torch.equal(first, native.connected_components(s, d, n))
    ws: dict = {}
    a = native.connected_components(s, d, n, workspace=ws)
    b = native.connected_components(s, d, n, workspace=ws)  # reused
    assert torch.equal(a, first) and torch.equal(b, first)
    assert np.array_equal(first.cpu().numpy(), rand_ref)
    assert 2 <= ws["cc_rounds"] <= native.components_max_rounds(n)


def test_round_cap_raises_instead_of_returning_labels():
    src, dst, n = GRAPHS["zigzag_4097"]()
    with pytest.raises(RuntimeError, match="no fixed point"):
        native.connected_components(_dev(src), _dev(dst), n, max_rounds=1)


def test_wrapper_validates_its_arguments(rand):
    src, dst, n = rand
    s, d = _dev(src), _dev(dst)
    with pytest.raises(TypeError):
        native.connected_components(s.to(torch.int64), d, n)
    with pytest.raises(ValueError):
        native.connected_components(s, d[:-1], n)
    with pytest.raises(ValueError):
        native.connected_components(s, d, 1 << 31)
    with pytest.raises(ValueError):
        native.connected_components(s, d, n, allowed_mask=1)  # no etype
    with pytest.raises(ValueError):
        native.connected_components(s, torch.from_numpy(dst), n)  # host tensor


# ── component_stats ─────────────────────────────────────────────────────────


def _assert_stats_equal(comp, kind, C, K, weight=None, worst=None):
    got = native.component_stats(
        _dev(comp), _dev(kind), C, K,
        weight=None if weight is None else _dev(weight),
        worst=None if worst is None else _dev(worst))
    want = cpu_ref.component_stats(comp, kind, C, K, weight=weight, worst=worst)
    for g, w, what in zip(got, want, ("kind_counts", "weight_sum", "worst_min")):
        assert g.dtype == torch.from_numpy(w).dtype, what
        assert np.array_equal(g.cpu().numpy(), w), what
    return got


def test_component_stats_random_graph(rand, rand_ref):
    n = rand[2]
    roots, comp = np.unique(rand_ref, return_inverse=True)
    rng = np.random.default_rng(5)
    kind = rng.integers(0, 5, n).astype(np.uint8)
    weight = rng.integers(0, 1000, n).astype(np.int32)
    worst = rng.integers(0, 7, n).astype(np.uint8)
    kc, _ws, _wm = _assert_stats_equal(comp.astype(np.int32), kind, len(roots), 5,
                                       weight=weight, worst=worst)
    assert int(kc.sum()) == n
    _assert_stats_equal(comp.astype(np.int32), kind, len(roots), 5)  # nullable columns


def test_component_stats_sum_needs_64_bits():
    big = 2**31 - 1
    comp = np.array([1, 0, 1, 1], dtype=np.int32)
    kind = np.array([0, 1, 1, 0], dtype=np.uint8)
    weight = np.array([big, 7, big, big], dtype=np.int32)
    _kc, ws, _wm = _assert_stats_equal(comp, kind, 2, 2, weight=weight)
    assert ws.tolist() == [7, 3 * big]


@pytest.mark.parametrize("run", [63, 64, 65])
def test_component_stats_runs_across_a_wave(run):
    """Runs of same-component adjacent nodes that end one short of, at and
    one past a 64-lane wave, twice over so a run also starts mid-wave, then
    300 nodes that alternate between two components; the sizes are no
    multiple of the block."""
    comp = np.concatenate([np.full(run, 0), np.full(run, 1), np.full(run, 0),
                           np.arange(300) % 2 + 2]).astype(np.int32)
    n = len(comp)
    rng = np.random.default_rng(run)
    kind = rng.integers(0, 8, n).astype(np.uint8)
    kind[:run] = 7  # a whole run of one class: the packed counter's maximum
    weight = rng.integers(-1000, 1000, n).astype(np.int32)
    worst = rng.integers(0, 256, n).astype(np.uint8)
    kc, _ws, _wm = _assert_stats_equal(comp, kind, 4, 8, weight=weight, worst=worst)
    assert int(kc[0, 7]) >= run


# ── backend ─────────────────────────────────────────────────────────────────


def test_hip_backend_against_native_backend():
    g = unified_80()
    hip = get_backend("hip")
    assert hip.name == "hip" and isinstance(hip, HipBackend)
    want = NativeBackend().components(g)
    got = hip.components(g)
    assert got == want and list(got) == list(want)
    rels = {RelationshipType.USES}
    assert hip.components(g, relationships=rels) == NativeBackend().components(g, rels)
    assert g.connected_components(backend="hip") == want
    assert UnifiedGraph().connected_components(backend="hip") == {}


# ── engines ─────────────────────────────────────────────────────────────────


@pytest.fixture(scope="module")
def engines():
    from agentbom_amd.graph.gpu_engine import EstateEngine
    from agentbom_amd.scan.synth import generate_estate

    est = generate_estate(n_agents=200, n_servers=1000, n_packages=50_000,
                          name_catalog=10_000, seed=42)
    return EstateEngine(est, device=DEV), EstateEngine(est, device="cpu")


@pytest.mark.parametrize("mask", [(1 << ET_USES) | (1 << ET_HAS_CRED), None])
def test_engine_components_gpu_against_cpu(engines, mask):
    gpu, cpu = engines
    got = gpu.components(mask)
    assert got.device.type == "cuda" and got.dtype == torch.int32
    assert torch.equal(got.cpu(), cpu.components(mask))


def test_engine_lateral_domains_gpu_against_cpu(engines):
    gpu, cpu = engines
    step = gpu.step()
    step_cpu = {k: v.cpu() if hasattr(v, "cpu") else v for k, v in step.items()}
    for k in (20, 3):
        got = gpu.lateral_domains(step, k=k)
        want = cpu.lateral_domains(step_cpu, k=k)
        assert sorted(got) == sorted(want)
        for key in ("root", "agents", "servers", "creds", "findings", "worst"):
            assert got[key].device.type == "cuda"
            assert got[key].dtype == want[key].dtype, key
            assert torch.equal(got[key].cpu(), want[key]), key
        assert got["n_domains"] == want["n_domains"] > 0
        assert got["largest_agents"] == want["largest_agents"] >= 2
        assert int(got["findings"].sum()) > 0
