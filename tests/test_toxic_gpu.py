"""The toxic-combination kernels (ops/csrc/toxic.hip) against the
``cpu_ref.toxic_combinations`` oracle: hand-built cases through
``native.toxic_combinations`` and a small estate through
``EstateEngine.toxic_combinations``.  Every comparison is exact; fp32 is
compared as int32 bit patterns.  The cases that pass an LDS cap stay inside
every buffer: the kernels check a cap before they store.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from remediation_cases import ESTATE_ARGS
from toxic_cases import (
    HAND_CASES, assert_engine_equals_oracle, device_inputs, engine_reference, full_server_list,
    many_packages, many_wide, one_advisory_two_waves, oracle, rules, run_at_lane_62, spread,
    wide_union,
)

from agentbom_amd.graph.gpu_engine import EstateEngine
from agentbom_amd.ops import cpu_ref, native
from agentbom_amd.scan.synth import generate_estate

pytestmark = pytest.mark.gpu

CAPS = {"servers": native.TOXIC_SRV_CAP, "agents": native.TOXIC_AG_CAP}


def _same(g, w, key):
    g, w = g.cpu(), torch.from_numpy(np.ascontiguousarray(w))
    assert g.dtype == w.dtype and g.shape == w.shape, key
    if g.dtype == torch.float32:
        g, w = g.view(torch.int32), w.view(torch.int32)
    print(key, "mismatches:", int((g != w).sum()), "of", w.numel())
    assert torch.equal(g, w), key


def _assert_same(got: dict, want: dict, table=None, case=None):
    """A ``native.toxic_combinations`` result against the oracle's."""
    _same(got["patterns"], want["patterns"], "patterns")
    _same(got["combo_score"], want["combo_score"], "combo_score")
    for key in cpu_ref.TOXIC_VULN_KEYS:
        _same(got["vulns"][key], want["vulns"][key], "vulns." + key)
    assert got["n_by_pattern"] == want["n_by_pattern"].tolist()
    assert got["n_multi_agent"] == want["n_multi_agent"]
    assert got["n_flagged"] == int(np.count_nonzero(want["patterns"]))
    if table is not None:
        _same(native.toxic_poison_servers(table, case.server_base), want["poison_servers"],
              "poison_servers")


def _run(case, ws=None, pool_slices=None):
    d = device_inputs(case)
    return native.toxic_combinations(**d, workspace=ws, pool_slices=pool_slices), d["table"]


def _assert_workspace_zero(ws):
    for key in native.TOXIC_ZERO_KEYS:
        assert key in ws and not bool(ws[key].any()), key


def test_caps_are_the_built_ones():
    lib = native.load()
    assert [lib.abom_toxic_cap(k) for k in range(4)] == [
        native.TOXIC_SRV_CAP, native.TOXIC_AG_CAP, native.TOXIC_T1_PKGS, -1]


@pytest.mark.parametrize("make", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_cases_equal_oracle(make):
    case = make()
    ws: dict = {}
    got, table = _run(case, ws)
    _assert_same(got, oracle(case), table, case)
    assert (ws["toxic_queued"], ws["toxic_rounds"]) == (0, 0)
    if case.findings:
        _assert_workspace_zero(ws)


def test_identity_map_passed_explicitly():
    case = rules()
    want = oracle(case)
    case.vuln_of = list(range(len(case.windows)))
    _assert_same(_run(case)[0], want)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_finding_counts(n):
    case = spread(n)
    _assert_same(_run(case)[0], oracle(case))


@pytest.mark.parametrize("make", (run_at_lane_62, one_advisory_two_waves),
                         ids=lambda f: f.__name__)
def test_fold_shapes(make):
    case = make()
    ws: dict = {}
    _assert_same(_run(case, ws)[0], oracle(case))
    _assert_workspace_zero(ws)


@pytest.mark.parametrize("delta", (-1, 0, 1))
@pytest.mark.parametrize("which", tuple(CAPS))
def test_unions_at_the_lds_caps(which, delta):
    case = wide_union(which, CAPS[which] + delta)
    want = oracle(case)
    assert want["vulns"]["n_" + which][0] == CAPS[which] + delta
    ws: dict = {}
    _assert_same(_run(case, ws)[0], want)
    # past the cap the advisory is counted in a bitmap slice, and is still exact
    assert ws["toxic_queued"] == (1 if delta > 0 else 0)
    assert ws["toxic_rounds"] == ws["toxic_queued"]
    _assert_workspace_zero(ws)


def test_package_threshold():
    # more packages than the wave tier takes, on few servers
    case = many_packages(native.TOXIC_T1_PKGS + 1, 3)
    ws: dict = {}
    _assert_same(_run(case, ws)[0], oracle(case))
    assert ws["toxic_queued"] == 1
    _assert_workspace_zero(ws)


def test_full_server_list_of_the_block_tier():
    # 1280 servers in one chunk of 256 packages: past the 1024 a block lists,
    # a thread visits the reach-index row itself (one plane; remediation's
    # test_install_threshold_and_full_server_list covers three)
    case = full_server_list()
    want = oracle(case)
    # by construction: 256 packages x 5 servers of their own, agents 0 .. 319,
    # fewer than the sum of the servers' agent lists
    assert want["vulns"]["n_packages"].tolist() == [256]
    assert want["vulns"]["n_servers"].tolist() == [1280]
    assert want["vulns"]["n_agents"].tolist() == [320] and len(case.uses) == 1600
    ws: dict = {}
    _assert_same(_run(case, ws)[0], want)
    assert ws["toxic_queued"] == 1
    _assert_workspace_zero(ws)


def test_pool_slices_are_reused_and_the_workspace_too():
    # four advisories past the server cap on two slices: every slice serves
    # two; then a small call on the same workspace
    first, second = many_wide(4, native.TOXIC_SRV_CAP + 1), rules()
    ws: dict = {}
    _assert_same(_run(first, ws, pool_slices=2)[0], oracle(first))
    assert (ws["toxic_queued"], ws["toxic_rounds"]) == (4, 2)
    _assert_workspace_zero(ws)
    _assert_same(_run(second, ws, pool_slices=2)[0], oracle(second))
    assert (ws["toxic_queued"], ws["toxic_rounds"]) == (0, 0)
    _assert_workspace_zero(ws)


def test_arguments_are_checked():
    d = device_inputs(rules())
    with pytest.raises(TypeError):
        native.toxic_combinations(**{**d, "pkg_idx": d["pkg_idx"].to(torch.int32)})
    with pytest.raises(TypeError):
        native.toxic_combinations(**{**d, "n_creds": d["n_creds"].to(torch.int64)})
    with pytest.raises(ValueError):
        native.toxic_combinations(**{**d, "pkg_idx": d["pkg_idx"].cpu()})


# ── engine level ────────────────────────────────────────────────────────────


@pytest.fixture(scope="module")
def engine():
    return EstateEngine(generate_estate(**ESTATE_ARGS), device="cuda")


@pytest.fixture(scope="module")
def stepped(engine):
    res = engine.step()
    assert 1000 < res["n_findings"] < 20000
    return res


@pytest.fixture(scope="module")
def caps(engine):
    return np.random.default_rng(5).integers(0, 32, engine.estate.n_tools).astype(np.uint8)


def _host_view(engine, stepped):
    """What ``engine_reference`` reads, copied to the host."""
    class Host:
        estate = engine.estate
        rev = {k: v.cpu() for k, v in engine.rev.items()}
        fwd = {k: v.cpu() for k, v in engine.fwd.items()}
        arena = {k: engine.arena[k].cpu() for k in ("severity", "kev", "impact")}
        tool_lut = engine.tool_lut.cpu()

    keys = ("pkg_idx", "win_idx", "scores", "n_creds", "n_tools")
    return Host, {k: stepped[k].cpu() for k in keys}


@pytest.mark.parametrize("mapped", (False, True), ids=("identity", "vuln_of"))
def test_engine_equals_oracle(engine, stepped, caps, mapped):
    W = engine.arena["severity"].numel()
    vmap = (np.arange(W) // 3).astype(np.int32) if mapped else None
    host, res = _host_view(engine, stepped)
    ref = engine_reference(host, res, caps, vmap)
    assert ref["n_by_pattern"].min() > 0 and len(ref["poison_servers"]) > 0
    dev_caps = torch.from_numpy(caps).cuda()
    dev_map = None if vmap is None else torch.from_numpy(vmap).cuda()
    full = engine.toxic_combinations(stepped, tool_caps=dev_caps, vuln_of=dev_map, k=None)
    assert full["patterns"].is_cuda and full["vulns"]["vuln"].is_cuda
    assert_engine_equals_oracle(full, ref)
    top = engine.toxic_combinations(stepped, tool_caps=dev_caps, vuln_of=dev_map, k=10)
    assert_engine_equals_oracle(top, ref, k=10)
    assert torch.equal(top["order"], full["order"][:10])
    for key in cpu_ref.TOXIC_VULN_KEYS:
        assert torch.equal(top["vulns"][key], full["vulns"][key][:10]), key
    for key in native.TOXIC_ZERO_KEYS:
        assert not bool(engine._toxic_ws[key].any()), key


def test_engine_without_caps(engine, stepped, caps):
    with_caps = engine.toxic_combinations(stepped, tool_caps=torch.from_numpy(caps).cuda(),
                                          k=None)
    got = engine.toxic_combinations(stepped, k=None)
    tools = cpu_ref.TP_EXECUTE_EXPLOIT | cpu_ref.TP_CACHE_POISON
    assert torch.equal(got["patterns"], with_caps["patterns"] & (0xFF ^ tools))
    assert got["poison_servers"].numel() == 0
    assert got["n_by_pattern"][2:4].tolist() == [0, 0]


def test_step_is_untouched(engine, caps):
    before = engine.step()
    engine.toxic_combinations(before, tool_caps=torch.from_numpy(caps).cuda(), k=5)
    engine.toxic_combinations(k=5)
    after = engine.step()
    for key, value in before.items():
        if torch.is_tensor(value):
            assert value.dtype == after[key].dtype, key
            if value.dtype == torch.float32:
                value, after[key] = value.view(torch.int32), after[key].view(torch.int32)
            assert torch.equal(value, after[key]), key
        else:
            assert value == after[key], key
