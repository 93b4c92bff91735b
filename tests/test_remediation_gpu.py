"""The remediation kernels (ops/csrc/remediation.hip) against the
``cpu_ref.remediation_plan`` oracle: hand-built cases through
``native.remediation_items`` and a small estate through
``EstateEngine.remediation_plan``.  Every comparison is exact; ``max_score``
is compared as int32 bit patterns.  The cases that pass an LDS cap stay inside
every buffer: the kernels check a cap before they store.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from remediation_cases import (
    ESTATE_ARGS, HAND_CASES, device_inputs, first_and_last_item, many_installs, many_wide,
    one_item_two_waves, oracle, spread, three_items, wide_union,
)

from agentbom_amd.graph.gpu_engine import EstateEngine
from agentbom_amd.ops import cpu_ref, native
from agentbom_amd.scan.synth import (
    ET_CONTAINS, ET_HAS_CRED, ET_PROVIDES_TOOL, ET_USES, generate_estate,
)

pytestmark = pytest.mark.gpu

CAPS = {"servers": native.REMEDIATION_SRV_CAP, "agents": native.REMEDIATION_AG_CAP,
        "creds": native.REMEDIATION_CR_CAP, "tools": native.REMEDIATION_TL_CAP}


def _assert_same(got: dict, want: dict, keys=cpu_ref.REMEDIATION_KEYS):
    """``got`` torch tensors, ``want`` numpy arrays or torch tensors."""
    for key in keys:
        w = want[key].cpu() if torch.is_tensor(want[key]) else torch.from_numpy(want[key])
        g = got[key].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, key
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        print(key, "mismatches:", int((g != w).sum()), "of", w.numel())
        assert torch.equal(g, w), key


def _run(case, ws=None, pool_slices=None):
    return native.remediation_items(**device_inputs(case), workspace=ws, pool_slices=pool_slices)


def _assert_workspace_zero(ws):
    for key in native.REMEDIATION_ZERO_KEYS:
        assert key in ws and not bool(ws[key].any()), key


def test_caps_are_the_built_ones():
    lib = native.load()
    assert [lib.abom_remediation_cap(k) for k in range(6)] == [
        native.REMEDIATION_SRV_CAP, native.REMEDIATION_AG_CAP, native.REMEDIATION_CR_CAP,
        native.REMEDIATION_TL_CAP, native.REMEDIATION_T1_INSTALLS, -1]


@pytest.mark.parametrize("make", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_cases_equal_oracle(make):
    case = make()
    ws: dict = {}
    _assert_same(_run(case, ws), oracle(case))
    assert (ws["remed_queued"], ws["remed_rounds"]) == (0, 0)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_finding_counts(n):
    case = spread(f"spread_{n}", n)
    _assert_same(_run(case), oracle(case))


@pytest.mark.parametrize("make", (one_item_two_waves, first_and_last_item),
                         ids=lambda f: f.__name__)
def test_fold_shapes(make):
    case = make()
    want = oracle(case)
    if make is one_item_two_waves:
        assert want["n_findings"].tolist() == [128]
    else:
        assert want["item"].tolist() == [0, max(case.item_of)]
    _assert_same(_run(case), want)


@pytest.mark.parametrize("delta", (-1, 0, 1))
@pytest.mark.parametrize("which", tuple(CAPS))
def test_unions_at_the_lds_caps(which, delta):
    case = wide_union(which, CAPS[which] + delta)
    want = oracle(case)
    assert want["n_" + which][0] == CAPS[which] + delta
    ws: dict = {}
    _assert_same(_run(case, ws), want)
    # past the cap the item is counted in a bitmap slice, and is still exact
    assert ws["remed_queued"] == (1 if delta > 0 else 0)
    assert ws["remed_rounds"] == ws["remed_queued"]
    _assert_workspace_zero(ws)


def test_install_threshold_and_full_server_list():
    # more installs than the wave tier takes, on few servers; then 256
    # installs whose first chunk names more servers than the block's list holds
    for case in (many_installs(native.REMEDIATION_T1_INSTALLS + 1, 1, 3),
                 many_installs(256, 5, 1400)):
        ws: dict = {}
        _assert_same(_run(case, ws), oracle(case))
        assert ws["remed_queued"] == 1
        _assert_workspace_zero(ws)


def test_pool_slices_are_reused():
    # four items past the server cap, two slices: every slice serves two items
    case = many_wide(4, native.REMEDIATION_SRV_CAP + 1)
    ws: dict = {}
    _assert_same(_run(case, ws, pool_slices=2), oracle(case))
    assert (ws["remed_queued"], ws["remed_rounds"]) == (4, 2)
    _assert_workspace_zero(ws)


def test_workspace_reuse():
    first, second = many_wide(3, native.REMEDIATION_SRV_CAP + 1), three_items()
    ws: dict = {}
    _run(first, ws, pool_slices=2)
    _assert_workspace_zero(ws)
    got = _run(second, ws, pool_slices=2)
    _assert_same(got, _run(second, {}, pool_slices=2))
    _assert_same(got, oracle(second))
    _assert_workspace_zero(ws)


@pytest.mark.parametrize("make", (three_items, lambda: many_wide(2, 300),
                                  lambda: spread("spread_257", 257)),
                         ids=("three_items", "many_wide", "spread"))
def test_torch_join_equals_native(make):
    case = make()
    d = device_inputs(case)
    d.pop("n_items")
    _assert_same(native.remediation_items_join(**d), _run(case))


def test_arguments_are_checked():
    d = device_inputs(three_items())
    with pytest.raises(TypeError):
        native.remediation_items(**{**d, "pkg_idx": d["pkg_idx"].to(torch.int32)})
    with pytest.raises(ValueError):
        native.remediation_items(**{**d, "pkg_idx": d["pkg_idx"].cpu()})


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
def reference(engine, stepped):
    """The oracle on the GPU step's own tensors, copied to the host."""
    est = engine.estate
    item_of = cpu_ref.remediation_item_of(est.pkg_name_id, est.pkg_key_hi, est.pkg_key_lo)
    windows = engine.arena["windows"]

    def host(t):
        return t.cpu().numpy()

    return cpu_ref.remediation_plan(
        host(stepped["pkg_idx"]), host(stepped["win_idx"]), host(stepped["scores"]), item_of,
        host(engine.rev["row_off"]), host(engine.rev["col"]), host(engine.rev["etype"]),
        host(engine.fwd["row_off"]), host(engine.fwd["col"]), host(engine.fwd["etype"]),
        ET_CONTAINS, ET_USES, ET_HAS_CRED, ET_PROVIDES_TOOL, est.pkg_base,
        host(windows["flags"]), host(windows["fixed_hi"]), host(windows["fixed_lo"]),
        host(engine.arena["severity"]), host(engine.arena["kev"]), est.n_agents)


def _ordered(ref: dict, k=None) -> dict:
    order = ref["order"] if k is None else ref["order"][:k]
    return {key: ref[key][order] for key in cpu_ref.REMEDIATION_KEYS + ("agents_pct",)}


PLAN_KEYS = cpu_ref.REMEDIATION_KEYS + ("agents_pct",)


def test_engine_item_of(engine):
    est = engine.estate
    item_of, n_items = engine.remediation_items()
    want = cpu_ref.remediation_item_of(est.pkg_name_id, est.pkg_key_hi, est.pkg_key_lo)
    assert n_items == int(want.max()) + 1
    assert np.array_equal(item_of.cpu().numpy(), want)


def test_engine_plan_equals_oracle(engine, stepped, reference):
    full = engine.remediation_plan(stepped, k=None)
    assert full["n_items"] == len(reference["item"]) > 10
    assert full["item"].is_cuda
    _assert_same(full, _ordered(reference), PLAN_KEYS)
    top = engine.remediation_plan(stepped, k=10)
    assert top["n_items"] == full["n_items"]
    for key in PLAN_KEYS:
        assert torch.equal(top[key], full[key][:10]), key
    for key in native.REMEDIATION_ZERO_KEYS:
        assert not bool(engine._remed_ws[key].any()), key


def test_engine_torch_arm_equals_native(engine, stepped, env):
    native_plan = engine.remediation_plan(stepped, k=None)
    env(AGENT_BOM_REMEDIATION_NATIVE=0)
    _assert_same(engine.remediation_plan(stepped, k=None), native_plan, PLAN_KEYS)


def test_engine_without_dedup_layout(engine, stepped):
    bare = EstateEngine(engine.estate, device="cuda")
    bare.match_dedup = bare.match_table = None
    want = engine.remediation_plan(stepped, k=None)
    # the same findings through the engine that has no layout, and its own step
    _assert_same(bare.remediation_plan(stepped, k=None), want, PLAN_KEYS)
    own = bare.step()
    assert torch.equal(own["pkg_idx"], stepped["pkg_idx"])
    assert torch.equal(own["win_idx"], stepped["win_idx"])
    assert torch.equal(own["scores"], stepped["scores"])
    _assert_same(bare.remediation_plan(own, k=None), want, PLAN_KEYS)


def test_engine_plan_runs_the_step_itself(engine, stepped):
    got = engine.remediation_plan(k=5)
    want = engine.remediation_plan(stepped, k=5)
    _assert_same(got, want, PLAN_KEYS)
