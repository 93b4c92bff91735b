"""The remediation-plan oracle (``cpu_ref.remediation_plan``) against answers
worked out by hand, and ``EstateEngine.remediation_plan`` on the CPU.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from remediation_cases import (
    ESTATE_ARGS, TOP, device_inputs, empty_findings, many_installs, many_wide, oracle,
    order_ties, spread, three_items, wide_union,
)

from agentbom_amd.graph.gpu_engine import EstateEngine
from agentbom_amd.ops import cpu_ref
from agentbom_amd.scan.synth import generate_estate

U64_KEYS = ("fix_hi", "fix_lo")


def _assert_expected(case, got):
    for key, want in case.expected.items():
        if key in U64_KEYS:
            assert got[key].view(np.uint64).tolist() == want, key
        else:
            assert got[key].tolist() == want, key
    assert got["order"].tolist() == case.expected_order


@pytest.fixture(scope="module")
def three():
    case = three_items()
    return case, oracle(case)


def test_three_items_over_six_packages(three):
    case, got = three
    assert set(got) == set(cpu_ref.REMEDIATION_KEYS) | {"agents_pct", "order"}
    _assert_expected(case, got)


def test_dtypes(three):
    _case, got = three
    for key in cpu_ref.REMEDIATION_KEYS:
        want = {"max_score": np.float32, "worst_sev": np.uint8, "kev": np.uint8,
                "fix_hi": np.int64, "fix_lo": np.int64}.get(key, np.int32)
        assert got[key].dtype == want, key
    assert got["agents_pct"].dtype == np.float32 and got["order"].dtype == np.int64


def test_duplicate_contains_edge_counts_once(three):
    # item 1: p2 has the edge from s0 twice, p5 has no containing server
    _case, got = three
    assert got["n_servers"][1] == 1 and got["installs"][1] == 2


def test_two_installs_on_one_server_and_a_server_without_agents(three):
    # item 2: p3 and p4 both in s2; s3 adds a tool and no agent
    _case, got = three
    assert (got["n_servers"][2], got["n_agents"][2], got["n_tools"][2]) == (2, 2, 2)


def test_two_items_share_a_server(three):
    # s0 holds p0 (item 0) and p2 (item 1): both count it and its agents
    _case, got = three
    assert got["n_agents"][0] == 2 and got["n_agents"][1] == 2


def test_fixed_keys(three):
    _case, got = three
    # item 0: three fixed keys with one hi; the lo with bit 63 set is the largest
    assert (got["fix_hi"][0], got["fix_lo"].view(np.uint64)[0], got["n_unfixed"][0]) == (
        1, TOP + 1, 0)
    # item 1: nothing fixed; the key words of an unfixed window are not read
    assert (got["fix_hi"][1], got["fix_lo"][1], got["n_unfixed"][1]) == (0, 0, 2)
    # item 2: one fixed, one not
    assert (got["fix_hi"][2], got["fix_lo"][2], got["n_unfixed"][2]) == (1, 9, 1)


def test_order_ties():
    case = order_ties()
    _assert_expected(case, oracle(case))


def test_empty_findings():
    got = oracle(empty_findings())
    for key in cpu_ref.REMEDIATION_KEYS + ("agents_pct", "order"):
        assert got[key].shape == (0,), key


def test_unmatched_items_are_left_out():
    case = spread("first_and_last", 12, n_items=10, matched_items=[0, 9])
    got = oracle(case)
    assert got["item"].tolist() == [0, 9] and got["installs"].tolist() == [6, 6]


def test_item_of_orders_triples_unsigned():
    gk = np.asarray([5, TOP, 5, 5, TOP, 5], dtype=np.uint64)
    hi = np.asarray([1, 0, 1, TOP, 0, 1], dtype=np.uint64)
    lo = np.asarray([2, 0, TOP, 0, 0, 2], dtype=np.uint64)
    # (5,1,2) < (5,1,TOP) < (5,TOP,0) < (TOP,0,0)
    assert cpu_ref.remediation_item_of(gk, hi, lo).tolist() == [0, 3, 1, 2, 3, 0]


@pytest.mark.parametrize("make", (
    three_items, order_ties, empty_findings, lambda: spread("spread_65", 65),
    lambda: wide_union("agents", 70), lambda: wide_union("servers", 40),
    lambda: many_wide(3, 33), lambda: many_installs(50, 3, 40)),
    ids=("three_items", "order_ties", "empty", "spread", "wide_agents", "wide_servers",
         "many_wide", "many_installs"))
def test_torch_join_equals_oracle(make):
    # the comparison arm is plain torch: on the CPU it runs on host tensors
    from agentbom_amd.ops import native

    case = make()
    d = device_inputs(case, device="cpu")
    d.pop("n_items")
    got, want = native.remediation_items_join(**d), oracle(case)
    for key in cpu_ref.REMEDIATION_KEYS:
        assert got[key].dtype == torch.from_numpy(want[key]).dtype, key
        assert np.array_equal(got[key].numpy(), want[key]), key


@pytest.fixture(scope="module")
def cpu_engine():
    return EstateEngine(generate_estate(**ESTATE_ARGS), device="cpu")


def test_engine_item_of_equals_oracle(cpu_engine):
    est = cpu_engine.estate
    item_of, n_items = cpu_engine.remediation_items()
    want = cpu_ref.remediation_item_of(est.pkg_name_id, est.pkg_key_hi, est.pkg_key_lo)
    assert item_of.dtype == torch.int32 and n_items == int(want.max()) + 1
    assert np.array_equal(item_of.numpy(), want)


def test_engine_plan_on_the_cpu(cpu_engine):
    res = cpu_engine.step()
    assert res["n_findings"] > 100
    full = cpu_engine.remediation_plan(res, k=None)
    top = cpu_engine.remediation_plan(res, k=10)
    M = full["n_items"]
    assert M > 10 and top["n_items"] == M
    for key in cpu_ref.REMEDIATION_KEYS + ("agents_pct",):
        assert full[key].shape == (M,), key
        assert torch.equal(top[key], full[key][:10]), key
    # ranked: score descending, then agents descending, then item ascending
    rows = list(zip((-full["max_score"]).tolist(), (-full["n_agents"]).tolist(),
                    full["item"].tolist()))
    assert rows == sorted(rows)
    assert int(full["n_findings"].sum()) == res["n_findings"]
    assert int(full["installs"].sum()) == int(torch.unique(res["pkg_idx"]).numel())
    # per item, the distinct union is bounded by the per-package counts
    assert int(full["n_agents"].max()) <= cpu_engine.estate.n_agents
    assert torch.equal(full["agents_pct"],
                       full["n_agents"].float() * 100.0 / cpu_engine.estate.n_agents)
    # a plan without a step result runs the step itself
    again = cpu_engine.remediation_plan(k=10)
    for key in cpu_ref.REMEDIATION_KEYS:
        assert torch.equal(again[key], top[key]), key
