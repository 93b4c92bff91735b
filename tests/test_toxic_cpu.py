"""The toxic-combination oracle (``cpu_ref.toxic_combinations``) against
answers worked out by hand, ``EstateEngine.toxic_combinations`` on the CPU,
and the helpers of ``graph.toxic_combos``.  Every comparison is exact; fp32 is
compared as int32 bit patterns.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from remediation_cases import ESTATE_ARGS
from toxic_cases import (
    HAND_CASES, assert_engine_equals_oracle, engine_reference, one_advisory_two_waves, oracle,
    rules, run_at_lane_62, two_windows_one_advisory,
)

from agentbom_amd.graph.gpu_engine import EstateEngine
from agentbom_amd.graph.toxic_combos import estate_combinations, tool_caps_from_labels
from agentbom_amd.ops import cpu_ref
from agentbom_amd.scan.synth import generate_estate

TOP_DTYPES = {"patterns": np.uint8, "combo_score": np.float32, "poison_servers": np.int32,
              "n_by_pattern": np.int64}
VULN_DTYPES = {"max_score": np.float32, "worst_sev": np.uint8, "kev": np.uint8,
               "patterns": np.uint8, "order": np.int64}


def _bits(a, dtype):
    a = np.asarray(a, dtype=dtype)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_expected(case, got):
    want = case.expected
    for key, dtype in TOP_DTYPES.items():
        assert got[key].dtype == dtype, key
        assert np.array_equal(_bits(got[key], dtype), _bits(want[key], dtype)), key
    assert got["n_multi_agent"] == want["n_multi_agent"]
    assert set(got["vulns"]) == set(cpu_ref.TOXIC_VULN_KEYS) | {"order"}
    for key, values in want["vulns"].items():
        dtype = VULN_DTYPES.get(key, np.int32)
        assert got["vulns"][key].dtype == dtype, key
        assert np.array_equal(_bits(got["vulns"][key], dtype), _bits(values, dtype)), key


@pytest.mark.parametrize("make", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_cases(make):
    case = make()
    _assert_expected(case, oracle(case))


def test_constants():
    assert (cpu_ref.TC_EXEC, cpu_ref.TC_WRITE, cpu_ref.TC_DELETE, cpu_ref.TC_READ,
            cpu_ref.TC_RETRIEVAL, cpu_ref.TC_DANGEROUS) == (1, 2, 4, 8, 16, 7)
    assert (cpu_ref.TP_CRED_BLAST, cpu_ref.TP_KEV_WITH_CREDS, cpu_ref.TP_EXECUTE_EXPLOIT,
            cpu_ref.TP_CACHE_POISON, cpu_ref.TP_LATERAL_CHAIN,
            cpu_ref.TP_MULTI_AGENT_CVE) == (1, 2, 4, 8, 16, 32)
    assert len(cpu_ref.TOXIC_PATTERN_NAMES) == 6


def test_severity_three_against_four_and_kev_at_medium():
    got = oracle(rules())["patterns"]
    assert got[0] & cpu_ref.TP_CRED_BLAST and not got[1] & cpu_ref.TP_CRED_BLAST
    assert got[2] == cpu_ref.TP_KEV_WITH_CREDS


def test_tool_impact_classes():
    got = oracle(rules())["patterns"]
    # class 1: the exec tool of s0 is no db tool, the one of s1 is; class 0: none
    assert not got[3] & cpu_ref.TP_EXECUTE_EXPLOIT and got[5] & cpu_ref.TP_EXECUTE_EXPLOIT
    assert not got[5] & cpu_ref.TP_CACHE_POISON
    assert got[6] == cpu_ref.TP_LATERAL_CHAIN


def test_identity_map_equals_no_map():
    case = rules()
    none = oracle(case)
    explicit = oracle(case, vuln_of=np.arange(len(case.windows), dtype=np.int32))
    for key in TOP_DTYPES:
        assert np.array_equal(none[key], explicit[key]), key
    for key in none["vulns"]:
        assert np.array_equal(none["vulns"][key], explicit["vulns"][key]), key


def test_two_windows_of_one_advisory_count_the_package_once():
    got = oracle(two_windows_one_advisory())["vulns"]
    assert (got["n_findings"][0], got["n_packages"][0]) == (2, 1)


def test_inconsistent_n_tools_is_refused():
    case = rules()
    case.findings[0] = (0, 0, 4.0, 1, 0)  # exposes t0, yet the step counted no tool
    with pytest.raises(ValueError):
        oracle(case)


@pytest.mark.parametrize("make", (run_at_lane_62, one_advisory_two_waves),
                         ids=lambda f: f.__name__)
def test_generated_cases_hold_their_shape(make):
    case = make()
    got = oracle(case)
    assert len(got["patterns"]) == len(case.findings)
    assert int(got["vulns"]["n_findings"].sum()) == len(case.findings)
    if make is one_advisory_two_waves:
        assert got["vulns"]["n_findings"].tolist() == [128]
        assert got["vulns"]["n_packages"].tolist() == [128]
    else:
        # the run of four: two advisories, two findings on one package each
        assert case.findings[62][0] == case.findings[65][0] == 62
        assert len({case.vuln_of[f[1]] for f in case.findings[62:66]}) == 2


# ── graph.toxic_combos ──────────────────────────────────────────────────────


def test_tool_caps_from_labels():
    caps = tool_caps_from_labels([
        "run_command", "runner", "job-runner.status", "execute", "eval.js", "shell",
        "write_file", "upsert-vectors", "delete_row", "destroy", "read", "Search.Docs",
        "get", "getter", "semantic_search", "retrieve_chunks", "retrieval", "rag",
        "storage", "list"])
    E, W, D, R, V = (cpu_ref.TC_EXEC, cpu_ref.TC_WRITE, cpu_ref.TC_DELETE, cpu_ref.TC_READ,
                     cpu_ref.TC_RETRIEVAL)
    assert caps.dtype == np.uint8
    assert caps.tolist() == [E, 0, 0, E, E, E, W, W, D, D, R, R, R, 0, R | V, V, V, V, 0, 0]


def test_estate_combinations():
    result = {
        "order": torch.tensor([2, 0], dtype=torch.int64),
        "patterns": torch.tensor([5, 0, 48], dtype=torch.uint8),
        "combo_score": torch.tensor([6.0, 0.0, 9.5], dtype=torch.float32),
        "pkg_idx": torch.tensor([7, 8, 9]), "win_idx": torch.tensor([1, 0, 2]),
        "vuln_of": torch.tensor([4, 4, 6], dtype=torch.int32)}
    assert estate_combinations(result, k=5) == [
        {"finding": 2, "package": 9, "advisory": 6,
         "patterns": ["lateral_chain", "multi_agent_cve"], "score": 9.5},
        {"finding": 0, "package": 7, "advisory": 4,
         "patterns": ["cred_blast", "execute_exploit"], "score": 6.0}]
    assert len(estate_combinations(result, k=1)) == 1
    assert estate_combinations({**result, "vuln_of": None}, k=1)[0]["advisory"] == 2


# ── engine on the CPU ───────────────────────────────────────────────────────


@pytest.fixture(scope="module")
def cpu_engine():
    return EstateEngine(generate_estate(**ESTATE_ARGS), device="cpu")


@pytest.fixture(scope="module")
def stepped(cpu_engine):
    return cpu_engine.step()


def test_engine_on_the_cpu(cpu_engine, stepped):
    est = cpu_engine.estate
    caps = np.random.default_rng(5).integers(0, 32, est.n_tools).astype(np.uint8)
    W = cpu_engine.arena["severity"].numel()
    vuln_of = (np.arange(W) // 3).astype(np.int32)
    for vmap in (None, vuln_of):
        ref = engine_reference(cpu_engine, stepped, caps, vmap)
        assert ref["n_by_pattern"].min() > 0 and len(ref["poison_servers"]) > 0
        got = cpu_engine.toxic_combinations(
            stepped, tool_caps=torch.from_numpy(caps),
            vuln_of=None if vmap is None else torch.from_numpy(vmap), k=None)
        assert_engine_equals_oracle(got, ref)
        top = cpu_engine.toxic_combinations(
            stepped, tool_caps=torch.from_numpy(caps),
            vuln_of=None if vmap is None else torch.from_numpy(vmap), k=10)
        assert_engine_equals_oracle(top, ref, k=10)
    rows = estate_combinations(top, k=3)
    assert [r["finding"] for r in rows] == top["order"][:3].tolist()


def test_engine_without_caps_on_the_cpu(cpu_engine, stepped):
    got = cpu_engine.toxic_combinations(stepped, k=None)
    tools = cpu_ref.TP_EXECUTE_EXPLOIT | cpu_ref.TP_CACHE_POISON
    assert not bool((got["patterns"] & tools).any())
    assert got["poison_servers"].numel() == 0
    assert got["n_by_pattern"][2] == 0 and got["n_by_pattern"][3] == 0
    # a call without a step result runs the step itself
    again = cpu_engine.toxic_combinations(k=None)
    assert torch.equal(again["patterns"], got["patterns"])
    assert torch.equal(again["combo_score"], got["combo_score"])
