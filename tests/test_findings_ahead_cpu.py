"""The capacity policy of the ahead finding assembly
(``native.findings_ahead_capacity``): pure Python, no GPU."""

from __future__ import annotations

from agentbom_amd.ops import native


def test_capacity_holds_the_size_it_was_derived_from():
    for n in (0, 1, 15, 16, 17, 63, 64, 1000, 327_063, 3_257_823, (1 << 31) - 1):
        cap = native.findings_ahead_capacity(n)
        assert cap >= n + 64
        assert cap <= n + n // 16 + 64


def test_capacity_is_monotone_and_never_negative():
    caps = [native.findings_ahead_capacity(n) for n in range(0, 5000, 7)]
    assert caps == sorted(caps)
    assert native.findings_ahead_capacity(-5) == native.findings_ahead_capacity(0) == 64


def test_toggle_reads_the_environment(monkeypatch):
    from agentbom_amd.graph.gpu_engine import findings_ahead_enabled

    monkeypatch.delenv("AGENT_BOM_FINDINGS_AHEAD", raising=False)
    assert findings_ahead_enabled()
    monkeypatch.setenv("AGENT_BOM_FINDINGS_AHEAD", "0")
    assert not findings_ahead_enabled()
    monkeypatch.setenv("AGENT_BOM_FINDINGS_AHEAD", "1")
    assert findings_ahead_enabled()
