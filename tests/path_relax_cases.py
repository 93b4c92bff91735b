"""Shared inputs for the path-relax tests (CPU oracle and HIP kernel).

Hand-built one-hop cases with the expected labels written out, plus seeded
random graphs that carry per-edge weights.  Everything here is plain numpy;
tests/test_attack_paths_dp.py checks cpu_ref.path_relax against it and
tests/test_path_relax_gpu.py checks ops/csrc/paths.hip.

Edge types used throughout: 0, 1 and 3 are traversable, 2 is traversable and
a gate edge, 4 and 5 are not traversable (4 carries a large boost so that a
kernel which forgot the traversable table would show it).
"""

from __future__ import annotations

import numpy as np

f32 = np.float32
NO_EDGE = 0xFFFFFFFF
W_SCALE = f32(0.3)

ETYPE_BOOST = {0: 0.3, 1: 0.5, 2: 1.5, 3: 0.25, 4: 9.0, 5: 0.0}
TRAVERSABLE = [0, 1, 2, 3]
GATE_TYPES = [2]


def tables():
    eb = np.zeros(256, dtype=np.float32)
    for t, b in ETYPE_BOOST.items():
        eb[t] = b
    tv = np.zeros(256, dtype=np.uint8)
    tv[TRAVERSABLE] = 1
    eg = np.zeros(256, dtype=np.uint8)
    eg[GATE_TYPES] = 1
    return eb, tv, eg


def pack(score, edge: int) -> int:
    """(ordered_f32(score) << 32) | edge for a non-negative score."""
    bits = int(np.array([score], dtype=np.float32).view(np.uint32)[0])
    return ((bits | 0x80000000) << 32) | int(edge)


SEED = pack(0.0, NO_EDGE)


def hop_score(prev, etype: int, boost_v, weight):
    """prev + ((etype_boost + node_boost) + weight * 0.3f), one f32 rounding
    per operation — the arithmetic the host reconstruction repeats."""
    step = f32(ETYPE_BOOST[etype]) + f32(boost_v)
    scaled = f32(weight) * W_SCALE
    step = f32(step + scaled)
    return f32(f32(prev) + step)


def _case(n, edges, cur, nb=None, ng=None, expect=None):
    """edges: list of (src, dst, etype, weight); cur/expect: {(node, slot): label}."""
    src = np.array([e[0] for e in edges], dtype=np.int32)
    dst = np.array([e[1] for e in edges], dtype=np.int32)
    et = np.array([e[2] for e in edges], dtype=np.uint8)
    w = np.array([e[3] for e in edges], dtype=np.float32)
    nbv = np.zeros(n, dtype=np.float32)
    for v, b in (nb or {}).items():
        nbv[v] = b
    ngv = None
    if ng is not None:
        ngv = np.zeros(n, dtype=np.uint8)
        ngv[list(ng)] = 1
    curv = np.zeros(n * 2, dtype=np.uint64)
    for (v, g), lab in cur.items():
        curv[v * 2 + g] = np.uint64(lab)
    want = np.zeros(n * 2, dtype=np.uint64)
    for (v, g), lab in (expect or {}).items():
        want[v * 2 + g] = np.uint64(lab)
    return dict(n=n, src=src, dst=dst, et=et, w=w, nb=nbv, ng=ngv, cur=curv,
                expect=want)


def hand_cases() -> dict:
    """name -> case; every expected label is written out below."""
    cases = {}

    # Two edges into slot (2, 0) with bit-equal scores: edge 1 (the larger
    # index) wins.  Edge 2 has the largest index but a lower score and loses:
    # the score ranks first, the index only breaks ties.
    cases["tie_larger_edge_wins"] = _case(
        3,
        [(0, 2, 0, 0.7), (1, 2, 0, 0.7), (0, 2, 0, 0.1)],
        cur={(0, 0): SEED, (1, 0): SEED},
        nb={2: 0.4},
        expect={(2, 0): pack(hop_score(0.0, 0, 0.4, 0.7), 1)},
    )

    # 2-cycle guard.  e0: 0->1, e1: 1->0, e2: 1->2.  Node 1's label came over
    # e0 from node 0, so e1 must not carry it back; e2 still relaxes.
    cyc = [(0, 1, 0, 0.7), (1, 0, 0, 1.3), (1, 2, 1, 0.9)]
    cases["guard_slot0"] = _case(
        3, cyc, cur={(1, 0): pack(1.0, 0)}, nb={0: 5.0, 2: 0.2},
        expect={(2, 0): pack(hop_score(1.0, 1, 0.2, 0.9), 2)},
    )
    cases["guard_slot1"] = _case(
        3, cyc, cur={(1, 1): pack(1.0, 0)}, nb={0: 5.0, 2: 0.2},
        expect={(2, 1): pack(hop_score(1.0, 1, 0.2, 0.9), 2)},
    )
    # a seed label has no predecessor and is never blocked
    cases["guard_seed_not_blocked"] = _case(
        3, cyc, cur={(1, 0): SEED}, nb={0: 5.0, 2: 0.2},
        expect={(0, 0): pack(hop_score(0.0, 0, 5.0, 1.3), 1),
                (2, 0): pack(hop_score(0.0, 1, 0.2, 0.9), 2)},
    )
    # the guard is per label: slot 0 came from node 0 (over e0), slot 1 from
    # node 2 (over e3: 2->1), so each edge carries exactly one of the two
    cases["guard_per_slot"] = _case(
        3, cyc + [(2, 1, 0, 0.6)],
        cur={(1, 0): pack(1.0, 0), (1, 1): pack(2.0, 3)}, nb={0: 5.0, 2: 0.2},
        expect={(0, 1): pack(hop_score(2.0, 0, 5.0, 1.3), 1),
                (2, 0): pack(hop_score(1.0, 1, 0.2, 0.9), 2)},
    )

    # Gate propagation.  Node 0 holds a slot-0 seed, node 1 a slot-1 label
    # that came over e4 from node 4.
    #   e0: 0->2 gate edge            -> (2, 1)
    #   e1: 0->3 plain, node 3 gated  -> (3, 1)
    #   e2: 0->5 plain, plain node    -> (5, 0)
    #   e3: 1->5 plain, slot-1 label  -> (5, 1)
    #   e4: 4->1 source unlabelled    -> nothing
    gate_edges = [(0, 2, 2, 0.7), (0, 3, 0, 1.9), (0, 5, 0, 0.35),
                  (1, 5, 1, 0.45), (4, 1, 0, 1.0)]
    gate_cur = {(0, 0): SEED, (1, 1): pack(1.25, 4)}
    gate_nb = {2: 0.1, 3: 0.6, 5: 1.1}
    cases["gate_propagation"] = _case(
        6, gate_edges, cur=gate_cur, nb=gate_nb, ng=[3],
        expect={(2, 1): pack(hop_score(0.0, 2, 0.1, 0.7), 0),
                (3, 1): pack(hop_score(0.0, 0, 0.6, 1.9), 1),
                (5, 0): pack(hop_score(0.0, 0, 1.1, 0.35), 2),
                (5, 1): pack(hop_score(1.25, 1, 1.1, 0.45), 3)},
    )
    # the same graph without a node_gate array: node 3 no longer gates
    cases["gate_propagation_no_node_gate"] = _case(
        6, gate_edges, cur=gate_cur, nb=gate_nb, ng=None,
        expect={(2, 1): pack(hop_score(0.0, 2, 0.1, 0.7), 0),
                (3, 0): pack(hop_score(0.0, 0, 0.6, 1.9), 1),
                (5, 0): pack(hop_score(0.0, 0, 1.1, 0.35), 2),
                (5, 1): pack(hop_score(1.25, 1, 1.1, 0.45), 3)},
    )

    # A non-traversable type contributes nothing, whatever its boost/weight.
    cases["non_traversable_edge"] = _case(
        3, [(0, 1, 4, 2.0), (0, 2, 0, 0.7), (0, 2, 5, 1.9)],
        cur={(0, 0): SEED, (0, 1): pack(3.0, NO_EDGE)}, nb={1: 1.0, 2: 0.4},
        expect={(2, 0): pack(hop_score(0.0, 0, 0.4, 0.7), 1),
                (2, 1): pack(hop_score(3.0, 0, 0.4, 0.7), 1)},
    )

    # A source whose two labels are both zero contributes nothing.
    cases["unlabelled_source"] = _case(
        4, [(0, 2, 2, 1.9), (1, 3, 0, 0.7), (0, 3, 0, 1.9)],
        cur={(1, 0): SEED}, nb={2: 2.0, 3: 0.4},
        expect={(3, 0): pack(hop_score(0.0, 0, 0.4, 0.7), 1)},
    )
    return cases


def random_weights(rng, num_edges: int) -> np.ndarray:
    """f32 weights uniform in [0, 2); about a quarter exactly 1.0 (the graph
    default) and a few exactly 0.0."""
    w = (rng.random(num_edges) * 2).astype(np.float32)
    w[rng.random(num_edges) < 0.25] = 1.0
    if num_edges >= 8:
        w[rng.integers(0, num_edges, size=max(1, num_edges // 500))] = 0.0
    return w


def random_graph(num_nodes: int, num_edges: int, num_entries: int, seed: int) -> dict:
    """Random multigraph with etype in 0..5, boosts in [0, 2) and weights."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, num_nodes, size=num_edges).astype(np.int32)
    dst = rng.integers(0, num_nodes, size=num_edges).astype(np.int32)
    et = rng.integers(0, 6, size=num_edges).astype(np.uint8)
    nb = (rng.random(num_nodes) * 2).astype(np.float32)
    ng = (rng.random(num_nodes) < 0.1).astype(np.uint8)
    w = random_weights(rng, num_edges)
    entries = np.sort(rng.choice(num_nodes, size=min(num_entries, num_nodes),
                                 replace=False)).astype(np.int64)
    cur = np.zeros(num_nodes * 2, dtype=np.uint64)
    cur[entries * 2] = np.uint64(SEED)
    return dict(n=num_nodes, src=src, dst=dst, et=et, w=w, nb=nb, ng=ng,
                cur=cur, entries=entries)


def layered_dag(layers: int, width: int, num_edges: int, seed: int) -> dict:
    """Random DAG: every edge goes from a layer to one of the next two."""
    rng = np.random.default_rng(seed)
    n = layers * width
    lay = rng.integers(0, layers - 1, size=num_edges)
    jump = np.minimum(lay + 1 + rng.integers(0, 2, size=num_edges), layers - 1)
    src = (lay * width + rng.integers(0, width, size=num_edges)).astype(np.int32)
    dst = (jump * width + rng.integers(0, width, size=num_edges)).astype(np.int32)
    et = rng.integers(0, 6, size=num_edges).astype(np.uint8)
    nb = (rng.random(n) * 2).astype(np.float32)
    ng = (rng.random(n) < 0.1).astype(np.uint8)
    w = random_weights(rng, num_edges)
    entries = np.arange(0, width, 8, dtype=np.int64)  # a slice of layer 0
    tm = np.zeros(n, dtype=np.uint8)
    tm[(layers - 3) * width:] = 1
    return dict(n=n, src=src, dst=dst, et=et, w=w, nb=nb, ng=ng,
                entries=entries, tm=tm)
