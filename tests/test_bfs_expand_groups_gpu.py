"""bfs_expand_kernel over frontiers that a sub-wave group layout would split
unevenly: out-degrees around a group of eight lanes and up to the heavy
threshold, frontier sizes that leave a partial group in the last wave and the
last block, and many vertices on the same few targets.  dist is compared with
cpu_ref.bfs exactly, next frontiers as sets.  (The eight-lane kernel these
cases were written for was measured slower and is not in the tree, see
profiles/r11_bfs_parent_index.md; they hold for any layout of the expand.)
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from bfs_graphs import UNVISITED, csr, fan_edges

pytestmark = pytest.mark.gpu

DEGREES = [7, 8, 9, 15, 16, 17, 63]
FRONTIERS = [1, 31, 32, 33, 255, 256, 257]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fan(frontier, degree, dev):
    from agentbom_amd.ops import cpu_ref

    src, dst, n = fan_edges(frontier, degree)
    fwd = csr(src, dst, np.zeros(len(src)), n)
    ref = cpu_ref.bfs(fwd["row_off"], fwd["col"], np.asarray([0]), n, etype=fwd["etype"])
    return {"fwd": {k: torch.from_numpy(v).to(dev) for k, v in fwd.items()}, "n": n,
            "frontier": frontier, "ref": ref}


@pytest.fixture(scope="module")
def fans(dev):
    return {(f, d): _fan(f, d, dev) for f in FRONTIERS for d in DEGREES}


@pytest.fixture(scope="module")
def shared_targets(dev):
    """10k frontier vertices that all point at the same 3 targets."""
    from agentbom_amd.ops import cpu_ref

    f = 10_000
    src = np.concatenate([np.zeros(f, dtype=np.int64),
                          np.repeat(np.arange(1, f + 1, dtype=np.int64), 3)])
    dst = np.concatenate([np.arange(1, f + 1, dtype=np.int64),
                          np.tile(f + 1 + np.arange(3, dtype=np.int64), f)])
    n = f + 4
    fwd = csr(src, dst, np.zeros(len(src)), n)
    ref = cpu_ref.bfs(fwd["row_off"], fwd["col"], np.asarray([0]), n, etype=fwd["etype"])
    return {"fwd": {k: torch.from_numpy(v).to(dev) for k, v in fwd.items()}, "n": n,
            "frontier": f, "ref": ref}


def _check_bfs(g, dev):
    from agentbom_amd.ops import native

    fwd = g["fwd"]
    dist = native.bfs(fwd["row_off"], fwd["col"], torch.zeros(1, dtype=torch.int32, device=dev),
                      g["n"], etype=fwd["etype"])
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), g["ref"])


def _check_level_two(g, dev):
    """bfs_level from the level-1 frontier: the claims, each once."""
    from agentbom_amd.ops import native

    f, fwd = g["frontier"], g["fwd"]
    dist = np.full(g["n"], UNVISITED, dtype=np.uint32)
    dist[0], dist[1:f + 1] = 0, 1
    dist_t = torch.from_numpy(dist.view(np.int32)).to(dev)
    frontier = torch.arange(1, f + 1, dtype=torch.int32, device=dev)
    nxt = native.bfs_level(fwd["row_off"], fwd["col"], frontier, dist_t, 2,
                           etype=fwd["etype"]).cpu().numpy()
    want = np.flatnonzero(g["ref"] == 2)
    assert len(nxt) == len(want)
    assert set(nxt.tolist()) == set(want.tolist())
    assert np.array_equal(dist_t.cpu().numpy().view(np.uint32), g["ref"])


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("frontier", FRONTIERS)
def test_fans(fans, dev, frontier, degree):
    g = fans[(frontier, degree)]
    assert int((g["ref"] == 2).sum()) == frontier * degree
    _check_bfs(g, dev)
    _check_level_two(g, dev)


def test_shared_targets(shared_targets, dev):
    g = shared_targets
    assert int((g["ref"] == 2).sum()) == 3
    _check_bfs(g, dev)
    _check_level_two(g, dev)


def test_mixed_degrees_and_masked_edges(dev):
    """One frontier with every degree from 0 to 70 (the heavy queue takes 64
    and up) and every third edge of a masked type."""
    from agentbom_amd.ops import cpu_ref, native

    degs = np.arange(71, dtype=np.int64)
    f = len(degs)
    src = np.concatenate([np.zeros(f, dtype=np.int64),
                          np.repeat(np.arange(1, f + 1, dtype=np.int64), degs)])
    dst = np.concatenate([np.arange(1, f + 1, dtype=np.int64),
                          f + 1 + np.arange(degs.sum(), dtype=np.int64)])
    et = np.zeros(len(src), dtype=np.uint8)
    et[f::3] = 5
    n = 1 + f + int(degs.sum())
    fwd = csr(src, dst, et, n)
    ref = cpu_ref.bfs(fwd["row_off"], fwd["col"], np.asarray([0]), n, etype=fwd["etype"],
                      allowed_mask=0x1)
    assert 0 < int((ref == 2).sum()) < int(degs.sum())
    fwd_d = {k: torch.from_numpy(v).to(dev) for k, v in fwd.items()}
    dist = native.bfs(fwd_d["row_off"], fwd_d["col"],
                      torch.zeros(1, dtype=torch.int32, device=dev), n, etype=fwd_d["etype"],
                      allowed_mask=0x1)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), ref)
