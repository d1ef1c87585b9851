"""CPU: rala_hip_layout_split - how the points of a layout batch are shared out over the ranks of a sharded run (no context, no
device).  Units in point order: a component of at most fused_max points is one unit of cost n^2, a larger one its tiles of 256
points at (points in the tile) * n each; part k ends behind the first unit at which the prefix cost reaches
ceil(total * (k + 1) / parts)."""
import numpy as np
import pytest

from rala_amd import hip

import layout_ranks as lr

SUITE = (1, 6, 7, 63, 64, 65, 255, 256, 257, 300, 1023, 1024, 1025, 1300)
FUSED = (0, 64, 1024)
PARTS = tuple(range(1, 10))


def _size_lists():
    rng = np.random.default_rng(22)
    lists = [SUITE, (0,) + SUITE, SUITE + (0,), SUITE[:7] + (0, 0) + SUITE[7:], SUITE[::-1], (1300,), (0, 0, 0), (), (5,),
             (1024, 1024, 1024), (257,) * 5]
    for _ in range(12):
        n = int(rng.integers(1, 40))
        sizes = rng.choice([0, 1, 2, 5, 64, 200, 256, 257, 700, 1024, 1025, 3000], size=n)
        sizes = [int(s) if rng.random() < 0.7 else int(rng.integers(0, 2000)) for s in sizes]
        lists.append(tuple(sizes))
    return lists


def _comp_off(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.uint32)
    np.cumsum(np.asarray(sizes, dtype=np.uint32), out=off[1:])
    return off


@pytest.mark.parametrize("fused_max", FUSED)
def test_split_properties(fused_max):
    for sizes in _size_lists():
        n_all = sum(sizes)
        us = lr.units(sizes, fused_max)
        total = sum(u[1] for u in us)
        assert total == sum(n * n for n in sizes)
        edges = {0} | {u[0] for u in us}                    # where a cut may lie: unit boundaries
        largest = max([u[1] for u in us], default=0)
        for parts in PARTS:
            got = hip.layout_split(_comp_off(sizes), fused_max, parts)
            assert got is not None, (sizes, fused_max, parts)
            first, cost = got
            # ascending, contiguous, covering [0, N)
            assert len(first) == parts + 1 and first[0] == 0 and first[-1] == n_all
            assert all(a <= b for a, b in zip(first, first[1:]))
            # no cut inside a fused component or off a tile boundary (N itself is the end of the last unit, or 0)
            assert all(f in edges for f in first), (sizes, fused_max, parts, first)
            # the costs are the parts' and sum to the total
            assert sum(cost) == total
            for k in range(parts):
                assert cost[k] == sum(u[1] for u in us if first[k] < u[0] <= first[k + 1])
                assert cost[k] <= -(-total // parts) + largest, (sizes, fused_max, parts, k)
            # ... and the whole answer is the rule's
            assert (first, cost) == lr.split(sizes, fused_max, parts), (sizes, fused_max, parts)
            # cost may be NULL
            assert hip.layout_split(_comp_off(sizes), fused_max, parts, with_cost=False)[0] == first


def test_one_component_of_1300_points_over_8_parts():
    for fused_max in FUSED:
        first, cost = hip.layout_split(_comp_off((1300,)), fused_max, 8)
        empty = [k for k in range(8) if first[k] == first[k + 1]]
        assert len(empty) == 2, first
        assert all(cost[k] == 0 for k in empty)
        assert all(f % 256 == 0 or f == 1300 for f in first)
        assert 0 < first[1] < 1300                          # the cuts lie inside the component


def test_fused_components_stay_whole():
    sizes = (1000, 1000, 1000)
    first, cost = hip.layout_split(_comp_off(sizes), 1024, 3)
    assert first == [0, 1000, 2000, 3000] and cost == [10 ** 6] * 3
    first, cost = hip.layout_split(_comp_off(sizes), 1024, 6)
    assert set(first) == {0, 1000, 2000, 3000} and sorted(cost) == [0, 0, 0] + [10 ** 6] * 3
    first, _ = hip.layout_split(_comp_off(sizes), 0, 6)     # as tiles they do not
    assert any(f % 1000 for f in first)


def test_refusals():
    ok = _comp_off((5, 300, 0, 7))
    assert hip.layout_split(ok, 1024, 3) is not None
    assert hip.layout_split(ok, 1024, 0) is None                                # no parts
    assert hip.layout_split(ok, 1025, 3) is None                                # fused_max beyond a workgroup
    bad = ok.copy()
    bad[0] = 1
    assert hip.layout_split(bad, 1024, 3) is None                               # does not start at 0
    bad = ok.copy()
    bad[1], bad[2] = ok[2], ok[1]
    assert hip.layout_split(bad, 1024, 3) is None                               # decreases
    L = hip.lib()
    first = np.zeros(4, dtype=np.uint32)
    assert L.rala_hip_layout_split(4, None, 1024, 3, first.ctypes.data, None) == -2          # components without offsets
    assert L.rala_hip_layout_split(4, ok.ctypes.data, 1024, 3, None, None) == -2             # nowhere to write
    assert L.rala_hip_layout_split(0, None, 1024, 3, first.ctypes.data, None) == 0 and list(first) == [0, 0, 0, 0]
