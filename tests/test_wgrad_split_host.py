"""CPU-only: the K split of the grouped weight-gradient ring launches, through the C ABI queries that run the very range
function the kernels run (rfn_wgrad_split_parts) and the launchers' workgroup count (rfn_wgrad_split_workgroups).  The
flat stage space of one output tile is G * n_stages stages, group g owning [g * n_stages, (g + 1) * n_stages); workgroup
w of Wt owns [w T / Wt, (w + 1) T / Wt) and processes it as parts that never cross a group."""
import ctypes
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recurrent-flows-msc_amd"))

MAX_PARTS = 32  # a range can touch at most G <= 16 groups


def _parts(L, G, n_stages, Wt, w):
    buf = (ctypes.c_longlong * (3 * MAX_PARTS))()
    n = L.rfn_wgrad_split_parts(G, n_stages, Wt, w, buf, MAX_PARTS)
    assert 0 <= n <= MAX_PARTS, (G, n_stages, Wt, w, n)
    return [(int(buf[3 * i]), int(buf[3 * i + 1]), int(buf[3 * i + 2])) for i in range(n)]


def _check_split(L, G, n_stages, Wt):
    """every (group, stage) exactly once, no part across a group, totals within one stage of each other, parts of a
    workgroup in increasing order -- and, beyond the issue's list, the ranges themselves contiguous and in w order"""
    owner = [bytearray(n_stages) for _ in range(G)]
    totals = []
    nxt = 0  # flat position the next part must start at: ranges tile the flat space in (w, part) order
    for w in range(Wt):
        parts = _parts(L, G, n_stages, Wt, w)
        tot = 0
        for (g, s0, cnt) in parts:
            assert 0 <= g < G and cnt >= 1 and 0 <= s0 and s0 + cnt <= n_stages, (G, n_stages, Wt, w, parts)
            assert g * n_stages + s0 == nxt, (G, n_stages, Wt, w, parts)   # increasing, contiguous
            nxt += cnt
            tot += cnt
            row = owner[g]
            for s in range(s0, s0 + cnt):
                assert row[s] == 0, ("stage owned twice", G, n_stages, Wt, w, g, s)
                row[s] = 1
        assert [p[0] for p in parts] == sorted(set(p[0] for p in parts)), ("one part per group, ascending", parts)
        totals.append(tot)
    assert nxt == G * n_stages
    assert all(all(row) for row in owner), ("stage not owned", G, n_stages, Wt)
    assert max(totals) - min(totals) <= 1, (G, n_stages, Wt, min(totals), max(totals))
    return totals


def test_random_splits_cover_every_stage_once():
    from rfn_hip import lib
    L = lib.load()
    rng = random.Random(20240611)
    cases = [(rng.randint(1, 16), rng.randint(1, 5000), rng.randint(1, 256)) for _ in range(120)]
    # more workgroups than stages (empty ranges), the extremes, and exact divisions
    cases += [(1, 1, 256), (3, 5, 256), (16, 1, 255), (2, 100, 256), (16, 5000, 256), (16, 5000, 1), (1, 5000, 7),
              (4, 64, 256), (4, 64, 128), (2, 512, 128), (7, 13, 91), (7, 13, 92)]
    assert any(Wt > G * n for (G, n, Wt) in cases)
    for (G, n_stages, Wt) in cases:
        totals = _check_split(L, G, n_stages, Wt)
        if Wt > G * n_stages:
            assert min(totals) == 0 and max(totals) == 1


@pytest.mark.parametrize("n_stages", [19456, 4864, 1216])   # levels 0, 1, 2 of the bench step: 608 frames of 32x32 ...
@pytest.mark.parametrize("tiles", [1, 2])                   # one and two column tiles
def test_bench_step_shapes(n_stages, tiles):
    from rfn_hip import lib
    L = lib.load()
    G = 10
    Wt = L.rfn_wgrad_split_workgroups(tiles, G, n_stages)
    assert Wt == 256 // tiles                                # every CU has a workgroup
    totals = _check_split(L, G, n_stages, Wt)
    T = G * n_stages
    assert min(totals) >= T // Wt and max(totals) <= -(-T // Wt)
    # at most one boundary per workgroup at these shapes, and G - 1 workgroups at most flush twice
    nparts = [len(_parts(L, G, n_stages, Wt, w)) for w in range(Wt)]
    assert max(nparts) <= 2 and sum(n - 1 for n in nparts) <= G - 1


def test_workgroup_count_keeps_eight_stages_each():
    from rfn_hip import lib
    L = lib.load()
    assert L.rfn_wgrad_split_workgroups(1, 2, 512) == 128     # 1024 stages: 256 workgroups would get 4 each
    assert L.rfn_wgrad_split_workgroups(1, 10, 320) == 256
    assert L.rfn_wgrad_split_workgroups(2, 4, 800) == 128
    assert L.rfn_wgrad_split_workgroups(1, 1, 64) == 8        # an ungrouped launch: min(256 / tiles, n_stages / 8)
    assert L.rfn_wgrad_split_workgroups(1, 1, 3) == 1
    assert L.rfn_wgrad_split_workgroups(300, 1, 4096) == 1
    assert L.rfn_wgrad_split_workgroups(0, 1, 8) < 0 and L.rfn_wgrad_split_parts(17, 8, 1, 0, None, 0) < 0
    assert L.rfn_wgrad_split_parts(2, 8, 4, 4, None, 0) < 0   # w out of range
