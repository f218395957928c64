"""CPU side of the reachability query (fiesta_hip_reach_field, include/fiesta_hip.h): the definition.

fiesta_amd.reach_model (traversability in numpy, then a heap Dijkstra) is the model the GPU tests compare the kernels with, so it
must be the header's definition: it is checked against an independent Bellman-Ford -- a plain triple loop over the voxels, repeated
until nothing changes -- on random 9 x 8 x 11 arrays, and on hand cases whose answers are known.  Everything is integer: comparisons
are exact.  Also: the whole-call argument rules that the library checks before it touches a device, the ctypes mirrors of the two
structs, and that the k_reach_* kernels use no scratch and spill nothing.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fiesta_amd.reach_model import REACH_THROUGH_UNKNOWN, reach_model, reach_moves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (9, 8, 11)
INF = 2 ** 31 - 1


def loop_model(observed, occupied, seeds, dist=None, lo=None, hi=None, min_clearance=0.0, connectivity=26, flags=0, origin_vox=(0, 0, 0)):
    """the header's definition, voxel by voxel: traversable(v), then Bellman-Ford over the moves; returns the cost array of the
    clipped box and the number of usable seed entries"""
    nx, ny, nz = observed.shape
    o = origin_vox
    b0 = [0, 0, 0] if lo is None else [max(lo[c] - o[c], 0) for c in range(3)]
    b1 = [nx - 1, ny - 1, nz - 1] if hi is None else [min(hi[c] - o[c], observed.shape[c] - 1) for c in range(3)]
    if any(b0[c] > b1[c] for c in range(3)):
        return np.zeros((0, 0, 0), np.int32), 0
    ex, ey, ez = (b1[c] - b0[c] + 1 for c in range(3))
    cost = np.full((ex, ey, ez), -1, np.int64)
    for i in range(ex):
        for j in range(ey):
            for k in range(ez):
                a, b, c = i + b0[0], j + b0[1], k + b0[2]
                free = observed[a, b, c] and not occupied[a, b, c]
                if free and min_clearance > 0:
                    free = dist[a, b, c] >= min_clearance
                if free or ((flags & 1) and not observed[a, b, c]):
                    cost[i, j, k] = INF
    used = 0
    for s in seeds:
        i, j, k = (int(s[c]) - o[c] - b0[c] for c in range(3))
        if 0 <= i < ex and 0 <= j < ey and 0 <= k < ez and cost[i, j, k] >= 0:
            cost[i, j, k] = 0
            used += 1
    moves = [(dx, dy, dz, 2 + abs(dx) + abs(dy) + abs(dz)) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    changed = True
    while changed:
        changed = False
        for i in range(ex):
            for j in range(ey):
                for k in range(ez):
                    if cost[i, j, k] <= 0:                 # (blocked, or a seed)
                        continue
                    for dx, dy, dz, w in moves:
                        a, b, c = i + dx, j + dy, k + dz
                        if 0 <= a < ex and 0 <= b < ey and 0 <= c < ez and 0 <= cost[a, b, c] < INF and cost[a, b, c] + w < cost[i, j, k]:
                            cost[i, j, k] = cost[a, b, c] + w
                            changed = True
    return cost.astype(np.int32), used


def random_scene(seed):
    rng = np.random.RandomState(seed)
    obs = rng.rand(*SHAPE) < (0.55, 0.75, 0.95)[seed % 3]
    occ = rng.rand(*SHAPE) < 0.25          # (also on unobserved voxels: unknown whatever their bit says)
    dist = rng.choice([0.0, 0.1, 0.2, 0.3, 0.5, 10000.0], SHAPE)
    return rng, obs, occ, dist


@pytest.mark.parametrize("seed", range(6))
def test_model_is_the_definition_on_random_arrays(seed):
    rng, obs, occ, dist = random_scene(seed)
    org = tuple(int(v) for v in rng.randint(-20, 20, 3))
    seeds = rng.randint(-1, np.array(SHAPE) + 1, (8, 3)) + org      # some outside, some on blocked voxels, maybe repeated
    seeds = np.concatenate([seeds, seeds[:1]])
    boxes = [(None, None), (np.array((1, 2, 1)) + org, np.array((7, 6, 9)) + org), (np.array((-3, -3, 4)) + org, np.array((30, 30, 30)) + org),
             (np.array((3, 3, 3)) + org, np.array((2, 9, 9)) + org)]
    finite = 0
    for conn in (6, 26):
        for flags in (0, REACH_THROUGH_UNKNOWN):
            for clr in (0.0, 0.25):
                # the whole array with every combination, each other box with one of them
                for lo, hi in boxes[:1] + [boxes[1 + (conn // 26 + flags + int(clr > 0)) % 3]]:
                    want, used = loop_model(obs, occ, seeds, dist, lo, hi, clr, conn, flags, org)
                    got = reach_model(obs, occ, seeds, dist, lo, hi, clr, conn, flags, origin_vox=org)
                    assert got["cost"].dtype == np.int32 and got["cost"].shape == want.shape
                    assert np.array_equal(got["cost"], want), (conn, flags, clr, lo, hi)
                    assert got["n_seeds_used"] == used
                    assert got["n_traversable"] == int((want >= 0).sum())
                    reached = (want >= 0) & (want < INF)
                    assert got["n_reached"] == int(reached.sum()) and got["max_cost"] == (int(want[reached].max()) if reached.any() else 0)
                    finite += int((reached & (want > 0)).sum())
    assert finite > 0
    # without a clearance the distances are not read
    assert np.array_equal(reach_model(obs, occ, seeds, None, origin_vox=org)["cost"], reach_model(obs, occ, seeds, dist, min_clearance=-1.0, origin_vox=org)["cost"])


def test_moves_are_the_chamfer():
    assert sorted(w for *_, w in reach_moves(6)) == [3] * 6
    assert sorted(w for *_, w in reach_moves(26)) == [3] * 6 + [4] * 12 + [5] * 8
    with pytest.raises(ValueError):
        reach_moves(18)


def test_three_four_five_on_an_empty_block():
    obs = np.ones((7, 6, 9), bool)
    occ = np.zeros_like(obs)
    c26 = reach_model(obs, occ, [(1, 2, 3)], connectivity=26)["cost"]
    c6 = reach_model(obs, occ, [(1, 2, 3)], connectivity=6)["cost"]
    for v in ((1, 2, 3), (2, 2, 3), (2, 3, 3), (2, 3, 4), (6, 5, 8), (0, 0, 0), (4, 2, 8), (6, 2, 3)):
        d = sorted(abs(a - b) for a, b in zip(v, (1, 2, 3)))
        assert c26[v] == 5 * d[0] + 4 * (d[1] - d[0]) + 3 * (d[2] - d[1]), v     # diagonal steps first, the rest straight
        assert c6[v] == 3 * sum(d), v
    r = reach_model(obs, occ, [(1, 2, 3)], targets=[(6, 5, 8), (7, 0, 0), (1, 2, 3)])
    assert r["target_cost"].tolist() == [5 * 3 + 4 * 2 + 3 * 0, -1, 0] and r["max_cost"] == int(c26.max())
    assert r["box_lo"] == [0, 0, 0] and r["box_hi"] == [6, 5, 8] and r["n_traversable"] == r["n_reached"] == obs.size


def test_pocket_door_and_diagonal_gap():
    obs = np.ones(SHAPE, bool)
    occ = np.zeros(SHAPE, bool)
    # an enclosed pocket: a 5 x 5 x 5 shell around a 3 x 3 x 3 room
    occ[2:7, 1:6, 3:8] = True
    occ[3:6, 2:5, 4:7] = False
    inside = reach_model(obs, occ, [(4, 3, 5)])
    assert inside["n_reached"] == 27 and inside["max_cost"] == 5
    c = inside["cost"]
    assert c[0, 0, 0] == INF and c[2, 1, 3] == -1 and c[4, 3, 5] == 0 and c[3, 2, 4] == 5
    outside = reach_model(obs, occ, [(0, 0, 0)])
    assert outside["n_reached"] == obs.size - 125 and outside["cost"][4, 3, 5] == INF
    assert reach_model(obs, occ, [(0, 0, 0), (4, 3, 5)])["n_reached"] == obs.size - 125 + 27
    # a wall across x with a one-voxel door
    occ[:] = False
    occ[4] = True
    far = reach_model(obs, occ, [(0, 0, 0)], connectivity=6)
    assert far["n_reached"] == 4 * 8 * 11 and far["cost"][8, 7, 10] == INF
    occ[4, 6, 9] = False
    for conn, want in ((6, 3 * (8 + 6 + 9) + 3 * (1 + 1)), (26, None)):
        r = reach_model(obs, occ, [(0, 0, 0)], connectivity=conn)
        assert r["n_reached"] == obs.size - (8 * 11 - 1) and r["cost"][4, 6, 9] > 0
        if want:
            assert r["cost"][8, 7, 10] == want              # through the door, no shorter way
    # a diagonal gap: two free voxels that touch by an edge only
    occ[:] = True
    occ[2, 3, 5] = occ[3, 4, 5] = False
    assert reach_model(obs, occ, [(2, 3, 5)], connectivity=26)["cost"][3, 4, 5] == 4
    assert reach_model(obs, occ, [(2, 3, 5)], connectivity=6)["cost"][3, 4, 5] == INF
    occ[3, 4, 5], occ[3, 4, 6] = True, False               # ... by a corner only
    assert reach_model(obs, occ, [(2, 3, 5)], connectivity=26)["cost"][3, 4, 6] == 5


def test_unknown_clearance_and_box_rules():
    obs = np.ones(SHAPE, bool)
    occ = np.zeros(SHAPE, bool)
    obs[4] = False                                          # an unknown slab splits the block
    assert reach_model(obs, occ, [(0, 0, 0)])["cost"][8, 0, 0] == INF and reach_model(obs, occ, [(0, 0, 0)])["cost"][4, 0, 0] == -1
    thru = reach_model(obs, occ, [(0, 0, 0)], flags=REACH_THROUGH_UNKNOWN)
    assert thru["cost"][8, 0, 0] == 24 and thru["cost"][4, 0, 0] == 12 and thru["n_traversable"] == obs.size
    occ[4, 2, 2] = True                                     # a stale occupancy bit on an unknown voxel: still unknown
    assert reach_model(obs, occ, [(0, 0, 0)], flags=REACH_THROUGH_UNKNOWN)["cost"][4, 2, 2] == 5 * 2 + 3 * 2
    # the clearance applies to observed voxels only; +10000 passes; a seed that fails it is ignored
    dist = np.full(SHAPE, 10000.0)
    dist[2] = 0.1
    r = reach_model(obs, occ, [(0, 0, 0), (2, 0, 0)], dist, min_clearance=0.25, flags=REACH_THROUGH_UNKNOWN)
    assert r["n_seeds_used"] == 1 and r["cost"][2, 1, 1] == -1 and r["cost"][3, 0, 0] == INF and r["cost"][4, 0, 0] == INF
    assert reach_model(obs, occ, [(0, 0, 0)], dist, min_clearance=9999.0)["n_reached"] == 2 * 8 * 11
    # a box face that cuts the only route: the cut route is no route; a seed outside the box is ignored
    obs[:] = True
    occ[:] = False
    occ[4, :7] = True                                       # the door of this wall is the row y = 7
    assert reach_model(obs, occ, [(0, 0, 0)])["cost"][8, 0, 0] < INF
    cut = reach_model(obs, occ, [(0, 0, 0), (0, 7, 0)], lo=(0, 0, 0), hi=(8, 6, 10))
    assert cut["cost"].shape == (9, 7, 11) and cut["cost"][8, 0, 0] == INF and cut["n_seeds_used"] == 1
    assert cut["box_lo"] == [0, 0, 0] and cut["box_hi"] == [8, 6, 10]
    # empty boxes, no seeds, argument rules
    e = reach_model(obs, occ, [(0, 0, 0)], lo=(3, 3, 3), hi=(2, 9, 9), targets=[(3, 3, 3)])
    assert e["cost"].size == 0 and e["target_cost"].tolist() == [-1] and e["n_traversable"] == 0 and e["box_hi"] == [0, 0, 0]
    n = reach_model(obs, occ, np.zeros((0, 3), np.int32))
    assert n["n_reached"] == 0 and n["max_cost"] == 0 and (n["cost"][~occ] == INF).all()
    for bad in (dict(lo=(0, 0, 0)), dict(connectivity=18), dict(flags=2), dict(min_clearance=float("nan"))):
        with pytest.raises(ValueError):
            reach_model(obs, occ, [(0, 0, 0)], **bad)


def test_struct_mirrors_follow_the_header():
    from fiesta_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    for struct, mirror in (("fiesta_hip_reach_result", _lib.ReachResult), ("fiesta_hip_reach_info", _lib.ReachInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"\[.*?\]", "", n).strip(" *") for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(_lib.ReachInfo) == 6 * 4 + 6 * 8 and C.sizeof(_lib.ReachResult) == 2 * C.sizeof(C.c_void_p)
    assert re.search(r"#define FIESTA_HIP_REACH_THROUGH_UNKNOWN (\d+)", text).group(1) == str(REACH_THROUGH_UNKNOWN)


def test_argument_rules_are_checked_before_any_device_use():
    """every whole-call error that needs no map is refused -- with its own message -- before the handle is looked at: the calls below
    pass no map at all, on a machine that may have no GPU"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    box = (C.c_int32 * 3)(0, 0, 0)
    pts = (C.c_int32 * 3)(1, 1, 1)
    out = (C.c_int32 * 1)(77)
    res = _lib.ReachResult(None, None)
    res_t = _lib.ReachResult(None, C.cast(out, C.c_void_p))
    nan = float("nan")
    #        lo   hi   seeds n  targets n  clearance conn flags result        the message names
    cases = [(box, box, pts, 1, None, 0, 0.0, 26, 0, None, "result"),
             (box, box, pts, 1, None, 0, nan, 26, 0, res, "NaN"),
             (box, None, pts, 1, None, 0, 0.0, 26, 0, res, "lo and hi"),
             (None, box, pts, 1, None, 0, 0.0, 26, 0, res, "lo and hi"),
             (box, box, pts, 1, None, 0, 0.0, 18, 0, res, "connectivity"),
             (box, box, pts, 1, None, 0, 0.0, 0, 0, res, "connectivity"),
             (box, box, pts, 1, None, 0, 0.0, 26, 2, res, "flag"),
             (box, box, pts, 1, None, 0, 0.0, 26, -1, res, "flag"),
             (box, box, pts, -1, None, 0, 0.0, 26, 0, res, "negative"),
             (box, box, pts, 1, pts, -1, 0.0, 26, 0, res, "negative"),
             (box, box, None, 1, None, 0, 0.0, 26, 0, res, "seeds"),
             (box, box, pts, 1, None, 1, 0.0, 26, 0, res, "targets"),
             (box, box, pts, 1, None, 0, 0.0, 26, 0, res_t, "target_cost"),
             (box, box, pts, 1, pts, 1, 0.0, 26, 1, res_t, "null map")]      # nothing wrong but the missing map
    for fn in (lib.fiesta_hip_reach_field, lib.fiesta_hip_reach_field_dev):
        for lo, hi, seeds, ns, targets, nt, clr, conn, flags, r, word in cases:
            st = fn(None, lo, hi, seeds, ns, targets, nt, clr, conn, flags, C.byref(r) if r is not None else None, None)
            assert st == 1, (word, st)                                       # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    assert out[0] == 77


def test_reach_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_reach_" in k}
    for kernel, copies in (("k_reach_mask", 2), ("k_reach_seed", 1), ("k_reach_relax", 2), ("k_reach_targets", 1), ("k_reach_stats", 1)):
        assert sum(kernel in k for k in res) == copies, (kernel, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
