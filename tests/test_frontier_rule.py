"""CPU side of the frontier extraction (fiesta_hip_get_frontier_voxels, include/fiesta_hip.h): the definition.

fiesta_amd.frontier_model (numpy, shifted-array comparisons) is the model the GPU tests compare the kernels with, so it must be the
header's definition: it is checked against a literal triple loop over that definition, one voxel at a time, on random 9 x 7 x 11
arrays and on the special cases the header names.  Everything is integer or boolean: comparisons are exact.  Also: the library's
two frontier kernels use no scratch.

The bits of the mask: 0 is -x, 1 is +x, 2 is -y, 3 is +y, 4 is -z, 5 is +z.  A lone observed voxel at the low corner of a bounded
array therefore has mask 42 (+x, +y, +z: its other three neighbours are outside, and outside is not unknown), at the high corner
its mirror image 21.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (9, 7, 11)
DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def loop_model(observed, occupied, dist=None, lo=None, hi=None, min_clearance=0.0, origin_vox=(0, 0, 0), bounded=True):
    """the header's definition, voxel by voxel"""
    nx, ny, nz = observed.shape
    rows = []
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                if not observed[i, j, k] or occupied[i, j, k]:
                    continue
                u = 0
                for bit, (dx, dy, dz) in enumerate(DIRS):
                    a, b, c = i + dx, j + dy, k + dz
                    if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz:
                        unknown = not observed[a, b, c]
                    else:
                        unknown = not bounded
                    u |= int(unknown) << bit
                if u == 0:
                    continue
                v = (i + origin_vox[0], j + origin_vox[1], k + origin_vox[2])
                if lo is not None and not all(lo[c] <= v[c] <= hi[c] for c in range(3)):
                    continue
                if min_clearance > 0 and not dist[i, j, k] >= min_clearance:
                    continue
                rows.append(v + (u,))
    rows.sort()
    a = np.array(rows, np.int64).reshape(-1, 4)
    return a[:, :3].astype(np.int32), a[:, 3].astype(np.uint8)


def same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.uint8 and got[0].shape == (len(got[1]), 3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got, want)


def random_scene(seed):
    rng = np.random.RandomState(seed)
    obs = rng.rand(*SHAPE) < (0.3, 0.6, 0.9)[seed % 3]
    occ = rng.rand(*SHAPE) < 0.2          # (also on unobserved voxels: they are no frontiers whatever their bit says)
    dist = rng.choice([0.0, 0.1, 0.2, 0.3, 0.5, 10000.0], SHAPE)
    return rng, obs, occ, dist


@pytest.mark.parametrize("seed", range(12))
def test_model_is_the_definition_on_random_arrays(seed):
    from fiesta_amd import frontier_model
    rng, obs, occ, dist = random_scene(seed)
    total = 0
    for bounded in (True, False):
        want = loop_model(obs, occ, bounded=bounded)
        same(frontier_model(obs, occ, bounded=bounded), want)
        total += len(want[1])
        # box clipping, with an origin: boxes inside, across the edge, degenerate and empty
        org = tuple(int(v) for v in rng.randint(-20, 20, 3))
        for _ in range(3):
            a = rng.randint(-2, np.array(SHAPE) + 2) + org
            b = rng.randint(-2, np.array(SHAPE) + 2) + org
            lo, hi = np.minimum(a, b), np.maximum(a, b)
            same(frontier_model(obs, occ, lo=lo, hi=hi, origin_vox=org, bounded=bounded),
                 loop_model(obs, occ, lo=lo, hi=hi, origin_vox=org, bounded=bounded))
        same(frontier_model(obs, occ, lo=(3, 3, 3), hi=(2, 9, 9), bounded=bounded), loop_model(obs, occ, lo=(3, 3, 3), hi=(2, 9, 9), bounded=bounded))
        # the clearance filter on a hand-made distance array with +10000 entries
        for c in (0.0, -1.0, 0.05, 0.25, 0.3, 9999.0, 10001.0):
            want_c = loop_model(obs, occ, dist=dist, min_clearance=c, bounded=bounded)
            same(frontier_model(obs, occ, dist=dist, min_clearance=c, bounded=bounded), want_c)
            if c <= 0:
                same(want_c, want)
            if c == 10001.0:
                assert len(want_c[1]) == 0
    assert total > 0
    # the result is sorted lexicographically
    v = frontier_model(obs, occ)[0].astype(np.int64)
    key = (v[:, 0] * 1000 + v[:, 1]) * 1000 + v[:, 2]
    assert (np.diff(key) > 0).all()


def test_clearance_passes_no_obstacle_and_is_not_read_when_off():
    from fiesta_amd import frontier_model
    obs = np.zeros(SHAPE, bool)
    obs[2:6, 2:5, 3:8] = True
    occ = np.zeros(SHAPE, bool)
    dist = np.full(SHAPE, 10000.0)
    n = len(frontier_model(obs, occ)[1])
    assert n == 4 * 3 * 5 - 2 * 1 * 3
    assert len(frontier_model(obs, occ, dist=dist, min_clearance=9999.0)[1]) == n
    assert len(frontier_model(obs, occ, dist=dist, min_clearance=10001.0)[1]) == 0
    same(frontier_model(obs, occ, dist=None, min_clearance=0.0), frontier_model(obs, occ, dist=dist, min_clearance=0.05))
    same(frontier_model(obs, occ, dist=None, min_clearance=-3.0), loop_model(obs, occ))


def test_fully_observed_and_fully_unknown_have_no_frontier():
    from fiesta_amd import frontier_model
    occ = np.zeros(SHAPE, bool)
    occ[4, 3, 5] = True
    assert len(frontier_model(np.ones(SHAPE, bool), occ)[1]) == 0
    assert len(frontier_model(np.zeros(SHAPE, bool), occ)[1]) == 0
    assert len(frontier_model(np.zeros(SHAPE, bool), occ, bounded=False)[1]) == 0
    # unbounded: the outside of a fully observed array is unknown, so its faces are frontiers -- except the occupied voxel's
    vox, mask = frontier_model(np.ones(SHAPE, bool), occ, bounded=False)
    nx, ny, nz = SHAPE
    assert len(mask) == nx * ny * nz - (nx - 2) * (ny - 2) * (nz - 2)
    same((vox, mask), loop_model(np.ones(SHAPE, bool), occ, bounded=False))


def test_single_voxels():
    from fiesta_amd import frontier_model
    occ = np.zeros(SHAPE, bool)
    obs = np.zeros(SHAPE, bool)
    obs[4, 3, 5] = True
    vox, mask = frontier_model(obs, occ, origin_vox=(10, -20, 30))
    assert vox.tolist() == [[14, -17, 35]] and mask.tolist() == [63]
    occ[4, 3, 5] = True                      # occupied: no frontier
    assert len(frontier_model(obs, occ)[1]) == 0
    occ[:] = False
    for corner, bounded_mask in (((0, 0, 0), 0b101010), ((8, 6, 10), 0b010101), ((0, 6, 0), 0b100110), ((8, 0, 10), 0b011001)):
        obs[:] = False
        obs[corner] = True
        vox, mask = frontier_model(obs, occ)
        assert vox.tolist() == [list(corner)] and mask.tolist() == [bounded_mask], (corner, mask)
        assert frontier_model(obs, occ, bounded=False)[1].tolist() == [63]
        same((vox, mask), loop_model(obs, occ))
    # two observed neighbours hide each other's shared face
    obs[:] = False
    obs[4, 3, 5] = obs[4, 3, 6] = True
    assert frontier_model(obs, occ)[1].tolist() == [63 - 32, 63 - 16]


def test_argument_rules():
    from fiesta_amd import frontier_model
    obs = np.ones(SHAPE, bool)
    with pytest.raises(ValueError):
        frontier_model(obs, ~obs, lo=(0, 0, 0))
    vox, mask = frontier_model(obs, ~obs)
    assert vox.shape == (0, 3) and mask.shape == (0,)


def test_frontier_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_frontier_" in k}
    for kernel in ("k_frontier_dense", "k_frontier_hash"):
        assert sum(kernel in k for k in res) == 1, (kernel, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
