"""CPU side of the skeleton extraction (fiesta_hip_get_skeleton_voxels, include/fiesta_hip.h): the definition.

fiesta_amd.skeleton_model (numpy, shifted-array comparisons) is the model the GPU tests compare the kernels with, so it must be the
header's definition: it is checked against a literal triple loop over that definition, one voxel at a time, on exact brute-force
fields of random point obstacles (ties broken in the obstacles' order, and in a shuffled order), on the same fields with a few ids
replaced by a farther obstacle (the field is no exact transform: the wrong-side skips must be taken), and on two walls whose
skeleton is known.  Everything is integer: comparisons are exact.  Also: the library's two skeleton kernels use no scratch.

The bits of the mask: 0 is -x, 1 is +x, 2 is -y, 3 is +y, 4 is -z, 5 is +z.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
FIELDS = ((12, 10, 7), 5), ((12, 10, 33), 5), ((24, 20, 40), 12)


def loop_model(d2, coc, occ, min_sep2, dist=None, lo=None, hi=None, min_clearance=0.0, origin_vox=(0, 0, 0), skips=None):
    """the header's definition, voxel by voxel; skips (a list): the wrong-side pairs met are counted into skips[0]"""
    nx, ny, nz = d2.shape

    def site(i, j, k):
        return tuple(int(c) for c in coc[i, j, k]) if 0 <= d2[i, j, k] < INT32_MAX else None

    def sq(p, q):
        return sum((p[c] - q[c]) ** 2 for c in range(3))

    rows = []
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                if d2[i, j, k] < 0 or occ[i, j, k]:
                    continue
                a = site(i, j, k)
                if a is None:
                    continue
                v = (i + origin_vox[0], j + origin_vox[1], k + origin_vox[2])
                r, best = 0, 0
                for bit, (dx, dy, dz) in enumerate(DIRS):
                    p, q, s = i + dx, j + dy, k + dz
                    if not (0 <= p < nx and 0 <= q < ny and 0 <= s < nz):
                        continue
                    b = site(p, q, s)
                    if b is None:
                        continue
                    n = (v[0] + dx, v[1] + dy, v[2] + dz)
                    sep2 = sq(a, b)
                    if sep2 < min_sep2:
                        continue
                    gv, gn = sq(v, b) - sq(v, a), sq(n, b) - sq(n, a)
                    if gv < 0 or gn > 0:
                        if skips is not None:
                            skips[0] += 1
                        continue
                    if gv <= -gn:
                        r |= 1 << bit
                        best = max(best, sep2)
                if r == 0:
                    continue
                if lo is not None and not all(lo[c] <= v[c] <= hi[c] for c in range(3)):
                    continue
                if min_clearance > 0 and not dist[i, j, k] >= min_clearance:
                    continue
                rows.append(v + (r, int(d2[i, j, k]), best))
    rows.sort()
    a = np.array(rows, np.int64).reshape(-1, 6)
    return {"vox": a[:, :3].astype(np.int32), "mask": a[:, 3].astype(np.uint8), "d2": a[:, 4].astype(np.int32),
            "sep2": a[:, 5].astype(np.int32)}


def same(got, want):
    assert got["vox"].dtype == np.int32 and got["mask"].dtype == np.uint8 and got["d2"].dtype == np.int32 and got["sep2"].dtype == np.int32
    assert got["vox"].shape == (len(got["mask"]), 3) and got["d2"].shape == got["sep2"].shape == got["mask"].shape
    for name in ("vox", "mask", "d2", "sep2"):
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])


def exact_field(shape, sites, order=None, origin_vox=(0, 0, 0)):
    """the exact transform of point obstacles (array coordinates), ties to the first obstacle in `order`: d2, coc (map
    coordinates), occ"""
    sites = np.asarray(sites, np.int64).reshape(-1, 3)
    order = np.arange(len(sites)) if order is None else np.asarray(order)
    pos = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).astype(np.int64)
    d = ((pos[..., None, :] - sites[order]) ** 2).sum(axis=-1)            # (nx, ny, nz, sites)
    win = d.argmin(axis=-1)                                               # (the first minimum: the tie-break)
    d2 = np.take_along_axis(d, win[..., None], axis=-1)[..., 0]
    coc = sites[order][win] + np.asarray(origin_vox, np.int64)
    occ = np.zeros(shape, bool)
    occ[tuple(sites.T)] = True
    return d2.astype(np.int64), coc, occ


def random_sites(rng, shape, n):
    flat = rng.choice(int(np.prod(shape)), n, replace=False)
    return np.stack(np.unravel_index(flat, shape), axis=-1)


@pytest.mark.parametrize("case", range(len(FIELDS)))
@pytest.mark.parametrize("variant", ["exact", "shuffled", "inexact"])
def test_model_is_the_definition(case, variant):
    from fiesta_amd import skeleton_model
    shape, n_sites = FIELDS[case]
    rng = np.random.RandomState(100 + case)
    sites = random_sites(rng, shape, n_sites)
    order = rng.permutation(n_sites) if variant == "shuffled" else None
    d2, coc, occ = exact_field(shape, sites, order)
    if variant == "inexact":
        # a few voxels name a farther obstacle (d2 follows the id, as in the map): some pairs end on the wrong side of their bisector
        for flat in rng.choice(int(np.prod(shape)), int(np.prod(shape)) // 6, replace=False):
            i, j, k = np.unravel_index(flat, shape)
            if occ[i, j, k]:
                continue
            s = sites[rng.randint(n_sites)]
            coc[i, j, k] = s
            d2[i, j, k] = ((np.array([i, j, k]) - s) ** 2).sum()
        # ... and a few are not observed, or observed without an obstacle (the id left behind must not be read)
        hole = rng.rand(*shape) < 0.03
        d2[hole] = -1
        inf = (rng.rand(*shape) < 0.03) & ~hole & ~occ
        d2[inf] = INT32_MAX
    skips = [0]
    total = 0
    for min_sep2 in (1, 2, 9, 16):
        want = loop_model(d2, coc, occ, min_sep2, skips=skips)
        same(skeleton_model(d2, coc, occ, min_sep2), want)
        total += len(want["mask"])
        assert len(want["mask"]) > 0, (shape, variant, min_sep2)
        # the threshold: every row's witness reaches it, and raising it only removes rows
        assert (want["sep2"] >= min_sep2).all()
    assert (skips[0] > 0) == (variant == "inexact"), (variant, skips)
    # box clipping, with an origin: boxes inside, across the edge, degenerate and empty
    org = tuple(int(v) for v in rng.randint(-20, 20, 3))
    d2o, coco, occo = d2, coc + np.array(org), occ
    for _ in range(3):
        a = rng.randint(-2, np.array(shape) + 2) + org
        b = rng.randint(-2, np.array(shape) + 2) + org
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        same(skeleton_model(d2o, coco, occo, 4, lo=lo, hi=hi, origin_vox=org), loop_model(d2o, coco, occo, 4, lo=lo, hi=hi, origin_vox=org))
    whole = skeleton_model(d2o, coco, occo, 4, origin_vox=org)
    same(whole, loop_model(d2o, coco, occo, 4, origin_vox=org))
    assert np.array_equal(whole["vox"] - np.array(org, np.int32), skeleton_model(d2, coc, occ, 4)["vox"])   # (the rule is translation invariant)
    assert len(skeleton_model(d2, coc, occ, 4, lo=(3, 3, 3), hi=(2, 9, 9))["mask"]) == 0
    # the clearance filter, on the field's own distances (resolution 0.1)
    dist = np.where(d2 < 0, 10000.0, np.where(d2 == INT32_MAX, 10000.0, np.sqrt(np.maximum(d2, 0).astype(np.float64)) * 0.1))
    base = skeleton_model(d2, coc, occ, 4)
    for c in (0.0, -1.0, 0.15, 0.25, 0.3, 10001.0):
        want_c = loop_model(d2, coc, occ, 4, dist=dist, min_clearance=c)
        same(skeleton_model(d2, coc, occ, 4, dist=dist, min_clearance=c), want_c)
        if c <= 0:
            same(want_c, base)
        if c == 10001.0:
            assert len(want_c["mask"]) == 0
    assert 0 < len(skeleton_model(d2, coc, occ, 4, dist=dist, min_clearance=0.25)["mask"]) < len(base["mask"])
    # sorted lexicographically
    v = base["vox"].astype(np.int64)
    assert (np.diff((v[:, 0] * 1000 + v[:, 1]) * 1000 + v[:, 2]) > 0).all()


def walls_field(x_walls, shape=(12, 10, 40), prefer=0):
    """two full walls (planes of occupied voxels at the given x); every voxel's site is the wall voxel straight across, the nearer
    wall's -- on a tie the wall `prefer`, or per voxel at random (prefer = a RandomState)"""
    nx, ny, nz = shape
    d2 = np.zeros(shape, np.int64)
    coc = np.zeros(shape + (3,), np.int64)
    occ = np.zeros(shape, bool)
    for x in x_walls:
        occ[x] = True
    for i in range(nx):
        da, db = abs(i - x_walls[0]), abs(i - x_walls[1])
        for j in range(ny):
            for k in range(nz):
                if da != db:
                    w = 0 if da < db else 1
                else:
                    w = prefer if isinstance(prefer, int) else int(prefer.randint(2))
                coc[i, j, k] = (x_walls[w], j, k)
                d2[i, j, k] = (i - x_walls[w]) ** 2
    return d2, coc, occ


@pytest.mark.parametrize("min_sep2", [2, 4, 9, 16])
def test_two_walls_known_answers(min_sep2):
    from fiesta_amd import skeleton_model
    shape = (12, 10, 40)
    # an even gap (walls at x = 1 and x = 9): exactly the 400 voxels of the plane x = 5, whatever the tie-break -- only the bit moves
    seen = set()
    for prefer in (0, 1, np.random.RandomState(7)):
        d2, coc, occ = walls_field((1, 9), shape, prefer)
        got = skeleton_model(d2, coc, occ, min_sep2)
        same(got, loop_model(d2, coc, occ, min_sep2))
        assert len(got["mask"]) == 400 and (got["vox"][:, 0] == 5).all()
        assert (got["d2"] == 16).all() and (got["sep2"] >= 64).all()
        if isinstance(prefer, int):      # (a per-voxel tie-break also puts ridges between neighbours inside the plane)
            assert (got["sep2"] == 64).all() and set(got["mask"].tolist()) == {2 - prefer}, set(got["mask"].tolist())
            seen |= set(got["mask"].tolist())
        else:
            assert len(set(got["mask"].tolist())) > 2
    assert seen == {1, 2}
    # an odd gap (walls at x = 1 and x = 10): the bisector lies half way between x = 5 and x = 6, a tie that marks both planes
    d2, coc, occ = walls_field((1, 10), shape)
    got = skeleton_model(d2, coc, occ, min_sep2)
    same(got, loop_model(d2, coc, occ, min_sep2))
    assert len(got["mask"]) == 800 and sorted(set(got["vox"][:, 0].tolist())) == [5, 6]
    assert (got["mask"][got["vox"][:, 0] == 5] == 2).all() and (got["mask"][got["vox"][:, 0] == 6] == 1).all()
    assert (got["sep2"] == 81).all()
    # a flat wall alone: its adjacent voxels are distinct sites 1 apart -- min_sep2 = 1 marks the whole half space, 2 nothing of it
    if min_sep2 == 2:
        d2, coc, occ = walls_field((1, 1), shape)
        assert len(skeleton_model(d2, coc, occ, 2)["mask"]) == 0
        near = skeleton_model(d2, coc, occ, 1)
        same(near, loop_model(d2, coc, occ, 1))
        assert len(near["mask"]) == (12 - 1) * 10 * 40 and (near["sep2"] == 1).all()


def test_min_sep2_threshold_has_sep2_as_its_witness():
    from fiesta_amd import skeleton_model
    shape, n_sites = FIELDS[1]
    rng = np.random.RandomState(5)
    d2, coc, occ = exact_field(shape, random_sites(rng, shape, n_sites))
    lowest = skeleton_model(d2, coc, occ, 1)
    prev = lowest
    for t in (2, 3, 5, 9, 10, 17, 30, 60):
        got = skeleton_model(d2, coc, occ, t)
        assert (got["sep2"] >= t).all()
        # the rows that remain are those of the lower threshold whose LARGEST separation reaches t (their masks may lose bits)
        keys = {tuple(v) for v in got["vox"].tolist()}
        assert keys == {tuple(v) for v, s in zip(prev["vox"].tolist(), prev["sep2"].tolist()) if s >= t}
        prev = got
    assert len(lowest["mask"]) > len(prev["mask"]) > 0


def test_argument_rules():
    from fiesta_amd import skeleton_model
    d2, coc, occ = walls_field((1, 9), (12, 10, 8))
    for bad in (dict(min_sep2=0), dict(min_sep2=-3), dict(min_sep2=1.5), dict(min_sep2=4, min_clearance=float("nan")),
                dict(min_sep2=4, lo=(0, 0, 0)), dict(min_sep2=4, hi=(3, 3, 3)), dict(min_sep2=4, min_clearance=0.2)):
        with pytest.raises(ValueError):
            skeleton_model(d2, coc, occ, **bad)
    with pytest.raises(ValueError):
        skeleton_model(d2.ravel(), coc, occ, 4)
    got = skeleton_model(np.full((4, 4, 4), -1), np.zeros((4, 4, 4, 3)), np.zeros((4, 4, 4), bool), 1)
    assert got["vox"].shape == (0, 3) and got["mask"].shape == got["d2"].shape == got["sep2"].shape == (0,)


def test_skeleton_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_skeleton_" in k}
    for kernel in ("k_skeleton_dense", "k_skeleton_hash"):
        assert sum(kernel in k for k in res) == 1, (kernel, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
