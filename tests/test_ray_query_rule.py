"""CPU side of the ray query (fiesta_hip_ray_query, include/fiesta_hip.h): the definition.

fiesta_amd.ray_walk (plain Python f64) and fiesta_amd.ray_query_model (numpy over ray_walk) are what the GPU tests compare the
kernels with, so they must be the header's definition:
  * the walk equals the reference's Raycast -- the port library and, where it was built, the reference compiled verbatim -- with
    bounds of +-2^31, its last voxel replaced by the end point's voxel;
  * the model equals a literal per-voxel loop over the header's classification and result rules;
  * a ray the reference casts alone in a frame leaves no voxel of its walk unobserved (why the last voxel is replaced, not appended);
  * the invalid-ray rules;
  * the library's two ray-query kernels use no scratch and spill nothing.
Everything is integer, boolean or an f64 with a fixed operation order: comparisons are exact.
"""
import math
import os

import numpy as np
import pytest

from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2.0 ** 31
FREE, OCC, UNK, OUT = 0, 1, 2, 4


def manhattan(a, b):
    return int(np.abs(np.floor(b) - np.floor(a)).sum())


def voxel_rays(seed, n):
    """(a, b) pairs in voxel units: random, integer-coordinate and half-integer starts, axis-aligned, negative coordinates, one or two
    equal components, same-voxel; all with M + 1 <= 1500"""
    rng = np.random.RandomState(seed)
    rays = []
    for i in range(n):
        kind = i % 8
        span = (3.0, 12.0, 60.0, 400.0)[(i // 8) % 4]
        a = rng.uniform(-span, span, 3) + rng.choice([0.0, -1000.0, 517.0])
        b = a + rng.uniform(-span, span, 3)
        if kind == 1:
            a = np.floor(a)                                   # integer start: on a voxel corner
        elif kind == 2:
            a = np.floor(a) + 0.5                             # the centre
        elif kind == 3:
            b = a.copy()                                      # axis-aligned
            b[rng.randint(3)] += rng.uniform(-span, span)
        elif kind == 4:
            b[rng.randint(3)] = a[rng.randint(3)]             # a component of b equal to one of a (often the same axis)
            c = rng.randint(3)
            b[c] = a[c]
        elif kind == 5:
            c = rng.randint(3)                                # two equal components
            b[c], b[(c + 1) % 3] = a[c], a[(c + 1) % 3]
        elif kind == 6:
            a, b = np.floor(a), np.floor(b)                   # both ends on corners: every crossing is a tie
        elif kind == 7:
            b = np.floor(a) + rng.uniform(0, 1, 3)            # same voxel
        if manhattan(a, b) + 1 <= 1500:
            rays.append((a, b))
    return rays


def expected_walk(a, b, kind):
    R = pyoracle.raycast(a, b, (-BIG,) * 3, (BIG,) * 3, kind=kind)
    e = np.floor(np.asarray(b)).astype(np.int64)
    if len(R) == 0:
        return R, e.reshape(1, 3)
    W = R.astype(np.int64)
    assert np.array_equal(W, R)
    W[-1] = e
    return R, W


@pytest.mark.parametrize("kind", ["port", "ref"])
def test_walk_is_the_reference_traversal_with_the_end_voxel_last(kind):
    from fiesta_amd import ray_walk
    if not pyoracle.available(kind):
        if kind == "port":
            pyoracle.build("port")
        else:
            pytest.skip("the verbatim-compiled reference was not built here")
    rays = voxel_rays(11, 4000)
    assert len(rays) > 3000
    shorter = same = 0
    for a, b in rays:
        R, W = expected_walk(a, b, kind)
        got = ray_walk(a, b)
        assert got.dtype == np.int64 and np.array_equal(got, W), (a, b, got, W)
        M = manhattan(a, b)
        # (a ray shorter than its start voxel's corner distance stops at once: R is [floor(a)] alone and W is [floor(b)])
        assert (len(got) == 1 or np.array_equal(got[0], np.floor(a))) and np.array_equal(got[-1], np.floor(b)) and len(got) <= M + 1
        if M == 0:
            assert len(R) == 0 and len(got) == 1
            same += 1
        shorter += len(got) < M + 1
    assert same > 300 and shorter > 100          # (the squared-reach stop does happen)


def loop_model(obs, occ, origin, res, start, end, stop_mask, origin_vox, bounded, pos_range):
    """the header's rules, one voxel at a time, in Python floats"""
    from fiesta_amd import ray_walk
    n = len(start)
    out = {"n_visited": np.full(n, -1, np.int32), "hit_index": np.full(n, -1, np.int32), "hit_class": np.zeros(n, np.uint8),
           "hit_vox": np.full((n, 3), -2 ** 31, np.int32), "hit_dist": np.full(n, np.nan), "counts": np.zeros((n, 4), np.int32)}
    for i in range(n):
        s, t = [float(x) for x in start[i]], [float(x) for x in end[i]]
        if not all(math.isfinite(x) for x in s + t):
            continue
        W = ray_walk([x / res for x in s], [x / res for x in t])
        if W is None:
            continue
        out["n_visited"][i] = len(W)
        for k, r in enumerate(W.tolist()):
            p = [(r[c] + 0.5) * res for c in range(3)]
            v = [math.floor((p[c] - origin[c]) / res) for c in range(3)]
            j = [v[c] - origin_vox[c] for c in range(3)]
            in_array = all(0 <= j[c] < obs.shape[c] for c in range(3))
            if bounded and (any(p[c] < pos_range[0][c] or p[c] > pos_range[1][c] for c in range(3)) or not in_array):
                cls = OUT
            elif not in_array or not obs[tuple(j)]:
                cls = UNK
            else:
                cls = OCC if occ[tuple(j)] else FREE
            if cls & stop_mask:
                q = [p[c] - s[c] for c in range(3)]
                out["hit_index"][i], out["hit_class"][i], out["hit_vox"][i] = k, cls, v
                out["hit_dist"][i] = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
                out["n_visited"][i] = k + 1
                break
            out["counts"][i, (FREE, OCC, UNK, OUT).index(cls)] += 1
    return out


def same_results(got, want):
    for name, dtype in (("n_visited", np.int32), ("hit_index", np.int32), ("hit_class", np.uint8), ("hit_vox", np.int32),
                        ("hit_dist", np.float64), ("counts", np.int32)):
        assert got[name].dtype == dtype and got[name].shape == want[name].shape, name
        if name == "hit_dist":
            nan = np.isnan(want[name])            # (NaN where there is no hit; every other value bit for bit)
            assert np.array_equal(np.isnan(got[name]), nan) and np.array_equal(got[name][~nan].view(np.uint64), want[name][~nan].view(np.uint64)), name
        else:
            assert np.array_equal(got[name], want[name]), (name, np.flatnonzero(np.any((got[name] != want[name]).reshape(len(got[name]), -1), axis=1))[:8])


@pytest.mark.parametrize("seed", range(6))
def test_model_is_the_definition_on_random_arrays(seed):
    from fiesta_amd import ray_query_model
    rng = np.random.RandomState(seed)
    shape = (9, 7, 11)
    obs = rng.rand(*shape) < (0.5, 0.8, 0.95)[seed % 3]
    occ = rng.rand(*shape) < 0.15                 # (also on unobserved voxels: UNKNOWN takes precedence)
    res = (0.1, 0.25)[seed % 2]
    ov = (0, 0, 0) if seed < 2 else tuple(int(x) for x in rng.randint(-6, 6, 3))
    origin = np.array([-0.33, 0.2, -0.51]) if seed % 3 else np.array([-0.3, 0.2, -0.5])
    lo = origin + np.array(ov) * res
    hi = lo + np.array(shape) * res
    pos_range = (lo - 0.013, hi - 0.19)           # (PosInMap's range need not be the array's)
    n = 150
    start = rng.uniform(lo - 3 * res, hi + 3 * res, (n, 3))
    end = np.where(rng.rand(n, 1) < 0.3, start + rng.uniform(-res, res, (n, 3)), rng.uniform(lo - 3 * res, hi + 3 * res, (n, 3)))
    start[5], end[6, 1], end[7, 2] = np.nan, np.inf, 5000 * res      # invalid rays among the valid
    hits = 0
    for bounded in (True, False):
        for mask in range(8):
            want = loop_model(obs, occ, origin, res, start, end, mask, ov, bounded, pos_range)
            got = ray_query_model(obs, occ, origin, res, start, end, mask, origin_vox=ov, bounded=bounded, pos_range=pos_range)
            same_results(got, want)
            hits += int((got["hit_index"] >= 0).sum())
            assert (got["n_visited"][[5, 6, 7]] == -1).all() and not got["counts"][[5, 6, 7]].any()
            if mask == 0:
                assert (got["hit_index"] == -1).all() and np.isnan(got["hit_dist"]).all()
                ok = got["n_visited"] >= 0
                assert np.array_equal(got["counts"].sum(1)[ok], got["n_visited"][ok])
            if not bounded:
                assert not got["counts"][:, 3].any() and not (got["hit_class"] == OUT).any()
    assert hits > 500


def test_default_range_and_argument_rules():
    from fiesta_amd import ray_query_model
    obs = np.ones((4, 4, 4), bool)
    occ = np.zeros((4, 4, 4), bool)
    occ[2, 1, 1] = True
    r = ray_query_model(obs, occ, (0, 0, 0), 0.5, [[0.25, 0.75, 0.75]], [[1.9, 0.75, 0.75]], 1)
    assert r["hit_index"].tolist() == [2] and r["hit_vox"].tolist() == [[2, 1, 1]] and r["hit_class"].tolist() == [1]
    assert r["hit_dist"][0] == 1.0 and r["n_visited"].tolist() == [3] and r["counts"].tolist() == [[2, 0, 0, 0]]
    r = ray_query_model(obs, occ, (0, 0, 0), 0.5, [[0.25, 0.75, 0.75]], [[3.2, 0.75, 0.75]], 4)     # leaves the array at x = 4
    assert r["hit_index"].tolist() == [4] and r["hit_class"].tolist() == [4] and r["counts"].tolist() == [[3, 1, 0, 0]]
    r = ray_query_model(obs, occ, (0, 0, 0), 0.5, [[0.25, 0.75, 0.75]], [[3.2, 0.75, 0.75]], 6, bounded=False)
    assert r["hit_class"].tolist() == [2]
    with pytest.raises(ValueError):
        ray_query_model(obs, occ, (0, 0, 0), 0.5, [[0, 0, 0]], [[1, 1, 1]], 8)
    with pytest.raises(ValueError):
        ray_query_model(obs, occ, (0, 0, 0), 0.5, [[0, 0, 0]], [[1, 1, 1], [2, 2, 2]], 1)
    r = ray_query_model(obs, occ, (0, 0, 0), 0.5, np.zeros((0, 3)), np.zeros((0, 3)), 7)
    assert r["hit_vox"].shape == (0, 3) and r["counts"].shape == (0, 4)


@pytest.mark.parametrize("res,origin", [(0.1, (0.0, 0.0, 0.0)), (0.125, (-1.0, -0.5, -0.25))])
def test_a_ray_cast_alone_leaves_none_of_its_walk_unknown(res, origin):
    """the sensor-consistency property: map origin a multiple of the resolution, ONE ray per frame (the reference's de-duplication
    leaves crossed voxels unobserved otherwise), min_ray_length 0"""
    from fiesta_amd import ray_query_model, ray_walks
    if not pyoracle.available("port"):
        pyoracle.build("port")
    dims = np.array([40, 24, 36])
    size = (dims - 0.5) * res                     # (ceil(size / res) voxels, whatever the rounding of the product)
    origin = np.array(origin)
    rng = np.random.RandomState(3)
    n = 300
    sensor = origin + size * np.array([0.45, 0.5, 0.4]) + 0.013
    pts = rng.uniform(origin + 0.2 * res, origin + size - 0.2 * res, (n, 3)).astype(np.float32)
    pts[:20] = (np.floor((pts[:20] - origin) / res) * res + origin).astype(np.float32)       # some on voxel faces
    m = pyoracle.OracleMap(origin, res, size, kind="port")
    m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80)
    T = np.eye(4)
    for i in range(n):
        m.raycast_frame(pts[i:i + 1], T, sensor, 0.0, 1000.0, origin - 1.0, origin + size + 1.0)
    m.UpdateOccupancy(True)
    d = m.dump_dense(want=("dist", "occ"))
    assert d["dist"].size == dims.prod()
    obs = (d["dist"] >= 0).reshape(dims)
    occ = d["occ"].reshape(dims).astype(bool)
    m.close()
    end = pts.astype(np.float64)                  # (the frame's end points: the identity transform of the f32 points in f64)
    start = np.repeat(sensor[None], n, 0)
    walks = ray_walks(start, end, res)
    got = ray_query_model(obs, occ, origin, res, start, end, UNK, pos_range=(origin, origin + size), walks=walks)
    assert (got["n_visited"] > 0).all()
    assert (got["hit_index"] == -1).all(), np.flatnonzero(got["hit_index"] != -1)


def test_invalid_rays():
    from fiesta_amd import ray_query_model, ray_walk
    assert ray_walk((0.5, 0.5, 0.5), (float("nan"), 0, 0)) is None
    assert ray_walk((float("inf"), 0.5, 0.5), (1, 0, 0)) is None
    assert ray_walk((0.5, 0.5, -float("inf")), (1, 0, 0)) is None
    assert ray_walk((2.0 ** 30, 0.5, 0.5), (2.0 ** 30, 0.5, 0.5)) is None
    assert ray_walk((0.5, 0.5, 0.5), (0.5, -2.0 ** 30, 0.5)) is None
    w = ray_walk((2.0 ** 30 - 0.5, 0.5, 0.5), (2.0 ** 30 - 3.5, 0.5, 0.5))
    assert w[:, 0].tolist() == [2 ** 30 - 1, 2 ** 30 - 2, 2 ** 30 - 3, 2 ** 30 - 4]
    assert len(ray_walk((0.5, 0.5, 0.5), (4095.5, 0.5, 0.5))) == 4096            # M = 4095
    assert ray_walk((0.5, 0.5, 0.5), (4096.5, 0.5, 0.5)) is None                 # M = 4096
    assert len(ray_walk((0.5, 0.5, 0.5), (1365.5, 1365.5, -1364.5))) <= 4096     # M = 4095 over three axes
    assert ray_walk((0.5, 0.5, 0.5), (1365.5, 1366.5, -1364.5)) is None
    # in the model: voxel units are start / resolution
    obs = np.ones((3, 3, 3), bool)
    res = 0.5
    start = np.array([[0.2, 0.2, 0.2]] * 6)
    end = np.array([[0.7, 0.2, 0.2], [np.nan, 0.2, 0.2], [0.2, np.inf, 0.2], [0.2, 0.2, 2.0 ** 29], [0.2 + 4095 * res, 0.2, 0.2],
                    [0.2 + 4096 * res, 0.2, 0.2]])
    r = ray_query_model(obs, ~obs, (0, 0, 0), res, start, end, 0)
    assert r["n_visited"].tolist() == [2, -1, -1, -1, 4096, -1]
    bad = [1, 2, 3, 5]
    assert (r["hit_index"][bad] == -1).all() and (r["hit_class"][bad] == 0).all() and (r["hit_vox"][bad] == -2 ** 31).all()
    assert np.isnan(r["hit_dist"][bad]).all() and not r["counts"][bad].any()
    assert r["counts"][0].tolist() == [2, 0, 0, 0] and r["counts"][4].tolist() == [3, 0, 0, 4093]


def test_ray_query_kernels_use_no_scratch_and_spill_nothing():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_ray_query" in k}
    for source in ("DenseRaySource", "HashRaySource"):
        assert sum(source in k for k in res) == 1, (source, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
