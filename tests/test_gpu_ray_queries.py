"""Batched ray queries on the GPU (fiesta_hip_ray_query[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/ray_query_kernels.hpp).

The expected result is always fiesta_amd.ray_query_model (the header's definition in numpy over the plain-Python walk;
tests/test_ray_query_rule.py checks both against the reference's traversal and a literal loop) fed from what the map itself reports
through calls that existed before: download_field (d2 >= 0, occ) or download_hash -- never from the call under test.  Every output
is an integer or an f64 with a fixed operation order: all comparisons are bit for bit, hit_dist included.
"""
import ctypes as C

import numpy as np
import pytest

from scenarios import P_DEFAULT

pytestmark = pytest.mark.gpu
RES = 0.1
DIMS = (40, 24, 70)             # nz is no multiple of 32: rays cross the word boundaries z = 31 | 32, 63 | 64 and the padding bits
FIELDS = ("n_visited", "hit_index", "hit_class", "hit_vox", "hit_dist", "counts")
FREE, OCC, UNK, OUT = 0, 1, 2, 4


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, what=""):
    for name in FIELDS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if name == "hit_dist":      # NaN where there is no hit, whatever its payload; every other value bit for bit
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name, np.flatnonzero(np.isnan(g) != np.isnan(w))[:8])
            ok = ~np.isnan(w)
            bad = np.flatnonzero(bits(g[ok]) != bits(w[ok]))
        else:
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert len(bad) == 0, f"{what}: {name} differs on {len(bad)} rays, first {bad[:5].tolist()}: got {g[bad[:3]].tolist()} want {w[bad[:3]].tolist()}"


def make_dense(origin, dims=DIMS, seed=5):
    """partly observed through SetOccupancyBox (an unknown slab at x = 21 .. 23, an unknown block above z = 40 beyond it, an
    unobserved rim), plus random occupied voxels"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap(origin, RES, tuple((s - 0.5) * RES for s in dims))      # (ceil(size / res) voxels)
    assert m.grid_size == tuple(dims)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((2, 2, 2), (20, dims[1] - 3, dims[2] - 3), 0)
    m.SetOccupancyBox((24, 1, 0), (dims[0] - 1, dims[1] - 1, 40), 0)
    m.UpdateOccupancy(True)
    rng = np.random.RandomState(seed)
    S = (rng.rand(160, 3) * np.array(dims)).astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


class DenseModel:
    """ray_query_model on the map's own dump"""

    def __init__(self, m, origin_vox=(0, 0, 0), dims=None):
        dims = tuple(dims or m.grid_size)
        f = m.download_field(("d2", "occ"))
        self.m, self.ov = m, origin_vox
        self.obs = (f["d2"] >= 0).reshape(dims)
        self.occ = f["occ"].reshape(dims) != 0

    def __call__(self, start, end, mask, walks=None):
        from fiesta_amd import ray_query_model
        return ray_query_model(self.obs, self.occ, self.m.origin, RES, start, end, mask, origin_vox=self.ov, pos_range=self.m.pos_range,
                               walks=walks)


def dense_rays(origin, dims=DIMS, seed=9):
    """the ray set of the dense tests, metres; returns (start, end, indices of the invalid rays)"""
    rng = np.random.RandomState(seed)
    org, size = np.asarray(origin, np.float64), np.array(dims) * RES
    S, E = [], []

    def add(s, e):
        S.append(np.asarray(s, np.float64).reshape(-1, 3))
        E.append(np.asarray(e, np.float64).reshape(-1, 3))
    add(org + rng.rand(300, 3) * size, org + rng.rand(300, 3) * size)                       # inside the map
    s = org + rng.rand(150, 3) * size
    d = rng.randn(150, 3)
    d /= np.linalg.norm(d, axis=1)[:, None]
    add(s - d * rng.uniform(3, 9, (150, 1)), s + d * rng.uniform(3, 9, (150, 1)))           # entering from outside and leaving again
    add(org + rng.rand(40, 3) * size, org + size * rng.uniform(1.05, 1.5, (40, 3)))         # leaving only
    for axis in range(3):                                                                   # axis-aligned, through voxel centres
        c = org + (np.floor(rng.rand(20, 3) * np.array(dims)) + 0.5) * RES
        e = c.copy()
        e[:, axis] = org[axis] + (np.floor(rng.rand(20) * dims[axis]) + 0.5) * RES
        add(c, e)
    c = org + (np.floor(rng.rand(30, 3) * np.array(dims)) + 0.5) * RES                      # along z across z = 31 | 32 and 63 | 64
    lo, hi = c.copy(), c.copy()
    lo[:, 2], hi[:, 2] = org[2] + rng.uniform(26, 31.9, 30) * RES, org[2] + rng.uniform(32.1, 69.9, 30) * RES
    add(lo[:15], hi[:15])
    add(hi[15:], lo[15:])
    s = org + rng.rand(30, 3) * size                                                        # across the map just below / above z = 32
    e = org + rng.rand(30, 3) * size
    s[:, 2], e[:, 2] = org[2] + rng.uniform(31.0, 33.0, 30) * RES, org[2] + rng.uniform(31.0, 33.0, 30) * RES
    add(s, e)
    s = org + rng.rand(30, 3) * size
    add(s, s + rng.uniform(-0.3, 0.3, (30, 3)) * RES)                                       # (mostly) same voxel
    add(s[:20], s[:20])                                                                     # zero length
    s, e = org + rng.rand(60, 3) * size, org + rng.rand(60, 3) * size                       # ending exactly on faces of the world grid
    e = np.round(e / RES) * RES
    s[:20] = np.round(s[:20] / RES) * RES                                                   # ... and starting on one
    add(s, e)
    add(np.round(s[:10] / RES) * RES, np.round(s[:10] / RES) * RES + np.array([3 * RES, 0, 0]))   # along an edge of the grid
    start, end = np.concatenate(S), np.concatenate(E)
    invalid = np.array([7, 100, 301, 460, 461, len(start) - 1])                             # invalid rays mixed in
    end[7, 1] = np.nan
    start[100, 2] = np.inf
    end[301, 0] = -np.inf
    start[460] = [RES * 2.0 ** 30, 0.0, 0.0]
    end[461, 0] = start[461, 0] + 4200 * RES                                                # more than 4095 voxel steps
    start[-1] = np.nan
    return start, end, invalid


@pytest.fixture(scope="module", params=["ragged_origin", "aligned_origin"])
def dense(request, hip_lib):
    from fiesta_amd import ray_walks
    origin = (-1.03, 0.27, -0.51) if request.param == "ragged_origin" else (-1.0, 0.5, -0.5)
    m = make_dense(origin)
    start, end, invalid = dense_rays(origin)
    model = DenseModel(m)
    walks = ray_walks(start, end, RES)
    want = {mask: model(start, end, mask, walks) for mask in range(8)}        # computed once, shared, left unchanged
    yield m, model, start, end, invalid, walks, want
    m.close()


def test_dense_all_stop_masks(dense):
    m, model, start, end, invalid, walks, want = dense
    assert 2000 < model.obs.sum() < model.obs.size and 100 < model.occ.sum()
    for mask in range(8):
        got = m.RayQuery(start, end, mask)
        assert_same(got, want[mask], f"stop_mask {mask}")
        assert (got["n_visited"][invalid] == -1).all() and np.isnan(got["hit_dist"][invalid]).all()
        assert (np.delete(got["n_visited"], invalid) >= 1).all()
    # the scene exercises every class, as a hit and as a count
    assert set(np.unique(want[7]["hit_class"])) == {0, OCC, UNK, OUT}
    assert (want[0]["counts"].sum(0) > 50).all() and (want[0]["hit_index"] == -1).all()
    assert (want[1]["hit_class"] == OCC).sum() > 20 and (want[1]["counts"][:, 2] > 0).sum() > 100      # a view's gain
    long_rays = want[0]["n_visited"] > 40
    assert long_rays.sum() > 50 and (want[7]["n_visited"][long_rays] < want[0]["n_visited"][long_rays]).mean() > 0.5


def test_batch_sizes(dense):
    m, model, start, end, invalid, walks, want = dense
    for n in (1, 63, 64, 65):
        for first in (0, 299):
            sl = slice(first, first + n)
            for mask in (0, 3, 7):
                got = m.RayQuery(start[sl], end[sl], mask)
                assert_same(got, {k: v[sl] for k, v in want[mask].items()}, f"{n} rays from {first}, stop_mask {mask}")
    one = m.RayQuery(start[3], end[3], 7)                      # a single triple
    assert_same(one, {k: v[3:4] for k, v in want[7].items()}, "one ray")
    # about 5000 rays, fresh ones: whole work-groups and a ragged last one
    rng = np.random.RandomState(21)
    org, size = m.origin, np.array(DIMS) * RES
    s = org + (rng.rand(5003, 3) * 1.4 - 0.2) * size
    e = org + (rng.rand(5003, 3) * 1.4 - 0.2) * size
    from fiesta_amd import ray_walks
    w = ray_walks(s, e, RES)
    for mask in (1, 6, 7):
        assert_same(m.RayQuery(s, e, mask), model(s, e, mask, w), f"5003 rays, stop_mask {mask}")


def test_more_rays_than_lanes_in_the_grid(dense):
    """the grid is capped at 2048 work-groups of 256 lanes: a larger batch strides, and nothing depends on the launch shape"""
    m, model, start, end, invalid, walks, want = dense
    n = 2048 * 256 + 37
    reps = -(-n // len(start))
    s, e = np.tile(start, (reps, 1))[:n], np.tile(end, (reps, 1))[:n]
    got = m.RayQuery(s, e, 7)
    assert_same(got, {k: np.concatenate([v] * reps)[:n] for k, v in want[7].items()}, "strided batch")


def device_query(m, start, end, mask, fields=FIELDS):
    import torch
    dev = torch.device("cuda", 0)
    n = len(start)
    s, e = torch.from_numpy(np.ascontiguousarray(start)).to(dev), torch.from_numpy(np.ascontiguousarray(end)).to(dev)
    shapes = {"n_visited": ((n,), torch.int32), "hit_index": ((n,), torch.int32), "hit_class": ((n,), torch.uint8),
              "hit_vox": ((n, 3), torch.int32), "hit_dist": ((n,), torch.float64), "counts": ((n, 4), torch.int32)}
    out = {k: torch.full(shapes[k][0], 77, dtype=shapes[k][1], device=dev) for k in fields}
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the copies and fills above must have landed)
    m.RayQueryDevice(s.data_ptr(), e.data_ptr(), n, mask, {k: t.data_ptr() for k, t in out.items()})
    m.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def test_device_variant_equals_host_variant(dense):
    m, model, start, end, invalid, walks, want = dense
    for mask in (0, 1, 2, 7):
        got = device_query(m, start, end, mask)
        assert_same(got, m.RayQuery(start, end, mask), f"device against host, stop_mask {mask}")
        assert_same(got, want[mask], f"device against model, stop_mask {mask}")
        assert np.array_equal(bits(got["hit_dist"][~np.isnan(got["hit_dist"])]), bits(want[mask]["hit_dist"][~np.isnan(want[mask]["hit_dist"])]))
    part = device_query(m, start, end, 7, fields=("hit_index", "counts"))          # missing fields are not written
    assert np.array_equal(part["hit_index"], want[7]["hit_index"]) and np.array_equal(part["counts"], want[7]["counts"])


def raw_call(m, start, end, n, mask, arrays, result=True, dev=False):
    from fiesta_amd._lib import RayResult
    from fiesta_amd.esdf_map import _p
    res = RayResult(*[None if arrays.get(k) is None else arrays[k].ctypes.data for k in FIELDS])
    fn = m._lib.fiesta_hip_ray_query_dev if dev else m._lib.fiesta_hip_ray_query
    return fn(m._h, _p(start), _p(end), n, mask, C.byref(res) if result else None)


def blank(n):
    return {"n_visited": np.full(n, 77, np.int32), "hit_index": np.full(n, 77, np.int32), "hit_class": np.full(n, 77, np.uint8),
            "hit_vox": np.full((n, 3), 77, np.int32), "hit_dist": np.full(n, 77.0), "counts": np.full((n, 4), 77, np.int32)}


def test_null_outputs_empty_batches_and_errors(dense):
    import fiesta_amd
    from fiesta_amd._lib import check
    m, model, start, end, invalid, walks, want = dense
    n = len(start)
    for leave_out in FIELDS:                                   # each result pointer NULL in turn
        arrays = blank(n)
        arrays[leave_out] = None
        assert raw_call(m, start, end, n, 7, arrays) == 0
        for k in FIELDS:
            if k != leave_out:
                assert_same({f: arrays[k] if f == k else want[7][f] for f in FIELDS}, want[7], f"without {leave_out}: {k}")
    assert raw_call(m, start, end, n, 7, {}) == 0              # all of them
    arrays = blank(4)
    assert raw_call(m, start, end, 0, 7, arrays) == 0          # n = 0 does nothing
    assert all((arrays[k] == 77).all() for k in FIELDS)
    errors = [raw_call(m, None, end, 4, 7, arrays), raw_call(m, start, None, 4, 7, arrays), raw_call(m, start, end, 4, 7, arrays, result=False),
              raw_call(m, start, end, 4, -1, arrays), raw_call(m, start, end, 4, 8, arrays), raw_call(m, start, end, -1, 7, arrays),
              raw_call(m, None, end, 0, 7, arrays), raw_call(m, start, end, 4, 8, arrays, dev=True), raw_call(m, start, end, -1, 7, arrays, dev=True),
              raw_call(m, None, end, 4, 7, arrays, dev=True), raw_call(m, start, end, 4, 7, arrays, result=False, dev=True)]
    for st in errors:
        assert st == 1                                         # FIESTA_HIP_ERR_INVALID
        with pytest.raises(fiesta_amd.FiestaHipError):
            check(st)
    assert all((arrays[k] == 77).all() for k in FIELDS)        # nothing launched
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.RayQuery(start[:2], end[:2], 9)
    assert_same(m.RayQuery(start, end, 7), want[7], "after the errors")
    assert m.GetOccupancy(np.array([[5, 5, 5]], np.int32)).shape == (1,)


def test_classes_follow_update_occupancy_not_update_esdf(hip_lib):
    origin = (-1.0, 0.5, -0.5)
    m = make_dense(origin, seed=6)
    before = DenseModel(m)
    # a ray along x through known free space: the first row (y, z) of the observed box without an obstacle
    row_free = (before.obs[2:21] & ~before.occ[2:21]).all(0)
    y, z = (int(v) for v in np.argwhere(row_free)[0])
    s = np.array(origin) + (np.array([[3, y, z]]) + 0.5) * RES
    e = np.array(origin) + (np.array([[19, y, z]]) + 0.5) * RES
    got = m.RayQuery(s, e, OCC)
    assert_same(got, before(s, e, OCC), "before")
    assert got["hit_index"][0] == -1 and got["n_visited"][0] == 17 and got["counts"][0].tolist() == [17, 0, 0, 0]
    dist_before = m.GetDistance(np.array([[11, y, z]], np.int32))
    for _ in range(3):
        m.SetOccupancy(np.array([[12, y, z]], np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)                                # no UpdateESDF
    assert np.array_equal(m.GetDistance(np.array([[11, y, z]], np.int32)), dist_before)      # the distance field is stale ...
    after = DenseModel(m)
    assert after.occ[12, y, z]
    got = m.RayQuery(s, e, OCC)                                # ... and the query is not
    assert_same(got, after(s, e, OCC), "after UpdateOccupancy")
    assert got["hit_index"][0] == 9 and got["hit_class"][0] == OCC and got["hit_vox"][0].tolist() == [12, y, z]
    assert abs(got["hit_dist"][0] - 0.9) < 1e-9
    m.UpdateESDF()
    assert_same(m.RayQuery(s, e, OCC), got, "UpdateESDF changes nothing")
    m.close()


def test_a_cast_frame_leaves_no_ray_blocked_by_unknown(hip_lib):
    """sensor consistency: after one frame (no de-duplication) and UpdateOccupancy, a query along the frame's own rays that stops at
    UNKNOWN finds nothing -- the walk is what the ray cast observed.  Map origin a multiple of the resolution, min_ray_length 0."""
    import fiesta_amd
    origin = np.zeros(3)
    m = fiesta_amd.ESDFMap(origin, RES, tuple((s - 0.5) * RES for s in DIMS))
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    size = np.array(DIMS) * RES
    rng = np.random.RandomState(4)
    sensor = size * np.array([0.4, 0.5, 0.45]) + 0.017
    pts = rng.uniform(0.3 * RES, size - 0.8 * RES, (1500, 3)).astype(np.float32)
    pts[:60] = (np.round(pts[:60] / RES) * RES).astype(np.float32)                # some on voxel faces (as far as f32 can say)
    assert (np.linalg.norm(pts - sensor, axis=1) < 9.0).all()
    m.RaycastFrame(pts, np.eye(4), sensor, 0.0, 9.0, tuple(origin - 1.0), tuple(size + 1.0), dedup=0)
    m.UpdateOccupancy(True)
    end = pts.astype(np.float64)                  # the frame's end points: T = identity applied in f64 to the f32 points
    start = np.repeat(sensor[None], len(end), 0)
    got = m.RayQuery(start, end, UNK)
    assert (got["n_visited"] >= 1).all()
    assert (got["hit_index"] == -1).all(), (np.flatnonzero(got["hit_index"] != -1)[:10], got["hit_vox"][got["hit_index"] != -1][:5])
    assert (got["counts"][:, 2] == 0).all() and (got["counts"][:, 3] == 0).all()
    assert_same(got, DenseModel(m)(start, end, UNK), "frame rays")
    m.close()


def hash_scene(shift, origin=(0.0, 0.0, 0.0)):
    """free boxes laid against and across tile faces (tiles are 16 x 16 x 32 voxels), also at negative coordinates; tiles without a
    page in between; occupied voxels on a tile face, at negative coordinates, inside"""
    import fiesta_amd
    s = np.asarray(shift, np.int32)
    m = fiesta_amd.ESDFMap(origin, RES, reserve_size=100000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    for lo, hi in (((3, 3, 3), (15, 15, 31)), ((30, 8, 8), (30, 8, 8)), ((-6, -5, -4), (2, 2, 2)), ((10, 20, 40), (22, 28, 50)),
                   ((16, 3, 20), (18, 6, 31)), ((4, 16, 30), (6, 17, 33)), ((-40, -30, -50), (-20, -10, -30))):
        m.SetOccupancyBox(s + lo, s + hi, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    S = s + np.array([(15, 8, 8), (-1, 0, 0), (8, 15, 31), (12, 24, 45), (0, 0, 0), (9, 9, 9), (-30, -20, -40), (17, 4, 25)], np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m, s


class HashModel:
    """ray_query_model on download_hash scattered into a padded array whose outside counts as unknown"""

    def __init__(self, m):
        h = m.download_hash()
        self.m = m
        self.org = h["vox"].min(0).astype(np.int64) - 1
        shape = tuple(int(v) for v in (h["vox"].max(0) - self.org + 2))
        i = tuple((h["vox"] - self.org).T)
        self.obs, self.occ = np.zeros(shape, bool), np.zeros(shape, bool)
        self.obs[i] = h["d2"] >= 0
        self.occ[i] = h["occ"] != 0

    def __call__(self, start, end, mask, walks=None):
        from fiesta_amd import ray_query_model
        return ray_query_model(self.obs, self.occ, self.m.origin, RES, start, end, mask, origin_vox=self.org, bounded=False, walks=walks)


@pytest.mark.parametrize("shift,origin", [((0, 0, 0), (0.0, 0.0, 0.0)), ((-48, 32, -64), (0.0, 0.0, 0.0)), ((-41, -23, -37), (0.03, -0.02, 0.01))])
def test_hash_block_map(hip_lib, shift, origin):
    from fiesta_amd import ray_walks
    m, sh = hash_scene(shift, origin)
    model = HashModel(m)
    rng = np.random.RandomState(2)
    org = np.asarray(origin) + sh * RES

    def vox(v):          # positions inside voxel v (scene coordinates)
        v = np.asarray(v, np.float64)
        return org + (v + rng.uniform(0.05, 0.95, v.shape)) * RES
    S, E = [], []
    S.append(vox(rng.randint(3, 16, (80, 3)) + [0, 0, 5])), E.append(vox(rng.randint(3, 16, (80, 3)) + [0, 0, 5]))      # inside one tile
    S.append(vox(rng.randint(-6, 3, (60, 3)))), E.append(vox(rng.randint(3, 30, (60, 3))))            # across tile faces, from negative coordinates
    S.append(vox(rng.randint(10, 23, (60, 3)) + [0, 10, 30])), E.append(vox(rng.randint(3, 16, (60, 3))))       # between boxes, across z = 31 | 32
    S.append(vox(rng.randint(-40, -20, (60, 3)) + [0, 10, -10])), E.append(vox(rng.randint(-6, 16, (60, 3))))   # through tiles without a page
    S.append(vox(rng.randint(60, 200, (40, 3)))), E.append(vox(rng.randint(-100, 40, (40, 3))))       # from far outside every page
    S.append(vox(rng.randint(-40, -20, (30, 3)) + [0, 10, -10])), E.append(vox(rng.randint(-40, -20, (30, 3)) + [0, 10, -10]))   # all negative
    start, end = np.concatenate(S), np.concatenate(E)
    end[11] = np.nan
    walks = ray_walks(start, end, RES)
    want = {mask: model(start, end, mask, walks) for mask in range(8)}
    assert {OCC, UNK} <= set(np.unique(want[7]["hit_class"])) and OUT not in np.unique(want[7]["hit_class"])
    assert (want[0]["counts"][:, 3] == 0).all() and (want[0]["counts"][:, [0, 2]].sum(0) > 100).all() and want[0]["counts"][:, 1].sum() > 0
    assert np.array_equal(want[4]["hit_index"], want[0]["hit_index"])                 # a hash-block map has no OUTSIDE
    for mask in range(8):
        assert_same(m.RayQuery(start, end, mask), want[mask], f"hash {shift} stop_mask {mask}")
    assert_same(device_query(m, start, end, 3), want[3], f"hash {shift} device variant")
    # far away: every page is parked and still answers
    pages = m.grid_total_size_
    m.hash_recentre(sh + np.array([3000, -3000, 3000]))
    assert m.grid_total_size_ == pages
    for mask in (0, 1, 7):
        assert_same(m.RayQuery(start, end, mask), want[mask], f"hash {shift} parked, stop_mask {mask}")
    assert_same(device_query(m, start, end, 7), want[7], f"hash {shift} parked, device variant")
    m.close()


def test_empty_hash_map_is_all_unknown(hip_lib):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=1000, mode="hash")
    got = m.RayQuery([[0.05, 0.05, 0.05], [0.05, 0.05, 0.05]], [[0.55, 0.05, 0.05], [0.55, 0.05, 0.05]], UNK)
    assert got["hit_index"].tolist() == [0, 0] and got["hit_class"].tolist() == [UNK, UNK] and got["hit_vox"].tolist() == [[0, 0, 0]] * 2
    got = m.RayQuery([[0.05, 0.05, 0.05]], [[0.55, 0.05, 0.05]], 5)
    assert got["hit_index"].tolist() == [-1] and got["counts"].tolist() == [[0, 0, 6, 0]] and got["n_visited"].tolist() == [6]
    m.close()


def test_shard_answers_for_its_own_array(hip_lib):
    """a map created as a shard (owned box + ghost layers): voxels of the global map outside its array are OUTSIDE"""
    import fiesta_amd
    gg = (32, 16, 16)
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, (15.5 * RES,) * 3, shard_lo=(16, 0, 0), global_grid=gg)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((16, 3, 3), (28, 12, 12), 0)
    m.UpdateOccupancy(True)
    for _ in range(3):
        m.SetOccupancy(np.array([[22, 7, 7], [25, 5, 9]], np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    info = m.shard_info()
    lo, dims = np.array(info["local_origin"]), tuple(int(v) for v in info["local_dims"])
    assert lo[0] == 14 and dims[0] == 18
    model = DenseModel(m, origin_vox=lo, dims=dims)
    rng = np.random.RandomState(8)
    size = np.array(gg) * RES
    start = (rng.rand(300, 3) * 1.2 - 0.1) * size
    end = (rng.rand(300, 3) * 1.2 - 0.1) * size
    for mask in range(8):
        assert_same(m.RayQuery(start, end, mask), model(start, end, mask), f"shard stop_mask {mask}")
    # a ray from the other shard's half into this one: OUTSIDE until the array begins (ghost layer at x = 14)
    s, e = np.array([[0.25, 0.75, 0.75]]), np.array([[2.55, 0.75, 0.75]])
    got = m.RayQuery(s, e, 0)
    assert got["counts"][0, 3] == 12 and got["n_visited"][0] == 24
    assert m.RayQuery(s, e, OCC)["hit_vox"].tolist() == [[22, 7, 7]]
    m.close()
