"""Optional outputs of the planner calls' host variants (include/fiesta_hip.h: path_clearance, path_cost, ray_query, reach_paths,
cluster_voxels, view_coverage): every result pointer is nullable, and what a call writes into one array must not depend on which
of the others were requested.  The host variants stage each requested array through a section of a device buffer; this file pins
that bookkeeping through the C ABI alone (ctypes on fiesta_amd._lib; the Python wrappers always request every field).

Per call, on an array map and on a hash-block map: one call with every output requested is the expected result; then one call per
field with only that field requested (reach_paths: offsets as well, which the contract requires).  The requested array must equal
the all-outputs call's bit for bit -- the header leaves one thing open, the order inside a cluster's segment of `members`, which is
compared as a set per segment -- the arrays not requested must keep their sentinel bytes, and the guard bytes behind every array
must be untouched.

The shapes are the smallest at which the section arithmetic can go wrong: odd counts, so that the 4-byte and 1-byte sections end
off an 8-byte boundary."""
import ctypes as C

import numpy as np
import pytest

from scenarios import P_DEFAULT

pytestmark = pytest.mark.gpu
RES = 0.1
DIMS = (32, 32, 64)
GUARD = 64            # bytes behind every array
SENTINEL = 0xA5


class Arrays:
    """one sentinel-filled byte buffer per field, GUARD bytes longer than the field; view(name): the field's typed array"""

    def __init__(self, spec):
        self.spec = spec        # {name: (dtype, shape)}
        self.raw = {k: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize + GUARD, SENTINEL, np.uint8) for k, (dt, shape) in spec.items()}

    def ptr(self, name, requested):
        return self.raw[name].ctypes.data if name in requested else None

    def view(self, name):
        dt, shape = self.spec[name]
        return self.raw[name][:len(self.raw[name]) - GUARD].view(dt).reshape(shape)

    def untouched(self, name):
        return bool((self.raw[name] == SENTINEL).all())

    def guard_ok(self, name):
        return bool((self.raw[name][-GUARD:] == SENTINEL).all())


def same(a, b):
    return np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b)


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_map(mode):
    """32 x 32 x 64 voxels observed free but the corner block x, y >= 24, z >= 48; 40 obstacles"""
    import fiesta_amd
    if mode == "array":
        m = fiesta_amd.ESDFMap((0, 0, 0), RES, tuple((s - 0.5) * RES for s in DIMS))
        assert m.grid_size == DIMS
    else:
        m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=100000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    for lo, hi in (((0, 0, 0), (23, 31, 63)), ((24, 0, 0), (31, 23, 63)), ((24, 24, 0), (31, 31, 47))):
        m.SetOccupancyBox(lo, hi, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    S = (np.random.RandomState(3).rand(40, 3) * np.array(DIMS)).astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


class Scene:
    def __init__(self, mode):
        from fiesta_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        self.m = make_map(mode)
        rng = np.random.RandomState(11)
        size = np.array(DIMS) * RES
        # 5 paths of 3 .. 7 waypoints (25 in all); a step that gives thousands of samples: the device pipeline, not the host cache
        counts = np.array([3, 4, 5, 6, 7])
        self.off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.w = 0.2 + rng.rand(int(counts.sum()), 3) * (size - 0.4)
        # 37 rays
        self.start, self.end = rng.rand(37, 3) * size, rng.rand(37, 3) * size
        # the frontier of the unobserved corner (a box that leaves out the map's outer shell: a hash-block map has a frontier there too),
        # sorted (the call's order is unspecified), an odd number of entries
        vox, mask = self.m.GetFrontierVoxels(lo=(20, 20, 40), hi=(30, 30, 62))
        order = np.lexsort(vox.T[::-1])
        vox, mask = vox[order], mask[order]
        if len(vox) % 2 == 0:
            vox, mask = vox[:-1], mask[:-1]
        assert 100 < len(vox) < 1000 and len(vox) % 2 == 1
        self.vox, self.mask = np.ascontiguousarray(vox), np.ascontiguousarray(mask)
        self.key = rng.randint(0, 1000, len(vox)).astype(np.int32)
        # 3 reach-path targets on the retained field of one flood from a corner of the map
        lo, hi = (0, 0, 0), tuple(d - 1 for d in DIMS)
        self.m.ReachField(np.array([[1, 1, 1]], np.int32), lo=lo, hi=hi, want_cost=False)
        self.targets = np.ascontiguousarray(self.vox[[0, len(vox) // 2, len(vox) - 1]])
        # an odd number of views towards the corner, two groups
        self.n_views = 11
        self.vpos = np.array([1.2, 1.2, 3.0]) + rng.rand(self.n_views, 3) * np.array([1.0, 1.0, 1.5])
        d = np.array([2.8, 2.8]) - self.vpos[:, :2]
        self.vdir = np.ascontiguousarray(d / np.linalg.norm(d, axis=1)[:, None])
        self.vgroup = (np.arange(self.n_views) % 2).astype(np.int32)
        half = len(vox) // 2
        self.voff = np.array([0, half, len(vox)], np.int64)

    # every call: (fields {name: (dtype, shape)}, run(arrays, requested) -> status)
    def path_clearance(self):
        n = len(self.off) - 1
        spec = {"min_dist": (np.float64, (n,)), "min_index": (np.int64, (n,)), "min_pos": (np.float64, (n, 3)), "min_grad": (np.float64, (n, 3)),
                "first_below": (np.int64, (n,)), "first_below_pos": (np.float64, (n, 3)), "n_samples": (np.int64, (n,))}

        def run(a, req):
            res = self.L.PathResult(*[a.ptr(k, req) for k in spec])
            return self.lib.fiesta_hip_path_clearance(self.m._h, p(self.w), len(self.w), p(self.off), n, 0.002, 0.5, C.byref(res))
        return spec, run, ()

    def path_cost(self):
        n, nw = len(self.off) - 1, len(self.w)
        spec = {"cost": (np.float64, (n,)), "grad": (np.float64, (nw, 3)), "length": (np.float64, (n,)), "n_below": (np.int64, (n,)),
                "n_samples": (np.int64, (n,))}

        def run(a, req):
            res = self.L.PathCostResult(*[a.ptr(k, req) for k in spec])
            return self.lib.fiesta_hip_path_cost(self.m._h, p(self.w), nw, p(self.off), n, 0.002, 0.5, C.byref(res))
        return spec, run, ()

    def ray_query(self):
        n = len(self.start)
        spec = {"n_visited": (np.int32, (n,)), "hit_index": (np.int32, (n,)), "hit_class": (np.uint8, (n,)), "hit_vox": (np.int32, (n, 3)),
                "hit_dist": (np.float64, (n,)), "counts": (np.int32, (n, 4))}

        def run(a, req):
            res = self.L.RayResult(*[a.ptr(k, req) for k in spec])
            return self.lib.fiesta_hip_ray_query(self.m._h, p(self.start), p(self.end), n, 7, C.byref(res))
        return spec, run, ()

    def reach_paths(self):
        n, cap = len(self.targets), 4096
        spec = {"offsets": (np.int64, (n + 1,)), "waypoints_vox": (np.int32, (cap, 3)), "waypoints_pos": (np.float64, (cap, 3)),
                "status": (np.int32, (n,)), "n_moves": (np.int32, (n,))}

        def run(a, req):
            res = self.L.ReachPathsResult(*[a.ptr(k, req) for k in spec])
            return self.lib.fiesta_hip_reach_paths(self.m._h, None, None, None, p(self.targets), n, 26, 0, 1, cap, C.byref(res))
        return spec, run, ("offsets",)

    def cluster_voxels(self):
        n = len(self.vox)
        spec = {"label": (np.int32, (n,)), "size": (np.int32, (n,)), "root": (np.int64, (n,)), "box_lo": (np.int32, (n, 3)),
                "box_hi": (np.int32, (n, 3)), "centroid": (np.float64, (n, 3)), "mask_or": (np.uint8, (n,)), "key_min": (np.int32, (n,)),
                "key_argmin": (np.int64, (n,)), "offsets": (np.int64, (n + 1,)), "members": (np.int64, (n,))}

        def run(a, req):
            res = self.L.ClusterResult(*[a.ptr(k, req) for k in spec])
            a.info = self.L.ClusterInfo()
            return self.lib.fiesta_hip_cluster_voxels(self.m._h, p(self.vox), p(self.mask), p(self.key), n, 6, 1, n, n, C.byref(res), C.byref(a.info))
        return spec, run, ()

    def view_coverage(self):
        n, v, g = len(self.vox), self.n_views, 2
        spec = {"view_class": (np.uint8, (v,)), "n_in_view": (np.int32, (v,)), "n_visible": (np.int32, (v,)), "cover_count": (np.int32, (n,)),
                "first_view": (np.int32, (n,)), "best_view": (np.int64, (g,)), "best_count": (np.int32, (g,))}

        def run(a, req):
            res = self.L.ViewResult(*[a.ptr(k, req) for k in spec])
            vs = self.L.ViewSet(self.vpos.ctypes.data, self.vdir.ctypes.data, self.vgroup.ctypes.data, v, None, None, 0)
            sn = self.L.ViewSensor(0.0, 4.0, 2.0, 4.0, 0.0, 1, 0, 1, 0)
            a.info = self.L.ViewInfo()
            return self.lib.fiesta_hip_view_coverage(self.m._h, p(self.vox), n, p(self.voff), None, g, 0, C.byref(vs), C.byref(sn), C.byref(res),
                                                     C.byref(a.info))
        return spec, run, ()


@pytest.fixture(scope="module", params=["array", "hash"])
def scene(request, hip_lib):
    s = Scene(request.param)
    yield s
    s.m.close()


def info_tuple(a):
    info = getattr(a, "info", None)
    return None if info is None else tuple(getattr(info, k) for k, _ in info._fields_)


@pytest.mark.parametrize("call", ["path_clearance", "path_cost", "ray_query", "reach_paths", "cluster_voxels", "view_coverage"])
def test_each_output_alone_equals_all_outputs(scene, call):
    spec, run, always = getattr(scene, call)()
    want = Arrays(spec)
    assert run(want, set(spec)) == 0, scene.L.last_error()
    assert all(want.guard_ok(k) for k in spec)
    assert not any(want.untouched(k) for k in spec), [k for k in spec if want.untouched(k)]   # (the scene gives every field something to write)
    if call == "reach_paths":
        assert 0 < want.view("offsets")[-1] < 4096
    if call == "cluster_voxels":
        assert want.info.n_clusters >= 1 and want.info.n_members == len(scene.vox)
    if call == "view_coverage":
        assert want.info.n_visible > 0
    for field in spec:
        req = {field, *always}
        got = Arrays(spec)
        assert run(got, req) == 0, (field, scene.L.last_error())
        assert info_tuple(got) == info_tuple(want), field
        for k in spec:
            assert got.guard_ok(k), (field, k)
            if k not in req:
                assert got.untouched(k), f"{call}: {k} was written although only {sorted(req)} were requested"
                continue
            g, w = got.view(k), want.view(k)
            if call == "cluster_voxels" and k == "members":   # (the order inside a cluster's segment is unspecified: fiesta_hip.h)
                off = want.view("offsets")[:want.info.n_clusters + 1]
                g, w = g.copy(), w.copy()
                for c in range(len(off) - 1):
                    g[off[c]:off[c + 1]].sort(), w[off[c]:off[c + 1]].sort()
            assert same(g, w), f"{call}: {k} requested with {sorted(req)} differs from the all-outputs call"
