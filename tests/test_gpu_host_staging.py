"""Staging of the older host-pointer calls (include/fiesta_hip.h: set_occupancy_vox / pos, get_distance_vox / pos, get_dist_grad,
get_occupancy_vox / pos, download_field, download_hash, get_occupied_voxels, get_point_cloud, get_slice_marker and the host form of
get_frontier_voxels).  Each of them moves its host arrays through sections of the two device buffers the planner calls' host variants
use as well (planner.hpp: Staging); test_gpu_optional_outputs.py pins that bookkeeping for the planner calls, this file for the
rest, through the C ABI alone (ctypes on fiesta_amd._lib), on that file's map and with its sentinel / guard arrays.

What is pinned: a nullable output alone equals the same output of the call that asks for everything, and nothing else is written;
a compaction getter writes exactly min(total, capacity) entries, a subset of the full set, and returns the same total for every
capacity; entry i of a batch of 9 or 1031 (odd, so the 4-byte sections end off an 8-byte boundary; 9 is the first size the device
serves, 1031 lies beyond a fresh buffer's first 1024 bytes in every section) equals the same query asked alone, which the host
brick cache answers (test_gpu_dense_parity.py / test_gpu_hash_parity.py hold the two routes equal); calls of different sizes and a
planner call in between, all sharing the two buffers, answer as they do on a fresh map; get_dist_grad without a gradient array
returns the distances of the call with one.

Where the header leaves the order of a result unspecified (the frontier call, the compaction getters) results are compared as
sets of entries."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_optional_outputs import DIMS, GUARD, RES, SENTINEL, Arrays, make_map, p, same

pytestmark = pytest.mark.gpu
UNDEFINED = -10000
SIZES = (9, 1031)
FRONTIER_BOX = ((20, 20, 40), (30, 30, 62))   # (leaves out the map's outer shell: a hash-block map has a frontier there too)


class Store:
    def __init__(self, mode):
        from fiesta_amd import _lib
        self.L, self.lib, self.mode = _lib, _lib.load(), mode
        self.m = make_map(mode)
        rng = np.random.RandomState(23)
        size = np.array(DIMS) * RES
        n = max(SIZES)
        # all over the map, faces included, some outside; voxels likewise
        self.pos = rng.rand(n, 3) * size
        self.pos[::97] += 30.0
        self.vox = rng.randint(0, min(DIMS), (n, 3)).astype(np.int32) * np.array([1, 1, 2], np.int32)
        self.vox[::89] += 70
        self.rays = (rng.rand(5, 3) * size, rng.rand(5, 3) * size)
        self._alone = {}

    def close(self):
        self.m.close()

    def ok(self, status):
        assert status == 0, self.L.last_error()

    # ---- the batched queries: name -> (input, {output: (dtype, trailing shape)}) ----
    QUERIES = {"get_distance_vox": ("vox", {"out": (np.float64, ())}), "get_distance_pos": ("pos", {"out": (np.float64, ())}),
               "get_occupancy_vox": ("vox", {"out": (np.int32, ())}), "get_occupancy_pos": ("pos", {"out": (np.int32, ())}),
               "get_dist_grad": ("pos", {"dist": (np.float64, ()), "grad": (np.float64, (3,))})}

    def query(self, name, lo, hi, m=None, skip=()):
        """entries lo .. hi - 1 of the query set in one call -> Arrays (guards checked)"""
        src, outs = self.QUERIES[name]
        x = np.ascontiguousarray(getattr(self, src)[lo:hi])
        a = Arrays({k: (dt, (hi - lo,) + tail) for k, (dt, tail) in outs.items()})
        req = set(outs) - set(skip)
        self.ok(getattr(self.lib, "fiesta_hip_" + name)((m or self.m)._h, p(x), hi - lo, *[a.ptr(k, req) for k in outs]))
        assert all(a.guard_ok(k) for k in outs), name
        return a

    def alone(self, name):
        """every entry of the query set asked alone (the host brick cache), once per store"""
        if name not in self._alone:
            parts = [self.query(name, i, i + 1) for i in range(max(SIZES))]
            self._alone[name] = {k: np.concatenate([q.view(k) for q in parts]) for k in self.QUERIES[name][1]}
        return self._alone[name]

    def ray_query(self, m=None):
        n = len(self.rays[0])
        spec = {"n_visited": (np.int32, (n,)), "hit_index": (np.int32, (n,)), "hit_class": (np.uint8, (n,)), "hit_vox": (np.int32, (n, 3)),
                "hit_dist": (np.float64, (n,)), "counts": (np.int32, (n, 4))}
        a = Arrays(spec)
        res = self.L.RayResult(*[a.ptr(k, spec) for k in spec])
        self.ok(self.lib.fiesta_hip_ray_query((m or self.m)._h, p(self.rays[0]), p(self.rays[1]), n, 7, C.byref(res)))
        assert all(a.guard_ok(k) for k in spec)
        return a

    # ---- the getters with nullable outputs: name -> (fields, run(arrays, requested)) ----
    def download_field(self):
        n = int(np.prod(DIMS))
        spec = {"d2": (np.int32, (n,)), "coc": (np.int32, (n, 3)), "occ": (np.uint8, (n,)), "logodds": (np.float64, (n,))}
        return spec, lambda a, req: self.lib.fiesta_hip_download_field(self.m._h, *[a.ptr(k, req) for k in spec])

    def download_hash(self):
        n = C.c_int64(0)
        self.ok(self.lib.fiesta_hip_download_hash(self.m._h, C.byref(n), None, None, None, None))
        n = n.value
        assert n > 0
        spec = {"vox": (np.int32, (n, 3)), "d2": (np.int32, (n,)), "coc": (np.int32, (n, 3)), "occ": (np.uint8, (n,))}

        def run(a, req):
            k = C.c_int64(0)
            st = self.lib.fiesta_hip_download_hash(self.m._h, C.byref(k), *[a.ptr(f, req) for f in spec])
            assert k.value == n
            return st
        return spec, run

    # ---- the compaction getters: name -> ({field: (dtype, entries per item)}, run(arrays, requested, capacity) -> total) ----
    def compaction(self, name):
        lo, hi = (np.array(b, np.int32) for b in FRONTIER_BOX)
        spec, call = {
            "get_occupied_voxels": ({"vox": (np.int32, 3)}, lambda ptr, cap, n: self.lib.fiesta_hip_get_occupied_voxels(self.m._h, *ptr, cap, n)),
            "get_point_cloud": ({"xyz": (np.float32, 3)}, lambda ptr, cap, n: self.lib.fiesta_hip_get_point_cloud(self.m._h, 0, DIMS[2] - 1, *ptr, cap, n)),
            "get_slice_marker": ({"xyz": (np.float64, 3), "rgba": (np.float32, 4)},
                                 lambda ptr, cap, n: self.lib.fiesta_hip_get_slice_marker(self.m._h, 10, 1.0, *ptr, cap, n)),
            "get_frontier_voxels": ({"vox": (np.int32, 3), "mask": (np.uint8, 1)},
                                    lambda ptr, cap, n: self.lib.fiesta_hip_get_frontier_voxels(self.m._h, p(lo), p(hi), 0.0, *ptr, cap, n)),
        }[name]

        def run(a, req, cap):
            n = C.c_int64(-1)
            self.ok(call([a.ptr(k, req) for k in spec], cap, C.byref(n)))
            return n.value
        return spec, run


@pytest.fixture(scope="module")
def stores(hip_lib):
    s = {mode: Store(mode) for mode in ("array", "hash")}
    yield s
    for v in s.values():
        v.close()


def item_bytes(a, spec, k):
    """a compaction getter's array as one row of bytes per item"""
    dt, w = spec[k]
    return a.raw[k][:len(a.raw[k]) - GUARD].reshape(-1, w * np.dtype(dt).itemsize)


def entries(a, spec, count):
    """the first `count` items as a set of byte strings (all fields of an item together)"""
    return {r.tobytes() for r in np.concatenate([item_bytes(a, spec, k)[:count] for k in spec], axis=1)}


def written(a, spec, k):
    """per item: does it hold anything but sentinel bytes?"""
    return (item_bytes(a, spec, k) != SENTINEL).any(axis=1)


# ---- 1. optional outputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,call", [("array", "download_field"), ("hash", "download_hash")])
def test_download_each_output_alone_equals_all_outputs(stores, mode, call):
    s = stores[mode]
    spec, run = getattr(s, call)()
    want = Arrays(spec)
    s.ok(run(want, set(spec)))
    assert all(want.guard_ok(k) for k in spec) and not any(want.untouched(k) for k in spec)
    for field in spec:
        got = Arrays(spec)
        s.ok(run(got, {field}))
        for k in spec:
            assert got.guard_ok(k), (field, k)
            if k != field:
                assert got.untouched(k), f"{call}: {k} was written although only {field} was requested"
        assert same(got.view(field), want.view(field)), f"{call}: {field} alone differs from the all-outputs call"


@pytest.mark.parametrize("mode", ["array", "hash"])
def test_frontier_each_output_alone_equals_all_outputs(stores, mode):
    s = stores[mode]
    spec, run = s.compaction("get_frontier_voxels")
    total = run(Arrays({k: (dt, (0, w)) for k, (dt, w) in spec.items()}), set(), 0)
    assert total > 100
    shape = {k: (dt, (total, w)) for k, (dt, w) in spec.items()}
    want = Arrays(shape)
    assert run(want, set(spec), total) == total
    assert all(want.guard_ok(k) for k in spec) and all(written(want, spec, k).all() for k in spec)
    for field in spec:   # (the order of the entries is unspecified: fiesta_hip.h)
        got = Arrays(shape)
        assert run(got, {field}, total) == total
        for k in spec:
            assert got.guard_ok(k), (field, k)
            if k != field:
                assert got.untouched(k), f"get_frontier_voxels: {k} was written although only {field} was requested"
        g, w = (x.view(field).reshape(total, -1) for x in (got, want))
        assert np.array_equal(g[np.lexsort(g.T[::-1])], w[np.lexsort(w.T[::-1])]), field


# ---- 2. truncation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,call", [("array", "get_occupied_voxels"), ("array", "get_point_cloud"), ("hash", "get_point_cloud"),
                                       ("array", "get_slice_marker"), ("hash", "get_slice_marker"),
                                       ("array", "get_frontier_voxels"), ("hash", "get_frontier_voxels")])
def test_truncation(stores, mode, call):
    s = stores[mode]
    spec, run = s.compaction(call)
    total = run(Arrays({k: (dt, (0, w)) for k, (dt, w) in spec.items()}), set(), 0)   # (null arrays: the sizing call)
    assert total >= 3
    shape = {k: (dt, (total, w)) for k, (dt, w) in spec.items()}
    full = Arrays(shape)
    assert run(full, set(spec), total) == total
    everything = entries(full, spec, total)
    assert len(everything) == total and all(written(full, spec, k).all() for k in spec)
    for cap in (total, total - 1, 1, 0):
        got = Arrays(shape)
        assert run(got, set(spec), cap) == total, cap
        for k in spec:
            w = written(got, spec, k)
            assert w[:cap].all() and not w[cap:].any() and got.guard_ok(k), (call, cap, k)   # exactly min(total, capacity) entries
        part = entries(got, spec, cap)
        assert len(part) == cap and part <= everything, (call, cap)


# ---- 3. section arithmetic --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(Store.QUERIES))
@pytest.mark.parametrize("mode", ["array", "hash"])
def test_batch_entry_equals_the_query_asked_alone(stores, mode, name, n):
    s = stores[mode]
    alone, got = s.alone(name), s.query(name, 0, n)
    for k in alone:
        assert same(got.view(k), alone[k][:n]), (name, k, np.flatnonzero((got.view(k) != alone[k][:n]).reshape(n, -1).any(axis=1))[:5])
    if name.startswith("get_distance"):   # (the scene is not degenerate: many distances, and voxels that have none)
        assert len(np.unique(alone["out"])) > 20 and (np.abs(alone["out"]) == -UNDEFINED).any()


def counts_by_voxel(s, m):
    """pending (hit, miss) per voxel in an order both stores define: rows (x, y, z, hit, miss), sorted"""
    if s.mode == "array":
        n = int(np.prod(DIMS))
        hit, miss = np.empty(n, np.int32), np.empty(n, np.int32)
        s.ok(s.lib.fiesta_hip_download_counts(m._h, p(hit), p(miss)))
        return np.stack([hit, miss], axis=1)
    k = C.c_int64(0)
    s.ok(s.lib.fiesta_hip_download_hash(m._h, C.byref(k), None, None, None, None))
    vox, hit, miss = np.empty((k.value, 3), np.int32), np.empty(k.value, np.int32), np.empty(k.value, np.int32)
    s.ok(s.lib.fiesta_hip_download_hash(m._h, C.byref(k), p(vox), None, None, None))
    s.ok(s.lib.fiesta_hip_download_counts(m._h, p(hit), p(miss)))
    rows = np.concatenate([vox, hit[:, None], miss[:, None]], axis=1)
    return rows[np.lexsort(rows[:, :3].T[::-1])]


def fuse(s, m):
    ni, nd, any_ = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    counts = counts_by_voxel(s, m)
    s.ok(s.lib.fiesta_hip_update_occupancy(m._h, 1, C.byref(ni), C.byref(nd), C.byref(any_)))
    return counts, (ni.value, nd.value, any_.value)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["vox", "pos"])
@pytest.mark.parametrize("mode", ["array", "hash"])
def test_observe_batch_equals_the_device_variant(stores, mode, form, n):
    import torch
    s = stores[mode]
    rng = np.random.RandomState(100 + n)
    occ = rng.randint(0, 2, n).astype(np.int32)
    if form == "vox":
        where = (rng.rand(n, 3) * np.array(DIMS)).astype(np.int32)
        vox, fed = where, np.ones(n, bool)
    else:
        where = 0.05 + rng.rand(n, 3) * (np.array(DIMS) * RES - 0.2)
        where[::7, 0] = -0.35        # outside an array map (rejected there), voxel -4 of an unbounded one
        occ[3::11] = 2               # not an observation: rejected by both
        vox = np.floor(where / RES).astype(np.int32)
        fed = (occ != 2) & ((mode == "hash") | (where[:, 0] >= 0))
    want_ret = np.empty(n, np.int32)
    s.ok(s.lib.fiesta_hip_voxel_key(s.m._h, p(vox), n, p(want_ret)))
    want_ret[~fed] = UNDEFINED
    host, dev = make_map(mode), make_map(mode)
    try:
        ret = Arrays({"ret": (np.int32, (n,))})
        s.ok(getattr(s.lib, "fiesta_hip_set_occupancy_" + form)(host._h, p(where), p(occ), n, ret.ptr("ret", {"ret"})))
        assert ret.guard_ok("ret") and np.array_equal(ret.view("ret"), want_ret)
        dv, do = torch.from_numpy(np.ascontiguousarray(vox[fed])).cuda(), torch.from_numpy(np.ascontiguousarray(occ[fed])).cuda()
        torch.cuda.synchronize()
        s.ok(s.lib.fiesta_hip_set_occupancy_vox_dev(dev._h, C.c_void_p(dv.data_ptr()), C.c_void_p(do.data_ptr()), int(fed.sum())))
        (ch, qh), (cd, qd) = fuse(s, host), fuse(s, dev)
        assert np.array_equal(ch, cd) and qh == qd, (qh, qd)
        assert ch[:, -1].sum() == fed.sum()   # (every observation that was fed is counted once)
    finally:
        host.close(), dev.close()


# ---- 4. buffer sharing and growth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["array", "hash"])
def test_calls_sharing_the_buffers_answer_as_on_a_fresh_map(stores, mode):
    s = stores[mode]
    small = lambda m: s.query("get_dist_grad", 0, SIZES[0], m)            # noqa: E731
    large = lambda m: s.query("get_distance_pos", 0, SIZES[1], m)         # noqa: E731
    occ = lambda m: s.query("get_occupancy_vox", 0, SIZES[1], m)          # noqa: E731
    steps = [small, s.ray_query, large, s.ray_query, small, occ, s.ray_query, small]
    want = {}
    for f in set(steps):   # each call alone on a map of its own
        m = make_map(mode)
        try:
            want[f] = f(m)
        finally:
            m.close()
    m = make_map(mode)
    try:
        for i, f in enumerate(steps):
            got = f(m)
            for k in got.spec:
                assert same(got.view(k), want[f].view(k)), (i, k)
    finally:
        m.close()


# ---- 5. get_dist_grad without a gradient array ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", ["array", "hash"])
def test_dist_grad_with_null_grad(stores, mode, n):
    s = stores[mode]
    both, dist_only = s.query("get_dist_grad", 0, n), s.query("get_dist_grad", 0, n, skip=("grad",))   # (query() checks the status)
    assert dist_only.untouched("grad") and not both.untouched("grad")
    assert same(dist_only.view("dist"), both.view("dist"))
