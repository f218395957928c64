"""Does tests/planner_probe.py have teeth?  No GPU here: a stand-in map implements the read API the probe uses over plain numpy arrays.

The stand-in keeps what a store keeps: the FIELD (observed, occupied, distances; what download_field / download_hash, the batch
queries and the _dev path calls read), the PLANNER side (observed and occupied "bitmaps", for a hash-block map the set of pages in
its "page table"; what the planner calls read, answered by the models of fiesta_amd over these arrays) and the BRICKS (distances and
occupancy; what a scalar query and the host route of the path calls read).  With all three equal the probe passes, before and after a
transition.  Then the planner side lags behind the transition, one lag at a time -- one observed bit, one occupancy bit, one brick,
one page -- and for each the probe must raise, naming the first call that reads the stale item.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import fiesta_amd
import planner_probe as pp
from fiesta_amd.esdf_map import PATH_COST_FIELDS, PATH_FIELDS, RAY_FIELDS

TILE = np.array((16, 16, 32))
NEW_BOX = ((45, 10, 10), (55, 20, 20))      # scene coordinates: on the hash-block stand-in it lies in a tile that has no page yet


def host_array(ptr, shape, dtype):
    n = int(np.prod(shape)) if len(shape) else 1
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(int(ptr)), dtype).reshape(shape)


class Side:
    def __init__(self, obs, occ, dist):
        self.obs, self.occ, self.dist = obs.copy(), occ.copy(), dist.copy()


class StandIn:
    probe_device = "cpu"            # the probe's device buffers are host tensors: the _dev calls below read and write host pointers

    def __init__(self, kind):
        self.kind, self.mode, self.resolution = kind, "array" if kind == "dense" else "hash", pp.RES
        self.shift = np.zeros(3, np.int64) if kind == "dense" else pp.HASH_SHIFT.astype(np.int64)
        self.origin = np.zeros(3) if kind == "dense" else np.array(pp.HASH_ORIGIN)
        if kind == "dense":
            self.org, shape = np.zeros(3, np.int64), pp.SHAPE
            self.grid_size = pp.SHAPE
            self.pos_range = (self.origin, self.origin + np.array(pp.SHAPE) * pp.RES)
        else:                       # an array over every tile the scene and NEW_BOX touch
            tlo, thi = (self.shift + 0) // TILE, (self.shift + np.maximum(pp.SHAPE, np.array(NEW_BOX[1]) + 1) - 1) // TILE
            self.org, shape = tlo * TILE, tuple(int(v) for v in (thi - tlo + 1) * TILE)
            self.pos_range = None
        obs = np.zeros(shape, bool)
        obs[self.box(pp.OBS_LO, pp.OBS_HI)] = True
        obs[self.box(*pp.POCKET)] = False
        occ = np.zeros(shape, bool)
        occ[tuple((pp.OBSTACLES + self.shift - self.org).T)] = True
        self.field = Side(obs, occ, self.distances(obs, occ))
        self.sync()

    def box(self, lo, hi):
        return tuple(slice(int(a + s - o), int(b + s - o) + 1) for a, b, s, o in zip(lo, hi, self.shift, self.org))

    def distances(self, obs, occ):
        d = ndimage.distance_transform_edt(~occ) * pp.RES if occ.any() else np.full(occ.shape, 10000.0)
        return np.where(obs, d, 10000.0)

    def tiles(self, obs):
        if self.kind == "dense":
            return set()
        t = obs.reshape(obs.shape[0] // 16, 16, obs.shape[1] // 16, 16, obs.shape[2] // 32, 32).any(axis=(1, 3, 5))
        return {tuple(int(v) for v in i) for i in np.argwhere(t)}

    # ---- state changes ----
    def transition(self):
        """first observations (the slab; on a hash-block map also a box in a tile without a page), 20 inserts, 20 deletes"""
        f = self.field
        f.obs[self.box(*pp.SLAB)] = True
        if self.kind == "hash":
            f.obs[self.box(*NEW_BOX)] = True
        f.occ[tuple((pp.INSERTS + self.shift - self.org).T)] = True
        f.occ[tuple((pp.DELETES + self.shift - self.org).T)] = False
        f.dist = self.distances(f.obs, f.occ)

    def sync(self):
        """what every state-changing call of a store owes its readers"""
        f = self.field
        self.planner, self.bricks, self.pages = Side(f.obs, f.occ, f.dist), Side(f.obs, f.occ, f.dist), self.tiles(f.obs)

    # ---- the field side ----
    def download_field(self, want=("d2", "occ")):
        f = self.field
        return {"d2": np.where(f.obs, 1, -1).astype(np.int32).reshape(-1), "occ": f.occ.astype(np.uint8).reshape(-1)}

    def download_hash(self):
        f = self.field
        keep = np.zeros(f.obs.shape, bool)
        for t in self.tiles(f.obs):
            keep[tuple(slice(int(a * e), int((a + 1) * e)) for a, e in zip(t, TILE))] = True
        i = np.argwhere(keep)
        at = tuple(i.T)
        return {"vox": (i + self.org).astype(np.int32), "d2": np.where(f.obs[at], 1, -1).astype(np.int32), "coc": np.zeros((len(i), 3), np.int32),
                "occ": f.occ[at].astype(np.uint8)}

    def _lookup(self, side, vox, name, outside):
        i = np.asarray(vox, np.int64).reshape(-1, 3) - self.org
        inside = np.all((i >= 0) & (i < np.array(side.obs.shape)), axis=1)
        ic = np.where(inside[:, None], i, 0)
        return np.where(inside, getattr(side, name)[ic[:, 0], ic[:, 1], ic[:, 2]], outside)

    def _query(self, where, name, outside, dtype):
        a = np.asarray(where)
        v = a.reshape(-1, 3)
        out = self._lookup(self.bricks if len(v) <= 8 else self.field, v, name, outside).astype(dtype)    # (kHostQueries = 8)
        return out[0].item() if a.ndim == 1 else out

    def GetDistance(self, where):
        return self._query(where, "dist", 10000.0, np.float64)

    def GetOccupancy(self, where):
        return self._query(where, "occ", 0, np.int32)

    def _trilinear(self, side, pos):
        pos = np.asarray(pos, np.float64).reshape(-1, 3)
        q = (pos - self.origin) / self.resolution - 0.5
        i0 = np.floor(q).astype(np.int64)
        t = q - i0
        c = {(a, b, e): self._lookup(side, i0 + (a, b, e), "dist", 10000.0) for a in (0, 1) for b in (0, 1) for e in (0, 1)}
        wx, wy, wz = [(1 - t[:, k], t[:, k]) for k in range(3)]
        d = sum(wx[a] * wy[b] * wz[e] * c[a, b, e] for a, b, e in c)
        g = np.stack([sum((2 * a - 1) * wy[b] * wz[e] * c[a, b, e] for a, b, e in c), sum((2 * b - 1) * wx[a] * wz[e] * c[a, b, e] for a, b, e in c),
                      sum((2 * e - 1) * wx[a] * wy[b] * c[a, b, e] for a, b, e in c)], 1) / self.resolution
        return d, g

    def GetDistWithGradTrilinear(self, pos):
        return self._trilinear(self.bricks if len(np.asarray(pos).reshape(-1, 3)) <= 8 else self.field, pos)

    def synchronize(self):
        pass

    # ---- the planner side ----
    def _seen(self):
        p = self.planner
        if self.kind == "dense":
            return p.obs, p.occ
        paged = np.zeros(p.obs.shape, bool)
        for t in self.pages:
            paged[tuple(slice(int(a * e), int((a + 1) * e)) for a, e in zip(t, TILE))] = True
        return p.obs & paged, p.occ & paged

    def _kw(self):
        return dict(origin_vox=tuple(int(v) for v in self.org), bounded=self.kind == "dense")

    def GetFrontierVoxels(self, lo=None, hi=None, min_clearance=0.0, want_mask=True):
        obs, occ = self._seen()
        vox, mask = fiesta_amd.frontier_model(obs, occ, self.field.dist, lo, hi, min_clearance, **self._kw())
        return np.asarray(vox, np.int32).reshape(-1, 3), np.asarray(mask, np.uint8)

    def RayQuery(self, start, end, stop_mask=7):
        obs, occ = self._seen()
        return fiesta_amd.ray_query_model(obs, occ, self.origin, self.resolution, start, end, stop_mask, pos_range=self.pos_range, **self._kw())

    def RayQueryDevice(self, start_ptr, end_ptr, n, stop_mask=7, out=None):
        got = self.RayQuery(host_array(start_ptr, (n, 3), np.float64), host_array(end_ptr, (n, 3), np.float64), stop_mask)
        for name, dtype, shape in RAY_FIELDS:
            host_array(out[name], (n,) + shape, dtype)[...] = got[name]

    def ReachField(self, seeds, lo=None, hi=None, targets=None, min_clearance=0.0, connectivity=26, flags=0, want_cost=True):
        obs, occ = self._seen()
        return fiesta_amd.reach_model(obs, occ, seeds, self.field.dist, lo, hi, min_clearance, connectivity, flags, targets, tuple(int(v) for v in self.org))

    def FreeBoxes(self, seeds, lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0):
        obs, occ = self._seen()
        return fiesta_amd.free_box_model(obs, occ, seeds, self.field.dist, lo, hi, max_grow, min_clearance, flags, resolution=self.resolution,
                                         origin=tuple(self.origin), **self._kw())

    def PathCorridor(self, waypoints_vox, offsets, lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0, want_pos=True):
        obs, occ = self._seen()
        return fiesta_amd.corridor_model(obs, occ, waypoints_vox, offsets, self.field.dist, lo, hi, max_grow, min_clearance, flags,
                                         resolution=self.resolution, origin=tuple(self.origin), **self._kw())

    def ViewCoverage(self, vox, pos=None, dir=None, **sensor):
        obs, occ = self._seen()
        return fiesta_amd.view_coverage_model(obs, occ, self.origin, self.resolution, vox, pos=pos, dir=dir, dist=self.field.dist,
                                              pos_range=self.pos_range, **sensor, **self._kw())

    def _path_clearance(self, side, w, off, step, margin):
        class Route:
            GetDistWithGradTrilinear = staticmethod(lambda pos: self._trilinear(side, pos))
        return pp.t_path.model(Route, w, off, step, margin)

    def PathClearance(self, w, off, step, margin=0.0):
        return self._path_clearance(self.bricks, w, off, step, margin)          # (at most 256 samples: the host route)

    def PathClearanceDevice(self, w_ptr, n_w, off_ptr, n_paths, step, margin=0.0, out=None):
        got = self._path_clearance(self.field, host_array(w_ptr, (n_w, 3), np.float64), host_array(off_ptr, (n_paths + 1,), np.int64), step, margin)
        for name, dtype, shape in PATH_FIELDS:
            host_array(out[name], (n_paths,) + shape, dtype)[...] = got[name]

    def PathCost(self, w, off, step, margin):
        return fiesta_amd.path_cost_model(lambda pos: self._trilinear(self.bricks, pos), w, off, step, margin)

    def PathCostDevice(self, w_ptr, n_w, off_ptr, n_paths, step, margin, out=None):
        got = fiesta_amd.path_cost_model(lambda pos: self._trilinear(self.field, pos), host_array(w_ptr, (n_w, 3), np.float64),
                                         host_array(off_ptr, (n_paths + 1,), np.int64), step, margin)
        for name, dtype, per, shape in PATH_COST_FIELDS:
            host_array(out[name], (n_paths if per == "path" else n_w,) + shape, dtype)[...] = got[name]


def layout(kind):
    return pp.Layout.scene() if kind == "dense" else pp.Layout.scene(pp.HASH_SHIFT)


_moved = {}


def moved_stand_in(kind):
    """a stand-in probed once, then moved on by the transition; with it the planner side, bricks and pages of before"""
    if kind not in _moved:
        m = StandIn(kind)
        d0 = pp.probe(m, kind, layout(kind), "before")
        old = m.planner, m.bricks, m.pages
        m.transition()
        _moved[kind] = kind, m, d0, old
    return _moved[kind]


@pytest.fixture(params=["dense", "hash"])
def moved(request):
    return moved_stand_in(request.param)


def lagging(m, old):
    """everything follows the transition; returns the old planner side, bricks and pages for one item to be put back"""
    m.sync()
    return old


def test_the_probe_passes_while_every_side_follows(moved):
    kind, m, d0, old = moved
    m.sync()
    d1 = pp.probe(m, kind, layout(kind), "after")
    pp.assert_differs(d0, d1, pp.DIGEST_KEYS, f"{kind} stand-in")
    with pytest.raises(AssertionError, match="vacuous"):
        pp.assert_differs(d1, d1, ("frontier",), "no transition")
    with pytest.raises(AssertionError, match="differs from the first"):
        pp.assert_equal(d0, d1, "after a transition")
    pp.assert_equal(d1, pp.probe(m, kind, layout(kind), "again"))


def test_a_stale_observed_bit_shows_in_the_frontier_call(moved):
    kind, m, d0, (planner, bricks, pages) = moved
    lagging(m, None)
    v = tuple(np.array((30, 30, 41)) + m.shift - m.org)                 # a voxel of the slab: observed by the transition
    assert m.field.obs[v] and not planner.obs[v]
    m.planner.obs[v] = planner.obs[v]
    with pytest.raises(AssertionError, match=r"GetFrontierVoxels\(\)"):
        pp.probe(m, kind, layout(kind), "stale observed bit")


def test_a_stale_occupancy_bit_shows_in_the_ray_query(moved):
    kind, m, d0, (planner, bricks, pages) = moved
    lagging(m, None)
    L = layout(kind)
    hits = m.RayQuery(m.origin + L.ray_start * pp.RES, m.origin + L.ray_end * pp.RES, 7)
    ins = {tuple(r) for r in (pp.INSERTS + m.shift).tolist()}
    hit = [tuple(r) for r, c in zip(hits["hit_vox"].tolist(), hits["hit_class"]) if c == 1 and tuple(r) in ins]
    assert hit, "no probe ray ends on an inserted obstacle"
    v = tuple(np.array(hit[0]) - m.org)
    assert m.field.occ[v] and not planner.occ[v]
    m.planner.occ[v] = planner.occ[v]
    with pytest.raises(AssertionError, match=r"RayQuery\(stop_mask 7\)"):
        pp.probe(m, kind, layout(kind), "stale occupancy bit")


def test_a_stale_brick_shows_in_the_host_route_of_the_path_call(moved):
    kind, m, d0, (planner, bricks, pages) = moved
    lagging(m, None)
    L = layout(kind)
    pos, _ = fiesta_amd.path_samples(m.origin + L.path_w * pp.RES, L.path_off, pp.PATH_STEP)
    i = np.floor((pos - m.origin) / pp.RES).astype(np.int64) - m.org
    changed = m.field.dist[tuple(i.T)] != bricks.dist[tuple(i.T)]
    assert changed.any(), "the transition moved no distance under the probe's paths"
    b = tuple(slice(int(c) // 16 * 16, int(c) // 16 * 16 + 16) for c in i[changed][0])      # the 16^3 brick of the first such sample
    m.bricks.dist[b], m.bricks.occ[b] = bricks.dist[b], bricks.occ[b]
    with pytest.raises(AssertionError, match=r"PathClearance \(host route"):
        pp.probe(m, kind, layout(kind), "stale brick")


def test_a_stale_brick_under_a_scalar_query_only(moved):
    """with the probe's paths folded into the scene's lowest brick, a stale brick elsewhere is read by the scalar queries alone"""
    kind, m, d0, (planner, bricks, pages) = moved
    lagging(m, None)
    L = layout(kind)
    L.path_w = np.array([(4.3, 4.2, 4.4), (9.6, 7.1, 8.7), (12.2, 5.3, 11.9), (5.5, 9.5, 5.2), (5.5, 9.5, 12.8), (11.2, 11.1, 8.3), (6.9, 4.8, 4.1)]) + m.shift
    L.path_off = np.array([0, 3, 5, 7], np.int64)
    corner = tuple((np.array((4, 4, 4)) + m.shift - m.org) // 16)
    for v in L.scalar_vox - m.org:
        if tuple(v // 16) != corner and m.field.dist[tuple(v)] != bricks.dist[tuple(v)]:
            break
    else:
        pytest.fail("no scalar voxel of the layout lies on a distance that changed")
    b = tuple(slice(int(c) // 16 * 16, int(c) // 16 * 16 + 16) for c in v)
    m.bricks.dist[b], m.bricks.occ[b] = bricks.dist[b], bricks.occ[b]
    with pytest.raises(AssertionError, match=r"GetDistance\(\[.*\]\) alone"):
        pp.probe(m, kind, L, "stale brick under a scalar voxel")


def test_a_page_missing_from_the_table_shows_in_the_frontier_call():
    kind, m, d0, (planner, bricks, pages) = moved_stand_in("hash")
    lagging(m, None)
    fresh = m.pages - pages
    assert fresh, "the transition added no page"
    m.pages = m.pages - {sorted(fresh)[0]}
    with pytest.raises(AssertionError, match=r"GetFrontierVoxels\(\)"):
        pp.probe(m, kind, layout(kind), "page missing")
