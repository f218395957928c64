"""What the planner calls see of a map, held against what the map reports of itself -- a helper of tests/test_gpu_planner_map_states.py
(the probe after every state change) and tests/test_planner_probe_cpu.py (the probe against a stand-in whose planner side lags).

A planner call reads redundant state: the dense store's observed / occupied bitmaps, the hash-block store's page table,
and -- the scalar queries and the host route of the path calls -- a host-side cache of bricks that an epoch keeps valid.  probe()

  1. reads the map through the calls that predate the planner API: download_field / download_hash, GetDistance and
     GetDistWithGradTrilinear in batches of more than 8 positions (the device route, never the brick cache), into the obs / occ / dist
     arrays of DenseModel / HashModel of tests/test_gpu_frontiers.py and tests/test_gpu_ray_queries.py;
  2. runs a fixed, small set of planner calls and compares each with its model in fiesta_amd on those arrays: tolerance zero, no entry
     excluded (PathCost: the summation bound of tests/test_gpu_path_cost.py);
  3. returns a digest of the EXPECTED values (frontier rows, ray hit classes, n_traversable, 8 scalar distances), by which a caller
     shows that a transition changed something.

Every failed comparison is an AssertionError whose message names the call.  The lists are laid out by a Layout in scene voxel
coordinates; the scene itself (48 x 40 x 72 voxels at 0.1 m, partly observed, about 60 obstacles) is built here as well.
"""
import numpy as np

import test_gpu_corridor as t_corridor
import test_gpu_frontiers as t_frontiers
import test_gpu_path_cost as t_path_cost
import test_gpu_path_queries as t_path
import test_gpu_ray_queries as t_rays
import test_gpu_views as t_views
from scenarios import P_DEFAULT, all_voxels
from test_gpu_updated_unit import pick

RES = 0.1
SHAPE = (48, 40, 72)
OBS_LO, OBS_HI = (3, 3, 3), (44, 36, 40)          # observed free; the boundary in z lies at 40 | 41: the words z = 32 .. 63 are partly observed
POCKET = ((20, 18, 30), (22, 20, 32))             # 3 x 3 x 3, never observed, across the word boundary z = 31 | 32
SLAB = ((3, 3, 41), (44, 36, 47))                 # observed later: first observations
HASH_SHIFT = np.array((-20, 8, -40), np.int32)    # the scene on a hash-block map: across tile faces (16 x 16 x 32) and negative coordinates
HASH_ORIGIN = (0.03, -0.02, 0.01)
THROUGH = 1
REACH_SEED = (12, 10, 25)
REACH_BOX = ((8, 6, 18), (35, 33, 49))            # 28 x 28 x 32 voxels: the pocket, the observed / unknown boundary, z = 31 | 32
VIEW_VOX = ((10, 10, 20), (30, 12, 25), (15, 30, 35), (35, 30, 15), (24, 19, 36), (12, 20, 38), (38, 8, 38), (25, 25, 10))
SCALAR_VOX = ((12, 10, 26), (21, 19, 29), (30, 30, 40), (30, 30, 41), (5, 5, 5), (40, 33, 12), (24, 20, 33), (16, 24, 20))
NEXT_TO_SCALAR = (13, 10, 26)                     # free in every scene: the one-voxel insert beside SCALAR_VOX[0]


def _free_for_obstacles(v):
    """where pick() may put an obstacle: inside the observed box, off the pocket and off every voxel the layout stands on"""
    v = np.asarray(v, np.int64)
    ok = np.all((v >= np.array(OBS_LO) + 1) & (v <= np.array(OBS_HI) - 1), axis=1)
    ok &= ~np.all((v >= np.array(POCKET[0]) - 1) & (v <= np.array(POCKET[1]) + 1), axis=1)
    for r in (REACH_SEED, NEXT_TO_SCALAR) + VIEW_VOX + SCALAR_VOX:
        ok &= np.abs(v - np.array(r)).max(1) > 0
    return ok


OBSTACLES, INSERTS = pick(SHAPE, (60, 20), 41, _free_for_obstacles)      # the scene's obstacles; what the deltas insert
DELETES = OBSTACLES[:20]                                                 # ... and delete


class Layout:
    """the probe's fixed lists, in map voxel coordinates (positions: voxel units, metres = origin + v * resolution)"""

    @classmethod
    def scene(cls, shift=(0, 0, 0)):
        """for the scene above, moved by `shift` voxels"""
        L, rng = cls(), np.random.RandomState(1234)
        s = np.asarray(shift, np.int64)
        dims, olo, ohi = np.array(SHAPE), np.array(OBS_LO), np.array(OBS_HI)
        L.frontier_box = (s + (5, 4, 10), s + (40, 30, 50))            # z bounds are no multiples of 32: the box cuts bitmap words
        inside = lambda n: olo + rng.rand(n, 3) * (ohi - olo + 1)   # noqa: E731
        S, E = [], []
        S.append(1 + rng.rand(60, 3) * (dims - (2, 2, 12))), E.append(1 + rng.rand(60, 3) * (dims - (2, 2, 12)))     # anywhere
        a, aim = inside(50), np.concatenate([OBSTACLES[:30], INSERTS]) + 0.5
        S.append(a), E.append(a + (aim - a) * 1.25)                                     # at obstacles, present or to come
        b = inside(40)
        b[:, 2] = 41 + rng.rand(40) * 21
        S.append(inside(40)), E.append(b)                                               # across the observed / unknown boundary in z
        S.append(inside(30)), E.append(rng.rand(30, 3) * (dims + 30) - 15)              # out of the map
        c = np.floor(inside(20)) + 0.5
        lo, hi = c.copy(), c.copy()
        lo[:, 2], hi[:, 2] = 26 + rng.rand(20) * 5.9, 32.1 + rng.rand(20) * 37.8
        S.append(lo), E.append(hi)                                                      # along z across z = 31 | 32 and 63 | 64
        L.ray_start, L.ray_end = np.concatenate(S) + s, np.concatenate(E) + s
        L.reach_seed, L.reach_box = s + REACH_SEED, (s + REACH_BOX[0], s + REACH_BOX[1])
        special = [(21, 19, 31), (10, 10, 45), (0, 0, 0), tuple(OBSTACLES[0])]          # pocket, unknown above, rim, an obstacle
        L.box_seeds = np.concatenate([2 + rng.randint(0, 44, (12, 3)) * (1, 36 / 44, 48 / 44), special]).astype(np.int64) + s
        L.view_pos = np.array(VIEW_VOX) + (0.5, 0.4, 0.6) + s
        ang = np.arange(8) * (np.pi / 4) + 0.3
        L.view_dir = np.stack([np.cos(ang), np.sin(ang)], 1)
        L.sensor = dict(min_range=0.2, max_range=2.5, tan_h=1.0, tan_v=1.0, block_mask=3, min_visible=1)
        paths = [np.array([(8.3, 8.2, 10.4), (20.6, 15.1, 15.7), (30.2, 25.3, 22.9)]),
                 np.array([(21.5, 19.5, 25.2), (21.5, 19.5, 44.8)]),                    # through the pocket, into the unknown above
                 np.array([(40.2, 30.1, 8.3), (46.9, 38.8, 2.1)])]                      # out of the observed box
        L.path_w = np.concatenate(paths) + s
        L.path_off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
        L.scalar_vox = np.array(SCALAR_VOX, np.int64) + s
        L.batch_extra = (olo + rng.randint(0, 30, (8, 3))).astype(np.int64) + s
        L.matrix_sources = None
        return L

    @classmethod
    def shard(cls):
        """for shard A of tests/test_gpu_frontiers.py::test_shard_answers_for_its_own_array: owned x = 0 .. 15, ghost layer x = 16, 17"""
        L, rng = cls(), np.random.RandomState(4321)
        L.frontier_box = ((2, 2, 2), (17, 13, 13))
        S, E = [rng.rand(60, 3) * (20, 16, 16)], [rng.rand(60, 3) * (20, 16, 16)]
        a = 3 + rng.rand(30, 3) * (12, 9, 9)
        S.append(a), E.append(np.stack([16 + rng.rand(30) * 2.5, 3 + rng.rand(30) * 10, 3 + rng.rand(30) * 10], 1))     # into the ghost layer
        S.append(np.array([(5.5, 7.5, 7.5), (5.5, 4.5, 4.5)])), E.append(np.array([(17.5, 7.5, 7.5), (17.5, 4.5, 4.5)]))
        L.ray_start, L.ray_end = np.concatenate(S), np.concatenate(E)
        L.reach_seed, L.reach_box = np.array((8, 8, 8)), (np.array((2, 2, 2)), np.array((17, 13, 13)))
        L.box_seeds = np.concatenate([rng.randint(0, 16, (12, 3)) + (2, 0, 0), [(16, 7, 7), (17, 4, 4), (15, 12, 12), (0, 0, 0)]]).astype(np.int64)
        L.view_pos = np.array([(5, 5, 5), (8, 8, 8), (12, 6, 9), (14, 10, 10), (15, 7, 7), (6, 11, 4), (10, 4, 11), (13, 12, 6)]) + 0.5
        ang = np.arange(8) * (np.pi / 4) + 0.3
        L.view_dir = np.stack([np.cos(ang), np.sin(ang)], 1)
        L.sensor = dict(min_range=0.1, max_range=1.5, tan_h=1.0, tan_v=1.0, block_mask=3, min_visible=1)
        paths = [np.array([(4.3, 4.2, 4.4), (10.6, 8.1, 7.7), (17.6, 7.3, 7.2)]), np.array([(8.5, 8.5, 2.2), (8.5, 8.5, 14.8)]),
                 np.array([(14.2, 10.1, 8.3), (17.9, 4.4, 4.1)])]
        L.path_w = np.concatenate(paths)
        L.path_off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
        L.scalar_vox = np.array([(17, 7, 7), (16, 4, 4), (15, 7, 7), (8, 8, 8), (3, 3, 3), (16, 10, 12), (12, 12, 12), (17, 9, 6)], np.int64)
        L.batch_extra = rng.randint(2, 14, (8, 3)).astype(np.int64)
        L.matrix_sources = np.array([(8, 8, 8), (5, 5, 5), (16, 7, 7), (17, 8, 8), (1, 1, 1)], np.int64)
        return L


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
def occupy(m, vox, cycles=3):
    for _ in range(cycles):                               # (an obstacle needs three hits to count as occupied)
        m.SetOccupancy(np.ascontiguousarray(vox, np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)


def fill_scene(m, shift=(0, 0, 0), full=False):
    """the scene into an empty map: the box observed free without the pocket (full: every voxel of SHAPE), the obstacles, UpdateESDF"""
    s = np.asarray(shift, np.int32)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    if full:
        m.SetOccupancyBox(s, s + np.array(SHAPE, np.int32) - 1, 0)
    else:
        free = np.zeros(SHAPE, bool)
        free[tuple(slice(a, b + 1) for a, b in zip(OBS_LO, OBS_HI))] = True
        free[tuple(slice(a, b + 1) for a, b in zip(*POCKET))] = False
        m.SetOccupancy((np.argwhere(free) + s).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, OBSTACLES + s)
    m.UpdateESDF()
    return m


def dense_scene(engine=None, full=False):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, tuple((d - 0.5) * RES for d in SHAPE), update_engine=engine)
    assert tuple(m.grid_size) == SHAPE
    return fill_scene(m, full=full)


def hash_scene(shift=HASH_SHIFT):
    import fiesta_amd
    m = fiesta_amd.ESDFMap(HASH_ORIGIN, RES, reserve_size=100000, mode="hash")
    return fill_scene(m, shift)


def first_observations(m, shift=(0, 0, 0)):
    """the slab z = 41 .. 47 observed free, 20 inserts and 20 deletes -- up to, not including, UpdateESDF"""
    s = np.asarray(shift, np.int32)
    m.SetOccupancyBox(s + SLAB[0], s + SLAB[1], 0)
    delta(m, shift)


def delta(m, shift=(0, 0, 0), cycles=6):
    """20 inserts and 20 deletes without a new observation (3 hits / at most 4 misses change a voxel's state)"""
    s = np.asarray(shift, np.int32)
    for _ in range(cycles):
        m.SetOccupancy(INSERTS + s, 1, want_ret=False)
        m.SetOccupancy(DELETES + s, 0, want_ret=False)
        m.UpdateOccupancy(True)


# ---- what the map reports of itself ---------------------------------------------------------------------------------------------------
class Field:
    """obs / occ / dist over an array whose element (0, 0, 0) is map voxel `org`, from DenseModel / HashModel of the frontier and the
    ray query tests (a shard: the same reads over its local array)"""

    def __init__(self, m, kind):
        from fiesta_amd import frontier_model
        self.m, self.kind, self.bounded = m, kind, kind != "hash"
        if kind == "dense":
            fm, self.rays = t_frontiers.DenseModel(m), t_rays.DenseModel(m)
            self.obs, self.occ, self.dist, self.org = fm.obs, fm.occ, fm.dist, np.zeros(3, np.int64)
            self.frontier = fm
        elif kind == "hash":
            fm, self.rays = t_frontiers.HashModel(m), t_rays.HashModel(m)
            self.obs, self.occ, self.dist, self.org = fm.obs, fm.occ, fm.dist, np.asarray(fm.org, np.int64)
            self.frontier = fm
        else:
            info = m.shard_info()
            self.org, dims = np.array(info["local_origin"], np.int64), tuple(int(v) for v in info["local_dims"])
            self.rays = t_rays.DenseModel(m, origin_vox=self.org, dims=dims)
            self.obs, self.occ = self.rays.obs, self.rays.occ
            self.dist = m.GetDistance(all_voxels(dims) + self.org.astype(np.int32)).reshape(dims)
            self.frontier = lambda lo=None, hi=None, min_clearance=0.0: frontier_model(self.obs, self.occ, self.dist, lo, hi, min_clearance,
                                                                                       origin_vox=self.org)
        assert np.array_equal(self.obs, self.rays.obs) and np.array_equal(self.occ, self.rays.occ), "two dumps of one map differ"
        self.pos_range = m.pos_range if self.bounded else None
        self.kw = dict(dist=self.dist, origin_vox=tuple(int(v) for v in self.org), bounded=self.bounded)

    def covering(self, lo, hi):
        """(obs, occ, dist, lo) over an array that covers the box [lo, hi] -- reach_model clips its box to the arrays it is given, a
        hash-block map clips nothing: what no page holds is unknown (Model.hashed of tests/test_gpu_reach.py)"""
        if self.bounded:
            return self.obs, self.occ, self.dist, self.org
        lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        shape = tuple(int(v) for v in hi - lo + 1)
        obs, occ, dist = np.zeros(shape, bool), np.zeros(shape, bool), np.full(shape, 10000.0)
        a, b = np.maximum(lo, self.org), np.minimum(hi, self.org + np.array(self.obs.shape) - 1)
        if np.all(a <= b):
            dst = tuple(slice(int(p - q), int(r - q) + 1) for p, r, q in zip(a, b, lo))
            src = tuple(slice(int(p - q), int(r - q) + 1) for p, r, q in zip(a, b, self.org))
            obs[dst], occ[dst], dist[dst] = self.obs[src], self.occ[src], self.dist[src]
        return obs, occ, dist, lo


def descend(cost, box_lo, connectivity=26):
    """a voxel polyline out of a cost field: from the reached voxel of the highest cost (the first in array order) down to the
    seed, every fourth voxel of the descent and both ends"""
    from fiesta_amd import reach_moves
    reached = (cost >= 0) & (cost != np.iinfo(np.int32).max)
    if not reached.any():
        return np.zeros((0, 3), np.int64)
    at = np.argwhere(reached & (cost == cost[reached].max()))[0]
    chain = [at]
    while cost[tuple(at)] > 0:
        for dx, dy, dz, w in reach_moves(connectivity):
            nb = at + (dx, dy, dz)
            if np.all(nb >= 0) and np.all(nb < cost.shape) and cost[tuple(nb)] == cost[tuple(at)] - w:
                at = nb
                break
        else:
            raise AssertionError("the model's cost field is no fixed point")
        chain.append(at)
    chain = np.array(chain, np.int64)
    keep = np.unique(np.concatenate([np.arange(0, len(chain), 4), [len(chain) - 1]]))
    return chain[keep] + np.asarray(box_lo, np.int64)


# ---- device variants: buffers on `device` (a stand-in without a GPU answers from host pointers) -----------------------------------------
def _device_outputs(m, fields, n, device):
    import torch
    return {name: torch.full((n[per] if isinstance(n, dict) else n,) + tuple(shape), 77, dtype=getattr(torch, np.dtype(dt).name), device=device)
            for name, dt, per, shape in fields}


def _sync(device):
    import torch
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()      # (the map's stream does not wait for torch's: copies and fills must have landed)


def ray_query_device(m, start, end, mask, device):
    import torch
    from fiesta_amd.esdf_map import RAY_FIELDS
    s, e = torch.from_numpy(np.ascontiguousarray(start)).to(device), torch.from_numpy(np.ascontiguousarray(end)).to(device)
    out = _device_outputs(m, [(k, dt, None, sh) for k, dt, sh in RAY_FIELDS], len(start), device)
    _sync(device)
    m.RayQueryDevice(s.data_ptr(), e.data_ptr(), len(start), mask, {k: t.data_ptr() for k, t in out.items()})
    m.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def path_clearance_device(m, w, off, step, margin, device):
    import torch
    from fiesta_amd.esdf_map import PATH_FIELDS
    wt, ot = torch.from_numpy(np.ascontiguousarray(w)).to(device), torch.from_numpy(np.ascontiguousarray(off)).to(device)
    out = _device_outputs(m, [(k, dt, None, sh) for k, dt, sh in PATH_FIELDS], len(off) - 1, device)
    _sync(device)
    m.PathClearanceDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, step, margin, {k: t.data_ptr() for k, t in out.items()})
    m.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def path_cost_device(m, w, off, step, margin, device):
    import torch
    from fiesta_amd.esdf_map import PATH_COST_FIELDS
    wt, ot = torch.from_numpy(np.ascontiguousarray(w)).to(device), torch.from_numpy(np.ascontiguousarray(off)).to(device)
    out = _device_outputs(m, PATH_COST_FIELDS, {"path": len(off) - 1, "waypoint": len(w)}, device)
    _sync(device)
    m.PathCostDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, step, margin, {k: t.data_ptr() for k, t in out.items()})
    m.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


# ---- the probe ------------------------------------------------------------------------------------------------------------------------
PATH_STEP, PATH_MARGIN, COST_MARGIN = 0.05, 0.3, 0.8
REACH_KEYS = ("n_traversable", "n_reached")


def probe(m, kind, layout=None, what=""):
    """see the module's docstring; `layout`: a Layout (None: Layout.scene() or, kind "shard", Layout.shard()).  Returns the digest."""
    import fiesta_amd
    from fiesta_amd import corridor_model, free_box_model, ray_walks, reach_matrix_model, reach_model, view_coverage_model
    assert kind in ("dense", "shard", "hash")
    L = layout or (Layout.shard() if kind == "shard" else Layout.scene())
    device = getattr(m, "probe_device", "cuda:0")
    f = Field(m, kind)
    res, origin = m.resolution, np.asarray(m.origin, np.float64)
    tag = f"{what} [{kind}]".strip()
    metres = lambda v: origin + np.asarray(v, np.float64) * res   # noqa: E731
    i32 = lambda v: np.ascontiguousarray(v, np.int32)   # noqa: E731

    # frontiers: everything, and a box that cuts bitmap words, with a clearance
    whole = f.frontier()
    t_frontiers.assert_same(m.GetFrontierVoxels(), whole, f"{tag} GetFrontierVoxels()")
    lo, hi = L.frontier_box
    t_frontiers.assert_same(m.GetFrontierVoxels(i32(lo), i32(hi), 0.25), f.frontier(lo, hi, 0.25), f"{tag} GetFrontierVoxels(box, min_clearance 0.25)")
    frontier_rows = t_frontiers.rows(*whole)

    # rays: host and device variant
    start, end = metres(L.ray_start), metres(L.ray_end)
    walks = ray_walks(start, end, res)
    ray_class = {}
    for mask in (7, 1):
        want = f.rays(start, end, mask, walks)
        t_rays.assert_same(m.RayQuery(start, end, mask), want, f"{tag} RayQuery(stop_mask {mask})")
        t_rays.assert_same(ray_query_device(m, start, end, mask, device), want, f"{tag} RayQueryDevice(stop_mask {mask})")
        ray_class[mask] = want["hit_class"].copy()

    # reach: one seed, a box of at most 32^3 voxels, with and without the way through unknown space
    lo, hi = L.reach_box
    obs, occ, dist, org = f.covering(lo, hi)
    n_traversable, fields = [], {}
    for flags in (0, THROUGH):
        want = reach_model(obs, occ, L.reach_seed[None], dist, lo, hi, 0.0, 26, flags, None, org)
        got = m.ReachField(i32(L.reach_seed[None]), i32(lo), i32(hi), connectivity=26, flags=flags)
        assert got["cost"].shape == want["cost"].shape, f"{tag} ReachField(flags {flags}): cost {got['cost'].shape}, the model has {want['cost'].shape}"
        bad = np.argwhere(got["cost"] != want["cost"])
        assert len(bad) == 0, f"{tag} ReachField(flags {flags}): {len(bad)} costs differ, first at {(bad[:3] + want['box_lo']).tolist()}"
        for k in REACH_KEYS:
            assert got[k] == want[k], f"{tag} ReachField(flags {flags}): {k} {got[k]}, the model has {want[k]}"
        n_traversable.append(want["n_traversable"])
        fields[flags] = want
    if L.matrix_sources is not None:
        want = reach_matrix_model(obs, occ, L.matrix_sources, None, dist, lo, hi, 0.0, 26, 0, org)
        got = m.ReachMatrix(i32(L.matrix_sources), None, i32(lo), i32(hi))
        for k in ("cost", "source_status", "source_reached"):
            assert np.array_equal(got[k], want[k]), f"{tag} ReachMatrix: {k} differs: got {got[k].tolist()} want {want[k].tolist()}"
        for k in ("n_traversable", "n_sources_used", "box_lo", "box_hi"):
            assert got[k] == want[k], f"{tag} ReachMatrix: {k} {got[k]}, the model has {want[k]}"

    # free boxes and a corridor along a polyline out of the MODEL's cost field
    kw = dict(f.kw, resolution=res, origin=tuple(origin))
    want = free_box_model(f.obs, f.occ, L.box_seeds, max_grow=16, **kw)
    t_corridor.assert_same(m.FreeBoxes(i32(L.box_seeds), None, None, 16), want, t_corridor.BOX_KEYS, f"{tag} FreeBoxes")
    line = descend(fields[0]["cost"], fields[0]["box_lo"])
    if len(line) < 2:
        line = np.stack([L.reach_seed, L.reach_seed + (3, 2, 1)])
    off = np.array([0, len(line)], np.int64)
    want = corridor_model(f.obs, f.occ, line, off, lo=lo, hi=hi, max_grow=8, **kw)
    t_corridor.assert_same(m.PathCorridor(i32(line), off, i32(lo), i32(hi), 8), want, t_corridor.KEYS, f"{tag} PathCorridor")

    # view coverage: 8 explicit views against about 100 voxels of the model's frontier set
    targets = frontier_rows[::max(1, len(frontier_rows) // 100), :3] if len(frontier_rows) >= 8 else L.box_seeds
    pos = metres(L.view_pos)
    want = view_coverage_model(f.obs, f.occ, origin, res, targets, pos=pos, dir=L.view_dir, pos_range=f.pos_range, **L.sensor, **f.kw)
    t_views.assert_same(m.ViewCoverage(i32(targets), pos=pos, dir=L.view_dir, **L.sensor), want, f"{tag} ViewCoverage")

    # path clearance and cost: at most 256 samples, so the host variant answers from the brick cache; the device variant never does
    w, off = metres(L.path_w), L.path_off
    n_samples = fiesta_amd.path_samples(w, off, PATH_STEP)[1]
    assert 8 < n_samples.sum() <= 256 and (n_samples > 0).all(), n_samples
    want = t_path.model(m, w, off, PATH_STEP, PATH_MARGIN)
    host = m.PathClearance(w, off, PATH_STEP, PATH_MARGIN)
    t_path.assert_same(host, want, f"{tag} PathClearance (host route: the brick cache)")
    dev = path_clearance_device(m, w, off, PATH_STEP, PATH_MARGIN, device)
    t_path.assert_same(dev, want, f"{tag} PathClearanceDevice")
    t_path.assert_same(dev, host, f"{tag} PathClearanceDevice against PathClearance")
    want = t_path_cost.model_of(m, w, off, PATH_STEP, COST_MARGIN)
    t_path_cost.assert_within(m.PathCost(w, off, PATH_STEP, COST_MARGIN), want, f"{tag} PathCost (host route: the brick cache)")
    t_path_cost.assert_within(path_cost_device(m, w, off, PATH_STEP, COST_MARGIN, device), want, f"{tag} PathCostDevice")

    # scalar queries, one voxel per call (the brick cache), against the same voxels in one batch of 16 (the device route)
    batch = i32(np.concatenate([L.scalar_vox, L.batch_extra]))
    dist_b, occ_b = m.GetDistance(batch), m.GetOccupancy(batch)
    for i, v in enumerate(i32(L.scalar_vox)):
        d, o = m.GetDistance(v), m.GetOccupancy(v)
        assert np.float64(d).view(np.int64) == dist_b[i].view(np.int64), f"{tag} GetDistance({v.tolist()}) alone: {d!r}, in a batch of 16: {dist_b[i]!r}"
        assert o == occ_b[i], f"{tag} GetOccupancy({v.tolist()}) alone: {o}, in a batch of 16: {occ_b[i]}"
    return {"frontier": frontier_rows, "ray_class": np.concatenate([ray_class[7], ray_class[1]]), "n_traversable": tuple(n_traversable),
            "scalar": dist_b[:8].copy()}


DIGEST_KEYS = ("frontier", "ray_class", "n_traversable", "scalar")


def differs(d0, d1, key):
    a, b = d0[key], d1[key]
    return a != b if isinstance(a, tuple) else a.shape != b.shape or bool((a != b).any())


def assert_differs(d0, d1, keys, what=""):
    """the transition changed what it is about: a case that leaves the digest alone tests nothing"""
    for k in keys:
        assert differs(d0, d1, k), f"{what}: the transition left '{k}' unchanged: the case is vacuous"


def assert_equal(d0, d1, what=""):
    for k in DIGEST_KEYS:
        assert not differs(d0, d1, k), f"{what}: '{k}' differs from the first probe's"
