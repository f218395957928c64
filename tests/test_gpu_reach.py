"""Reachability on the GPU (fiesta_hip_reach_field[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/reach_kernels.hpp).

The expected field is always fiesta_amd.reach_model (the header's definition: numpy traversability and a heap Dijkstra;
tests/test_reach_rule.py checks it against a plain Bellman-Ford loop) fed from what the map itself reports through calls that existed
before: download_field (d2 >= 0, occ) or download_hash, and GetDistance of every voxel -- never from the call under test.  Costs are
integers and the fixed point is unique: every comparison is exact equality of whole fields, no tolerance, no excluded voxel.

The map is 48 x 40 x 72 voxels at 0.1 m: z is no multiple of 32, and the reach tiles (16 x 16 x 32) form a 3 x 3 x 3 grid.
"""
import ctypes as C

import numpy as np
import pytest

from scenarios import P_DEFAULT, all_voxels

pytestmark = pytest.mark.gpu
RES = 0.1
SHAPE = (48, 40, 72)
INF = 2 ** 31 - 1
THROUGH = 1
BOX = ((3, 2, 5), (44, 37, 66))     # unaligned z origin, a last word that is not full, faces that cut both turns of a corridor


def new_dense(shape=SHAPE):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, tuple((s - 0.5) * RES for s in shape))
    assert m.grid_size == tuple(shape)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    return m


def occupy(m, vox, esdf=True):
    S = np.ascontiguousarray(vox, np.int32).reshape(-1, 3)
    for _ in range(3):                                  # (an obstacle needs three hits to count as occupied)
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    if esdf:
        m.UpdateESDF()


def maze_walls(shape=SHAPE):
    """walls across x at every 6th x-plane, full height, with a gap 3 voxels wide that alternates between y = low and y = high"""
    occ = np.zeros(shape, bool)
    for k, x in enumerate(range(6, shape[0], 6)):
        occ[x] = True
        if k % 2 == 0:
            occ[x, :3] = False
        else:
            occ[x, shape[1] - 3:] = False
    return occ


class Model:
    """reach_model on the map's own dump, read once; results are kept (the tests share them and leave them unchanged)"""

    def __init__(self, obs, occ, dist, origin=(0, 0, 0)):
        self.obs, self.occ, self.dist, self.origin, self.memo = obs, occ, dist, tuple(int(v) for v in origin), {}

    @classmethod
    def dense(cls, m, origin=(0, 0, 0), with_dist=True):
        f = m.download_field(("d2", "occ"))
        dims = m.grid_size
        dist = m.GetDistance(all_voxels(dims) + np.asarray(origin, np.int32)).reshape(dims) if with_dist else None
        return cls((f["d2"] >= 0).reshape(dims), f["occ"].reshape(dims) != 0, dist, origin)

    @classmethod
    def hashed(cls, m, lo, hi):
        """download_hash scattered into an array that covers the box [lo, hi]: what no page holds is unknown"""
        h = m.download_hash()
        lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        shape = tuple(int(v) for v in hi - lo + 1)
        keep = np.all((h["vox"] >= lo) & (h["vox"] <= hi), axis=1)
        i = tuple((h["vox"][keep] - lo).T)
        obs, occ, dist = np.zeros(shape, bool), np.zeros(shape, bool), np.full(shape, 10000.0)
        obs[i] = h["d2"][keep] >= 0
        occ[i] = h["occ"][keep] != 0
        dist[i] = m.GetDistance(h["vox"][keep])
        return cls(obs, occ, dist, lo)

    def __call__(self, seeds, lo=None, hi=None, clearance=0.0, conn=26, flags=0, targets=None):
        from fiesta_amd import reach_model
        key = (np.asarray(seeds).tobytes(), None if lo is None else tuple(lo), None if hi is None else tuple(hi), clearance, conn, flags,
               None if targets is None else np.asarray(targets).tobytes())
        if key not in self.memo:
            self.memo[key] = reach_model(self.obs, self.occ, seeds, self.dist, lo, hi, clearance, conn, flags, targets, self.origin)
        return self.memo[key]


INFO_KEYS = ("box_lo", "box_hi", "n_traversable", "n_seeds_used", "n_reached", "max_cost")


def assert_same(got, want, what=""):
    """the whole cost field, the target costs and every info field the model defines"""
    if got.get("cost") is not None:
        assert got["cost"].dtype == np.int32 and got["cost"].shape == want["cost"].shape, (what, got["cost"].shape, want["cost"].shape)
        bad = np.argwhere(got["cost"] != want["cost"])
        assert len(bad) == 0, f"{what}: {len(bad)} costs differ, first at {bad[:3].tolist()} got " \
                              f"{[int(got['cost'][tuple(b)]) for b in bad[:3]]} want {[int(want['cost'][tuple(b)]) for b in bad[:3]]}"
    if "target_cost" in want:
        assert np.array_equal(got["target_cost"], want["target_cost"]), (what, got["target_cost"][:8], want["target_cost"][:8])
    for k in INFO_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.fixture(scope="module")
def maze(hip_lib):
    m = new_dense()
    m.SetOccupancyBox((0, 0, 0), tuple(s - 1 for s in SHAPE), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    walls = maze_walls()
    occupy(m, np.argwhere(walls))
    model = Model.dense(m)
    assert model.obs.all() and np.array_equal(model.occ, walls)
    yield m, model
    m.close()


SEED = [(4, 20, 36)]


@pytest.mark.parametrize("conn", [6, 26])
def test_serpentine_maze(maze, conn):
    m, model = maze
    want = model(SEED, conn=conn)
    far = want["cost"][47, 20, 36]
    assert want["n_reached"] == want["n_traversable"] == int((~model.occ).sum())
    assert 3 * 46 * 3 < far <= want["max_cost"]                                   # the way through seven walls is much longer than the straight line
    got = m.ReachField(SEED, connectivity=conn)
    print(f"maze, connectivity {conn}: {got['rounds']} rounds, {got['tile_visits']} tile visits, max cost {got['max_cost']}")
    assert_same(got, want, f"maze {conn}")
    # the path re-enters the same tiles again and again: more rounds than tiles along x proves the wake-up path at work
    assert got["rounds"] > 3 and got["tile_visits"] > 27


@pytest.mark.parametrize("conn", [6, 26])
def test_maze_in_a_box(maze, conn):
    m, model = maze
    lo, hi = BOX
    want = model(SEED, lo, hi, conn=conn)
    assert want["cost"].shape == (42, 36, 62) and want["box_lo"] == list(lo) and want["box_hi"] == list(hi)
    # the gaps lie at y < 3 and y > 36: the box keeps one row of the low gaps (y = 2) and one of the high ones (y = 37), so the routes
    # get no shorter; a box without the high row cuts every second gap and the cut route is no route
    whole = model(SEED, conn=conn)
    assert want["n_reached"] == want["n_traversable"] and want["max_cost"] >= whole["cost"][3:45, 2:38, 5:67].max()
    assert_same(m.ReachField(SEED, lo, hi, connectivity=conn), want, f"boxed maze {conn}")
    hi2 = (44, 36, 66)
    cut = model(SEED, lo, hi2, conn=conn)
    assert cut["cost"][44 - 3, 20 - 2, 30] == INF and 0 < cut["n_reached"] < cut["n_traversable"]
    assert_same(m.ReachField(SEED, lo, hi2, connectivity=conn), cut, f"cut maze {conn}")


def test_boxes_clip_and_may_be_empty(maze):
    m, model = maze
    for lo, hi in (((-5, -5, -5), (100, 100, 100)), ((0, 0, 0), (47, 39, 71)), ((-3, 10, 31), (20, 50, 32)), ((0, 0, 64), (11, 39, 71)),
                   ((4, 20, 36), (4, 20, 36)), ((-2 ** 31, -2 ** 31, -2 ** 31), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))):
        want = model(SEED, lo, hi, targets=[(1, 20, 36), (5, 39, 70)])
        assert_same(m.ReachField(SEED, lo, hi, targets=[(1, 20, 36), (5, 39, 70)]), want, f"box {lo} {hi}")
    for lo, hi in (((100, 100, 100), (200, 200, 200)), ((5, 5, 5), (4, 9, 9)), ((5, 5, 5), (9, 9, 4)), ((0, 0, 72), (47, 39, 80))):
        got = m.ReachField(SEED, lo, hi, targets=[(1, 20, 36), (5, 5, 5)])
        assert got["cost"].size == 0 and got["target_cost"].tolist() == [-1, -1]
        assert all(got[k] == 0 for k in ("n_traversable", "n_seeds_used", "n_reached", "max_cost", "rounds", "tile_visits"))
        assert got["box_lo"] == [0, 0, 0] and got["box_hi"] == [0, 0, 0]
        assert_same(got, model(SEED, lo, hi, targets=[(1, 20, 36), (5, 5, 5)]), f"empty box {lo} {hi}")


def build_partial(esdf=True):
    """a free box with unobserved blocks -- a slab across x = 10 .. 13 that separates the low end from the rest, a block in a far
    corner -- and a wall at x = 30 whose only door is two voxels wide (y = 18, 19; z = 6 .. 40)"""
    m = new_dense()
    obs = np.ones(SHAPE, bool)
    obs[10:14] = False
    obs[40:, 30:, 50:] = False
    wall = np.zeros(SHAPE, bool)
    wall[30] = True
    wall[30, 18:20, 6:41] = False
    m.SetOccupancy(np.argwhere(obs & ~wall).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    if esdf:
        m.UpdateESDF()
    occupy(m, np.argwhere(wall), esdf=esdf)
    return m, obs, wall


@pytest.fixture(scope="module")
def partial(hip_lib):
    m, obs, wall = build_partial()
    model = Model.dense(m)
    assert np.array_equal(model.obs, obs) and np.array_equal(model.occ, wall)
    yield m, model
    m.close()


def test_unknown_space_blocks_unless_asked_to_pass(partial):
    m, model = partial
    seeds = [(2, 5, 5)]
    shut = model(seeds)
    assert shut["cost"][9, 5, 5] == 21 and shut["cost"][12, 5, 5] == -1 and shut["cost"][20, 5, 5] == INF
    assert_same(m.ReachField(seeds), shut, "default flags")
    thru = model(seeds, flags=THROUGH)
    assert thru["cost"][12, 5, 5] == 30 and thru["cost"][20, 5, 5] == 54 and thru["cost"][45, 35, 60] < INF and thru["cost"][30, 0, 0] == -1
    assert thru["n_traversable"] == int((~model.occ).sum()) == thru["n_reached"]
    assert_same(m.ReachField(seeds, flags=THROUGH), thru, "through unknown")
    assert_same(m.ReachField(seeds, flags=THROUGH, connectivity=6), model(seeds, flags=THROUGH, conn=6), "through unknown, 6")


def test_clearance_closes_the_narrow_door(partial):
    m, model = partial
    seeds = [(20, 19, 20)]
    assert model.dist[30, 17, 20] == 0.0 and model.dist[30, 18, 20] == RES and model.dist[20, 25, 20] == 10 * RES
    wide = model(seeds)
    assert wide["cost"][40, 19, 20] == 60 and wide["cost"][5, 5, 5] == INF
    assert_same(m.ReachField(seeds), wide, "clearance 0")
    for c in (0.0, -0.0, -1.0, -np.inf):
        assert_same(m.ReachField(seeds, min_clearance=c), wide, f"clearance {c}: no filter")
    shut = model(seeds, clearance=0.25)
    # both door voxels are one voxel from the wall: the far room is traversable (away from the walls) and not reached
    assert shut["cost"][30, 18, 20] == -1 and shut["cost"][30, 19, 20] == -1 and shut["cost"][40, 19, 20] == INF
    assert shut["cost"][31, 19, 20] == -1 and shut["cost"][25, 19, 20] == 15 and 0 < shut["n_reached"] < shut["n_traversable"]
    assert_same(m.ReachField(seeds, min_clearance=0.25), shut, "clearance 0.25")
    # the clearance is for observed voxels only; unknown ones pass untested
    both = model(seeds, clearance=0.25, flags=THROUGH)
    assert both["cost"][12, 5, 5] > 0 and both["cost"][5, 5, 5] < INF and both["cost"][40, 19, 20] == INF
    assert_same(m.ReachField(seeds, min_clearance=0.25, flags=THROUGH), both, "clearance 0.25 through unknown")
    for c in (0.1, 9999.0, 10001.0, np.inf):
        assert_same(m.ReachField(seeds, min_clearance=c, connectivity=6), model(seeds, clearance=c, conn=6), f"clearance {c}")
    assert model(seeds, clearance=10001.0, conn=6)["n_traversable"] == 0


def test_clearance_off_does_not_read_the_field(hip_lib):
    """no UpdateESDF has ever run on this map: the occupancy alone decides, and the answer is that of the updated map"""
    m, obs, wall = build_partial(esdf=False)
    model = Model.dense(m, with_dist=False)
    assert np.array_equal(model.obs, obs) and np.array_equal(model.occ, wall)
    seeds = [(20, 19, 20)]
    want = model(seeds)
    assert want["cost"][40, 19, 20] == 60 and want["n_reached"] > 90000
    assert_same(m.ReachField(seeds), want, "before any UpdateESDF")
    assert_same(m.ReachField(seeds, min_clearance=-2.0, connectivity=6), model(seeds, clearance=-2.0, conn=6), "before any UpdateESDF, 6")
    m.close()


def test_seeds(maze, partial):
    m, model = maze
    several = [(4, 20, 36), (46, 2, 70), (25, 39, 0), (4, 20, 36)]          # (one of them twice: it counts twice)
    want = model(several)
    assert want["n_seeds_used"] == 4 and want["max_cost"] < model(SEED)["max_cost"]
    assert_same(m.ReachField(several), want, "several seeds")
    mixed = [(6, 20, 36), (4, 20, 36), (48, 0, 0), (-1, 5, 5), (3, 2, 4), (2, 1, 5)]   # on a wall; good; outside the map; ... the box
    for lo, hi in ((None, None), BOX):
        want = model(mixed, lo, hi)
        assert want["n_seeds_used"] == (3 if lo is None else 1)
        assert_same(m.ReachField(mixed, lo, hi), want, f"mixed seeds {lo}")
    for seeds in ([(6, 20, 36), (100, 0, 0)], np.zeros((0, 3), np.int32)):
        want = model(seeds)
        assert want["n_seeds_used"] == 0 and want["n_reached"] == 0 and want["max_cost"] == 0 and (want["cost"][~model.occ] == INF).all()
        got = m.ReachField(seeds, targets=[(1, 1, 1), (6, 20, 36)])
        assert_same(got, want, "no usable seed")
        assert got["target_cost"].tolist() == [INF, -1] and got["tile_visits"] == 0
    pm, pmodel = partial
    unknown_seed = [(12, 5, 5), (2, 5, 5)]
    assert pmodel(unknown_seed)["n_seeds_used"] == 1 and pmodel(unknown_seed, flags=THROUGH)["n_seeds_used"] == 2
    assert_same(pm.ReachField(unknown_seed), pmodel(unknown_seed), "a seed in unknown space")


def test_targets_and_frontier_voxels_on_the_device(partial):
    import torch
    m, model = partial
    seeds = [(20, 19, 20)]
    targets = np.array([(40, 19, 20), (20, 19, 20), (30, 0, 0), (12, 5, 5), (5, 5, 5), (48, 0, 0), (-1, -1, -1), (3, 2, 66), (3, 2, 67),
                        (45, 35, 60)], np.int32)
    want = model(seeds, targets=targets)
    assert want["target_cost"].tolist()[:7] == [60, 0, -1, -1, INF, -1, -1]
    assert_same(m.ReachField(seeds, targets=targets), want, "targets")
    lo, hi = BOX
    boxed = model(seeds, lo, hi, targets=targets)
    assert boxed["target_cost"][7] >= 0 and boxed["target_cost"][8] == -1        # the last plane of the box, the first beyond it
    assert_same(m.ReachField(seeds, lo, hi, targets=targets), boxed, "targets, boxed")
    # the frontier call's device output straight into the reach call
    dev = torch.device("cuda", 0)
    fv, _ = m.GetFrontierVoxels()
    n = len(fv)
    assert n > 1000
    vox = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    tc = torch.full((n + 4,), -99, dtype=torch.int32, device=dev)
    sd = torch.tensor(seeds, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.GetFrontierVoxelsDevice(None, None, 0.0, vox.data_ptr(), 0, n, count.data_ptr())
    info = m.ReachFieldDevice(sd.data_ptr(), 1, targets_dev_ptr=vox.data_ptr(), n_targets=n, target_cost_dev_ptr=tc.data_ptr())
    assert int(count.item()) == n
    v, t = vox.cpu().numpy(), tc.cpu().numpy()
    field = model(seeds)["cost"]
    assert np.array_equal(t[:n], field[v[:, 0], v[:, 1], v[:, 2]]) and (t[n:] == -99).all()
    assert (t[:n] >= 0).all() and (t[:n] == INF).any() and (t[:n] < INF).any()   # frontier voxels are free; some are out of reach
    assert all(info[k] == model(seeds)[k] for k in INFO_KEYS)


def test_equal_results(maze):
    import torch
    m, model = maze
    lo, hi = BOX
    targets = np.array([(44, 37, 66), (1, 20, 36), (47, 0, 0), (6, 20, 36)], np.int32)
    want = model(SEED, lo, hi, targets=targets)
    full = m.ReachField(SEED, lo, hi, targets=targets)
    assert_same(full, want, "cost and targets")
    only = m.ReachField(SEED, lo, hi, targets=targets, want_cost=False)          # cost NULL: the map's own scratch field
    assert only["cost"] is None
    assert_same(only, want, "targets only")
    again = m.ReachField(SEED, lo, hi, targets=targets)
    assert np.array_equal(again["cost"], full["cost"]) and np.array_equal(again["target_cost"], full["target_cost"])
    assert all(again[k] == full[k] for k in INFO_KEYS)
    none = m.ReachField(SEED, lo, hi, want_cost=False)                            # no output at all: the info alone
    assert all(none[k] == want[k] for k in INFO_KEYS)
    # the device variant
    dev = torch.device("cuda", 0)
    nvox = int(np.prod(want["cost"].shape))
    cost = torch.full((nvox + 8,), -99, dtype=torch.int32, device=dev)
    tc = torch.full((len(targets) + 4,), -99, dtype=torch.int32, device=dev)
    sd, td = torch.tensor(SEED, dtype=torch.int32, device=dev), torch.tensor(targets, device=dev)
    torch.cuda.synchronize()
    info = m.ReachFieldDevice(sd.data_ptr(), 1, lo, hi, td.data_ptr(), len(targets), cost_dev_ptr=cost.data_ptr(), target_cost_dev_ptr=tc.data_ptr())
    c, t = cost.cpu().numpy(), tc.cpu().numpy()                                  # (the call has synchronised with the map's stream)
    assert np.array_equal(c[:nvox].reshape(want["cost"].shape), full["cost"]) and (c[nvox:] == -99).all()
    assert np.array_equal(t[:4], full["target_cost"]) and (t[4:] == -99).all()
    assert all(info[k] == full[k] for k in INFO_KEYS) and info["rounds"] == full["rounds"] > 0
    tc.fill_(-99)
    torch.cuda.synchronize()
    info = m.ReachFieldDevice(sd.data_ptr(), 1, lo, hi, td.data_ptr(), len(targets), target_cost_dev_ptr=tc.data_ptr())
    assert np.array_equal(tc.cpu().numpy()[:4], full["target_cost"]) and all(info[k] == full[k] for k in INFO_KEYS)
    info = m.ReachFieldDevice(sd.data_ptr(), 1, (5, 5, 5), (4, 9, 9), td.data_ptr(), len(targets), target_cost_dev_ptr=tc.data_ptr())
    assert tc.cpu().numpy().tolist() == [-1] * 4 + [-99] * 4 and info["n_traversable"] == 0 and info["box_hi"] == [0, 0, 0]


def test_info_fields(maze, partial):
    m, model = maze
    got = m.ReachField(SEED, connectivity=6, want_cost=False)
    want = model(SEED, conn=6)
    assert got["box_lo"] == [0, 0, 0] and got["box_hi"] == [47, 39, 71]
    assert got["n_traversable"] == want["n_traversable"] == 48 * 40 * 72 - 7 * 37 * 72
    assert got["n_reached"] == want["n_reached"] == got["n_traversable"] and got["n_seeds_used"] == 1
    assert got["max_cost"] == want["max_cost"] == int(want["cost"].max())
    assert got["rounds"] <= got["tile_visits"] <= got["rounds"] * 27
    pm, pmodel = partial
    got = pm.ReachField([(2, 5, 5)], want_cost=False)
    want = pmodel([(2, 5, 5)])
    assert all(got[k] == want[k] for k in INFO_KEYS) and got["n_reached"] == 10 * 40 * 72 < got["n_traversable"]


def test_the_map_is_untouched(partial):
    m, model = partial
    before = m.download_field()
    hit0, miss0 = m.download_counts()
    for kw in (dict(), dict(min_clearance=0.25), dict(flags=THROUGH, connectivity=6), dict(lo=BOX[0], hi=BOX[1], targets=[(20, 19, 20)])):
        m.ReachField([(20, 19, 20)], **kw)
    after = m.download_field()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    hit1, miss1 = m.download_counts()
    assert np.array_equal(hit0, hit1) and np.array_equal(miss0, miss1)
    assert not m.CheckUpdate()


HASH_SHIFT = np.array((-20, 8, -40), np.int64)      # the maze straddles tile faces and negative coordinates


@pytest.fixture(scope="module")
def hash_maze(hip_lib):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=200000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    walls = maze_walls()
    V = all_voxels(SHAPE).astype(np.int64) + HASH_SHIFT
    m.SetOccupancy(V.astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, np.argwhere(walls) + HASH_SHIFT)
    yield m
    m.close()


def test_hash_block_map(hash_maze):
    m = hash_maze
    s = HASH_SHIFT
    seed = [tuple(int(v) for v in s + (1, 20, 36))]
    targets = np.array([s + (47, 20, 36), s + (6, 20, 36), s + (-5, 0, 0), s + (100, 0, 0)], np.int32)
    # the maze's own box; a box around it that straddles tiles without a page; a box that cuts it, unaligned in z
    boxes = [(s, s + np.array(SHAPE) - 1), (s - 20, s + np.array(SHAPE) + 19), (s + BOX[0], s + BOX[1])]
    wide = Model.hashed(m, s - 24, s + np.array(SHAPE) + 23)
    assert wide.obs.sum() == np.prod(SHAPE) and wide.occ.sum() == 7 * 37 * 72
    results = []
    for lo, hi in boxes:
        for flags, conn, clr in ((0, 26, 0.0), (THROUGH, 26, 0.0), (0, 6, 0.25), (THROUGH, 6, 0.0)):
            want = wide(seed, lo, hi, clr, conn, flags, targets)
            got = m.ReachField(seed, lo, hi, targets, clr, conn, flags)
            assert_same(got, want, f"hash box {lo} {hi} flags {flags} conn {conn} clearance {clr}")
            results.append((lo, hi, clr, conn, flags, got))
    # around the maze the unknown space is a short cut past the walls, when asked for
    plain, thru = results[4][5], results[5][5]
    assert plain["target_cost"][0] > 2 * thru["target_cost"][0] > 0 and thru["target_cost"][2] > 0 and plain["target_cost"][2] == -1
    assert thru["n_traversable"] == 88 * 80 * 112 - 7 * 37 * 72 == thru["n_reached"]
    # every page parked (the window far away): the pages answer as before
    pages = m.grid_total_size_
    m.hash_recentre(s + np.array([3000, -3000, 3000]))
    assert m.grid_total_size_ == pages
    for lo, hi, clr, conn, flags, before in results[4:]:
        got = m.ReachField(seed, lo, hi, targets, clr, conn, flags)
        assert np.array_equal(got["cost"], before["cost"]) and np.array_equal(got["target_cost"], before["target_cost"])
        assert all(got[k] == before[k] for k in INFO_KEYS)
    # ... and a window that covers half of the maze: resident and parked pages in one box
    m.hash_recentre(s + np.array([24 + 512, 20, 36]))
    org, _ = m.hash_window()
    assert s[0] < org[0] < s[0] + 47
    lo, hi, clr, conn, flags, before = results[5]
    got = m.ReachField(seed, lo, hi, targets, clr, conn, flags)
    assert np.array_equal(got["cost"], before["cost"]) and all(got[k] == before[k] for k in INFO_KEYS)
    # a hash-block map has no outside: the box is mandatory, and bounded
    res = _result()
    assert raw_call(m, None, None, seed, res=res) == 1
    assert raw_call(m, (0, 0, 0), (1023, 1023, 256), seed, res=res) == 1 and raw_call(m, (-2 ** 31,) * 3, (2 ** 31 - 1,) * 3, seed, res=res) == 1
    assert_same(m.ReachField(seed, *boxes[0], targets=targets), wide(seed, *boxes[0], targets=targets), "after the errors")
    far = m.ReachField([(2 ** 30, 0, 0)], (2 ** 30 - 3, -1, -1), (2 ** 31 - 1, 1, 1), flags=THROUGH)   # clamped to 2^30: all unknown
    assert far["cost"].shape == (4, 3, 3) and far["n_reached"] == 36 and far["box_hi"] == [2 ** 30, 1, 1]


def test_shard_answers_for_its_own_array(hip_lib):
    """a shard (owned box + ghost layers): the box is its local array, reported in global voxel coordinates"""
    import fiesta_amd
    gg = (32, 16, 16)
    shards = [fiesta_amd.ESDFMap((0, 0, 0), RES, (15.5 * RES,) * 3, shard_lo=lo, global_grid=gg) for lo in ((0, 0, 0), (16, 0, 0))]
    for sh in shards:
        sh.SetParameters(*P_DEFAULT)
        sh.SetOriginalRange()
    a, b = shards
    a.SetOccupancyBox((3, 3, 3), (15, 12, 12), 0)
    b.SetOccupancyBox((16, 5, 5), (20, 10, 14), 0)
    for sh in shards:
        sh.UpdateOccupancy(True)
        sh.UpdateESDF()
    ia, ib = a.shard_info(), b.shard_info()
    oa, ob, da = np.array(ia["local_origin"]), np.array(ib["local_origin"]), np.array(ia["local_dims"])
    glo, ghi = np.array([16, 0, 0]), oa + da - 1
    assert a.halo_apply(glo - oa, ghi - oa, b.halo_pack(glo - ob, ghi - ob)) > 0
    for sh, org in ((a, oa), (b, ob)):
        model = Model.dense(sh, org)
        seeds = [(15, 7, 7), (17, 7, 7)]
        for kw, mk in ((dict(), dict()), (dict(lo=(10, 0, 0), hi=(40, 9, 9), flags=THROUGH), dict(lo=(10, 0, 0), hi=(40, 9, 9), flags=THROUGH))):
            want = model(seeds, targets=[(16, 7, 7), (3, 3, 3)], **mk)
            assert want["n_seeds_used"] >= 1 and want["n_reached"] > 0
            assert_same(sh.ReachField(seeds, targets=[(16, 7, 7), (3, 3, 3)], **kw), want, f"shard at {org}")
    assert Model.dense(a, oa)([(15, 7, 7)])["cost"][16 - oa[0], 7, 7] == 3          # into the ghost layer the exchange filled
    for sh in shards:
        sh.close()


def _result(cost=None, target_cost=None):
    from fiesta_amd._lib import ReachResult
    return ReachResult(None if cost is None else cost.ctypes.data, None if target_cost is None else target_cost.ctypes.data)


def raw_call(m, lo, hi, seeds, n_seeds=None, targets=None, n_targets=None, clearance=0.0, conn=26, flags=0, res=None, info=None, dev=False):
    """the C call itself; returns the status"""
    from fiesta_amd.esdf_map import _p
    blo = None if lo is None else np.ascontiguousarray(lo, np.int32)
    bhi = None if hi is None else np.ascontiguousarray(hi, np.int32)
    s = None if seeds is None else np.ascontiguousarray(seeds, np.int32).reshape(-1, 3)
    t = None if targets is None else np.ascontiguousarray(targets, np.int32).reshape(-1, 3)
    fn = m._lib.fiesta_hip_reach_field_dev if dev else m._lib.fiesta_hip_reach_field
    return fn(m._h, _p(blo), _p(bhi), _p(s), (0 if s is None else len(s)) if n_seeds is None else n_seeds, _p(t),
              (0 if t is None else len(t)) if n_targets is None else n_targets, float(clearance), int(conn), int(flags),
              None if res is None else C.byref(res), None if info is None else C.byref(info))


def test_errors_leave_the_map_usable(maze):
    import fiesta_amd
    from fiesta_amd._lib import ReachInfo
    m, model = maze
    cost = np.full(SHAPE, -77, np.int32)
    tc = np.full(2, -77, np.int32)
    res, info = _result(cost, tc), ReachInfo()
    info.n_reached = -5
    tg = [(1, 1, 1), (2, 2, 2)]
    for dev in (False, True):
        bad = [raw_call(m, None, None, SEED, targets=tg, clearance=np.nan, res=res, info=info, dev=dev),
               raw_call(m, (0, 0, 0), None, SEED, targets=tg, res=res, info=info, dev=dev),
               raw_call(m, None, (5, 5, 5), SEED, targets=tg, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, targets=tg, conn=18, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, targets=tg, conn=0, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, targets=tg, flags=2, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, targets=tg, flags=-2, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, n_seeds=-1, targets=tg, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, targets=tg, n_targets=-1, res=res, info=info, dev=dev),
               raw_call(m, None, None, None, n_seeds=1, targets=tg, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, targets=None, n_targets=2, res=res, info=info, dev=dev),
               raw_call(m, None, None, SEED, targets=None, res=res, info=info, dev=dev),          # target_cost without targets
               raw_call(m, None, None, SEED, targets=tg, res=None, info=info, dev=dev)]
        assert bad == [1] * len(bad), bad                      # FIESTA_HIP_ERR_INVALID
        assert "result" in fiesta_amd._lib.last_error()
    assert (cost == -77).all() and (tc == -77).all() and info.n_reached == -5   # nothing launched, nothing written
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.ReachField(SEED, min_clearance=float("nan"))
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.ReachField(SEED, connectivity=18)
    with pytest.raises(ValueError):
        m.ReachField(SEED, lo=(0, 0, 0))
    # every pointer of the result may be null, and so may the info
    assert raw_call(m, None, None, SEED, res=_result()) == 0
    assert raw_call(m, None, None, SEED, targets=tg, res=_result()) == 0
    assert raw_call(m, None, None, SEED, targets=tg, res=res, info=info) == 0
    want = model(SEED, targets=tg)
    assert np.array_equal(cost, want["cost"]) and np.array_equal(tc, want["target_cost"]) and info.n_reached == want["n_reached"]
    assert_same(m.ReachField(SEED, targets=tg), want, "after the errors")
