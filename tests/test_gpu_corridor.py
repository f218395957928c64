"""Free-space corridors on the GPU (fiesta_hip_free_boxes[_dev] and fiesta_hip_path_corridor[_dev], include/fiesta_hip.h; kernels:
fiesta_amd/csrc/corridor_kernels.hpp), on the dense and the hash-block store.

The expected values are always fiesta_amd.free_box_model / corridor_model (the header's definition in plain Python;
tests/test_corridor_rule.py checks it against literal loops), fed from what the map itself reports through calls that existed before
-- download_field or download_hash, GetDistance -- and, for the corridors, from the paths that ReachField / ReachPaths return: never
from the calls under test.  Every comparison is exact equality of every array, f64 bits included.

The map is that of tests/test_gpu_reach_paths.py, 48 x 40 x 72 voxels at 0.1 m (z is no multiple of 32, walls at every 6th x-plane
with alternating 3-voxel gaps, the closed pocket), with one block that is never observed and two obstacle voxels that close a
diagonal step from both sides.  The window is None or ((3, 2, 5), (44, 37, 66)), whose z origin is unaligned: with max_grow 64 the
boxes span more than two z-words and slabs run to more than 64 items.
"""
import ctypes as C

import numpy as np
import pytest

from scenarios import P_DEFAULT, all_voxels
from test_gpu_reach_paths import BOX, HASH_SHIFT, POCKET, RES, SEED, SHAPE, maze_walls, new_dense, occupy

pytestmark = pytest.mark.gpu
THROUGH = 1
OK, INVALID, BLOCKED = 0, 1, 2
ERR_INVALID = 1
INT32_MIN = -2 ** 31
UNKNOWN_BLOCK = (slice(14, 17), slice(10, 16), slice(40, 50))       # never observed, in the corridor between the walls at x = 12 and 18
SQUEEZE = ((9, 20, 20), (8, 21, 20))                                # occupied: the step (8, 20, 20) -> (9, 21, 20) has no free side
KEYS = ("offsets", "boxes", "boxes_pos", "stop", "entry", "status", "n_chain", "blocked_segment", "blocked_vox")
BOX_KEYS = ("box", "box_pos", "stop", "volume", "status")
MODES = ((False, 1), (True, 8), (True, 4096))                       # (shortcut, max_span): raw, span 8, span 4096


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same(got, want, keys, what=""):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        diff = bits(got[k]) != bits(want[k])
        bad = np.flatnonzero(diff.reshape(len(diff), -1).any(1)) if diff.size else []
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} rows, first at {bad[:3].tolist()}: got {got[k][bad[:3]].tolist()} " \
                              f"want {want[k][bad[:3]].tolist()}"


class World:
    """the map of one store, its dump (observed, occupied, GetDistance of every voxel) and the model's arguments; built once"""

    def __init__(self, store):
        import fiesta_amd
        self.store = store
        obs = np.ones(SHAPE, bool)
        obs[UNKNOWN_BLOCK] = False
        walls = maze_walls()
        walls[SQUEEZE[0]] = walls[SQUEEZE[1]] = True
        assert not (walls & ~obs).any()
        if store == "dense":
            self.shift = np.zeros(3, np.int64)
            self.m = new_dense()
        else:
            self.shift = HASH_SHIFT
            self.m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=200000, mode="hash")
            self.m.SetParameters(*P_DEFAULT)
            self.m.SetOriginalRange()
        s = self.shift
        self.m.SetOccupancy((np.argwhere(obs & ~walls) + s).astype(np.int32), 0, want_ret=False)
        self.m.UpdateOccupancy(True)
        self.m.UpdateESDF()
        occupy(self.m, np.argwhere(walls) + s)
        if store == "dense":
            self.org = np.zeros(3, np.int64)
            f = self.m.download_field(("d2", "occ"))
            self.obs, self.occ = (f["d2"] >= 0).reshape(SHAPE), f["occ"].reshape(SHAPE) != 0
            dims = SHAPE
        else:                                            # download_hash scattered into an array around the maze: the rest is unknown
            lo, hi = s - 6, s + np.array(SHAPE) + 5
            h = self.m.download_hash()
            keep = np.all((h["vox"] >= lo) & (h["vox"] <= hi), axis=1)
            assert keep.sum() >= obs.sum()
            i = tuple((h["vox"][keep] - lo).T)
            dims = tuple(int(v) for v in hi - lo + 1)
            self.obs, self.occ = np.zeros(dims, bool), np.zeros(dims, bool)
            self.obs[i], self.occ[i] = h["d2"][keep] >= 0, h["occ"][keep] != 0
            self.org = lo
        assert self.obs.sum() == obs.sum() and self.occ.sum() == walls.sum()
        self.dist = self.m.GetDistance((all_voxels(dims).astype(np.int64) + self.org).astype(np.int32)).reshape(dims)
        self.kw = dict(dist=self.dist, origin_vox=tuple(int(v) for v in self.org), bounded=store == "dense", resolution=RES, origin=(0.0, 0.0, 0.0))
        self.paths = {}

    def vox(self, v):
        """maze voxel(s) -> map voxel(s) of this store"""
        return (np.asarray(v, np.int64) + self.shift).astype(np.int32)

    def window(self, boxed):
        return (tuple(int(v) for v in self.vox(BOX[0])), tuple(int(v) for v in self.vox(BOX[1]))) if boxed else (None, None)

    def reach_paths(self, conn, shortcut, span):
        """the paths of the EXISTING calls to 300 seeded targets (ReachField in BOX, then ReachPaths): the corridor's input"""
        key = (conn, shortcut, span)
        if key not in self.paths:
            rng = np.random.RandomState(77)
            tg = self.vox(rng.randint(np.array(BOX[0]) - 1, np.array(BOX[1]) + 2, (300, 3)))
            lo, hi = self.window(True)
            self.m.ReachField(self.vox(SEED), lo, hi, connectivity=conn, want_cost=False)
            self.paths[key] = self.m.ReachPaths(tg, connectivity=conn, shortcut=shortcut, max_span=span)
        return self.paths[key]


_worlds = {}


@pytest.fixture(scope="module")
def worlds(hip_lib):
    def get(store):
        if store not in _worlds:
            _worlds[store] = World(store)
        return _worlds[store]
    yield get
    for w in _worlds.values():
        w.m.close()
    _worlds.clear()


def make_seeds(w, boxed):
    """about 2000 seeded random voxels in and just around the window, then the specials: a wall voxel, a voxel outside the window
    (boxed) or outside the array (not boxed), the pocket, an unobserved voxel, the array's two far corners, a voxel beyond +-2^30"""
    rng = np.random.RandomState(2025)
    lo, hi = (np.array(BOX[0]), np.array(BOX[1])) if boxed else (np.zeros(3, int), np.array(SHAPE) - 1)
    t = rng.randint(lo - 1, hi + 2, (2000, 3))
    special = np.array([(6, 20, 36), (1, 20, 36) if boxed else (-1, 20, 36), POCKET, (15, 12, 45), (0, 0, 0), tuple(s - 1 for s in SHAPE)])
    far = np.array([(2 ** 30 + 5, 0, 0)], np.int32)                             # beyond every window
    return np.concatenate([w.vox(np.concatenate([t, special])), far])


@pytest.mark.parametrize("boxed", [False, True])
@pytest.mark.parametrize("store", ["dense", "hash"])
def test_free_boxes(worlds, store, boxed):
    from fiesta_amd import free_box_model
    w = worlds(store)
    lo, hi = w.window(boxed)
    seeds = make_seeds(w, boxed)
    statuses, stops = set(), set()
    for max_grow in (0, 1, 4, 64):
        for clr in (0.0, 0.25):
            for flags in (0, THROUGH):
                want = free_box_model(w.obs, w.occ, seeds, lo=lo, hi=hi, max_grow=max_grow, min_clearance=clr, flags=flags, **w.kw)
                got = w.m.FreeBoxes(seeds, lo, hi, max_grow, clr, flags)
                assert_same(got, want, BOX_KEYS, f"{store} boxed={boxed} max_grow={max_grow} clearance={clr} flags={flags}")
                statuses |= set(want["status"].tolist())
                stops |= set(want["stop"][want["status"] == 0].ravel().tolist())
                if max_grow == 0:                                                   # guarantee 5
                    ok = got["status"] == 0
                    assert np.array_equal(got["box"][ok], np.concatenate([seeds[ok], seeds[ok]], axis=1)) and (got["volume"][ok] == 1).all()
                if max_grow == 64 and clr == 0.0:
                    ok = want["status"] == 0
                    ext = want["box"][ok, 3:].astype(np.int64) - want["box"][ok, :3] + 1
                    # boxes over more than two z-words, and slabs of more than 64 items (rows x z-words, or columns)
                    assert ext[:, 2].max() > (32 if boxed else 64) and (ext[:, 0] * ext[:, 1]).max() > 64 and (ext[:, 1] * ((ext[:, 2] + 31) // 32)).max() > 64
    special = want["status"][-7:].tolist()                                          # (max_grow 64, clearance 0.25, through unknown)
    outside = 0 if store == "hash" and not boxed else 1                             # (an unbounded hash-block map has no outside: unknown)
    assert special[0] == 2 and special[1] == outside and special[3] == 0 and special[6] == 1, special
    # (every status and every stop code occurs -- but EDGE cannot without a window on a map that has no outside)
    assert statuses == {0, 1, 2} and stops == ({1, 3} if store == "hash" and not boxed else {1, 2, 3}), (statuses, stops)


def test_free_boxes_device_variant_and_repeat(worlds):
    import torch
    from fiesta_amd import free_box_model
    for store in ("dense", "hash"):
        w = worlds(store)
        lo, hi = w.window(True)
        seeds = make_seeds(w, True)[-300:]
        n = len(seeds)
        want = free_box_model(w.obs, w.occ, seeds, lo=lo, hi=hi, max_grow=64, **w.kw)
        dev = torch.device("cuda", 0)
        sd = torch.tensor(seeds, device=dev)
        t = {"box": torch.full((n + 2, 6), -77, dtype=torch.int32, device=dev), "box_pos": torch.full((n + 2, 6), -77.0, dtype=torch.float64, device=dev),
             "stop": torch.full((n + 2, 6), 77, dtype=torch.uint8, device=dev), "volume": torch.full((n + 2,), -77, dtype=torch.int64, device=dev),
             "status": torch.full((n + 2,), -77, dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()
        for rep in range(2):                                                        # the same call twice: the same bits
            w.m.FreeBoxesDevice(sd.data_ptr(), n, lo, hi, 64, box_dev_ptr=t["box"].data_ptr(), box_pos_dev_ptr=t["box_pos"].data_ptr(),
                                stop_dev_ptr=t["stop"].data_ptr(), volume_dev_ptr=t["volume"].data_ptr(), status_dev_ptr=t["status"].data_ptr())
            w.m.synchronize()
            got = {k: v.cpu().numpy() for k, v in t.items()}
            assert all((np.abs(got[k][n:].astype(np.float64)) == 77).all() for k in BOX_KEYS)      # nothing beyond n entries
            assert_same({k: v[:n] for k, v in got.items()}, want, BOX_KEYS, f"{store} device, call {rep}")
        # each nullable output alone, host variant
        from fiesta_amd._lib import FreeBoxesResult
        from fiesta_amd.esdf_map import _p
        for i, k in enumerate(BOX_KEYS):
            a = np.zeros_like(want[k])
            res = FreeBoxesResult(*[a.ctypes.data if j == i else None for j in range(5)])
            blo, bhi = np.array(lo, np.int32), np.array(hi, np.int32)
            assert w.m._lib.fiesta_hip_free_boxes(w.m._h, _p(blo), _p(bhi), _p(seeds), n, 0.0, 64, 0, C.byref(res)) == 0
            assert np.array_equal(bits(a), bits(want[k])), (store, k)
        assert w.m.FreeBoxes(np.zeros((0, 3), np.int32))["status"].shape == (0,)
        empty = w.m.FreeBoxes(seeds, (5, 5, 5), (4, 9, 9))                          # an empty window: every seed OUTSIDE
        assert (empty["status"] == 1).all() and (empty["box"] == INT32_MIN).all() and np.isnan(empty["box_pos"]).all()


@pytest.mark.parametrize("boxed", [False, True])
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("store", ["dense", "hash"])
def test_corridors_along_reach_paths(worlds, store, conn, boxed):
    from fiesta_amd import corridor_model
    w = worlds(store)
    lo, hi = w.window(boxed)
    taken_b = 0
    for shortcut, span in MODES:
        rp = w.reach_paths(conn, shortcut, span)
        reached = rp["status"] == 0
        assert reached.sum() > 150                                                  # (so that the test cannot pass on empty corridors)
        for max_grow in (4, 64):
            stats = {}
            want = corridor_model(w.obs, w.occ, rp["waypoints_vox"], rp["offsets"], lo=lo, hi=hi, max_grow=max_grow, stats=stats, **w.kw)
            taken_b += stats["segments_b"]
            assert (want["status"][reached] == OK).all(), np.flatnonzero(want["status"][reached] != OK)[:5]
            assert (np.diff(want["offsets"])[reached] >= 1).all()
            got = w.m.PathCorridor(rp["waypoints_vox"], rp["offsets"], lo, hi, max_grow)
            assert_same(got, want, KEYS, f"{store} conn={conn} boxed={boxed} shortcut={shortcut} span={span} max_grow={max_grow}")
            print(f"{store} conn {conn} boxed {boxed} shortcut {shortcut} span {span} max_grow {max_grow}: {want['offsets'][-1]} boxes, "
                  f"{stats['segments_b']} segments took B")
    assert taken_b > 0


def hand_paths(w):
    """(waypoints, offsets, expected statuses): a segment through a wall; the diagonal squeeze; a first waypoint in a wall; one outside
    the window; a segment of more than 4095 voxel steps; an empty path; one waypoint; repeated waypoints; a free diagonal walk"""
    paths = [[(4, 20, 36), (8, 20, 36)], [(8, 19, 20), (8, 20, 20), (9, 21, 20)], [(6, 20, 36), (5, 20, 36)], [(1, 20, 36), (4, 20, 36)],
             [(4, 20, 36), (4, 20, 36 + 4096)], [], [(4, 20, 36)], [(4, 20, 36), (4, 20, 36), (4, 21, 37), (4, 21, 37), (4, 21, 37), (5, 22, 38)],
             [(4, 5, 8), (5, 30, 60)]]
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
    pts = w.vox(np.array([v for p in paths for v in p]))
    return pts, off, [BLOCKED, BLOCKED, BLOCKED, BLOCKED, INVALID, OK, OK, OK, OK]


@pytest.mark.parametrize("store", ["dense", "hash"])
def test_hand_made_paths(worlds, store):
    import fiesta_amd
    from fiesta_amd import corridor_model
    w = worlds(store)
    lo, hi = w.window(True)
    pts, off, statuses = hand_paths(w)
    want = corridor_model(w.obs, w.occ, pts, off, lo=lo, hi=hi, max_grow=4, **w.kw)
    assert want["status"].tolist() == statuses
    assert want["blocked_segment"].tolist() == [0, 1, -1, -1, -1, -1, -1, -1, -1]
    assert want["blocked_vox"][:4].tolist() == [w.vox(v).tolist() for v in ((6, 20, 36), SQUEEZE[1], (6, 20, 36), (1, 20, 36))]
    assert (want["blocked_vox"][4:] == INT32_MIN).all() and want["n_chain"].tolist()[:8] == [1, 2, 0, 0, 0, 0, 1, 6]
    assert np.diff(want["offsets"]).tolist()[:7] == [1, 2, 0, 0, 0, 0, 1] and want["n_chain"][8] == 1 + 1 + 25 + 52
    got = w.m.PathCorridor(pts, off, lo, hi, 4)
    assert_same(got, want, KEYS, f"{store} hand-made")
    # reversed offsets: INVALID for that path alone in the device variant, a whole-call error in the host variant
    rev = off.copy()
    rev[[1, 2]] = rev[[2, 1]]
    wrev = corridor_model(w.obs, w.occ, pts, rev, lo=lo, hi=hi, max_grow=4, **w.kw)
    assert wrev["status"].tolist() == [BLOCKED, INVALID, BLOCKED] + statuses[3:]     # ([0, 5): two paths joined; [5, 2): reversed; [2, 7))
    assert_same(trimmed(device_corridor(w.m, pts, rev, lo, hi, 4)), wrev, KEYS, f"{store} reversed offsets, device")
    with pytest.raises(fiesta_amd.FiestaHipError) as e:
        w.m.PathCorridor(pts, rev, lo, hi, 4)
    assert e.value.code == ERR_INVALID and "non-decreasing" in str(e.value)
    far = off.copy()
    far[-1] += 1                                                                     # beyond the waypoints
    assert device_corridor(w.m, pts, far, lo, hi, 4)["status"].tolist() == statuses[:-1] + [INVALID]
    assert_same(w.m.PathCorridor(pts, off, lo, hi, 4), want, KEYS, f"{store} after the errors")
    none = w.m.PathCorridor(np.zeros((0, 3), np.int32), [0], lo, hi, 4)
    assert none["offsets"].tolist() == [0] and len(none["boxes"]) == 0


def device_corridor(m, pts, off, lo, hi, max_grow, capacity=None, pad=4, flags=0, clr=0.0, wp_ptr=None, off_ptr=None, n_wp=None, n_paths=None):
    """PathCorridorDevice with torch tensors (or device addresses of the waypoints and their offsets): a sizing call unless `capacity`
    is given; returns numpy arrays, the per-box ones `pad` rows longer than the capacity and filled with 77s"""
    import torch
    dev = torch.device("cuda", 0)
    if wp_ptr is None:
        wd = torch.tensor(np.ascontiguousarray(pts, np.int32), device=dev)
        od = torch.tensor(np.ascontiguousarray(off, np.int64), device=dev)
        wp_ptr, off_ptr, n_wp, n_paths = wd.data_ptr(), od.data_ptr(), len(pts), len(off) - 1
    n = n_paths
    o = torch.full((n + 1,), -77, dtype=torch.int64, device=dev)
    per = {k: torch.full((n, 3) if k == "blocked_vox" else (n,), -77, dtype=torch.int32, device=dev) for k in ("status", "n_chain", "blocked_segment", "blocked_vox")}
    torch.cuda.synchronize()
    kw = dict(lo=lo, hi=hi, max_grow=max_grow, min_clearance=clr, flags=flags)
    if capacity is None:
        m.PathCorridorDevice(wp_ptr, n_wp, off_ptr, n, o.data_ptr(), capacity=0, **kw)
        m.synchronize()
        capacity = int(o.cpu()[n])
    box = {"boxes": torch.full((capacity + pad, 6), -77, dtype=torch.int32, device=dev), "boxes_pos": torch.full((capacity + pad, 6), -77.0, dtype=torch.float64, device=dev),
           "stop": torch.full((capacity + pad, 6), 77, dtype=torch.uint8, device=dev), "entry": torch.full((capacity + pad,), -77, dtype=torch.int32, device=dev)}
    o.fill_(-77)
    torch.cuda.synchronize()
    m.PathCorridorDevice(wp_ptr, n_wp, off_ptr, n, o.data_ptr(), capacity=capacity, boxes_dev_ptr=box["boxes"].data_ptr(),
                         boxes_pos_dev_ptr=box["boxes_pos"].data_ptr(), stop_dev_ptr=box["stop"].data_ptr(), entry_dev_ptr=box["entry"].data_ptr(),
                         status_dev_ptr=per["status"].data_ptr(), n_chain_dev_ptr=per["n_chain"].data_ptr(),
                         blocked_segment_dev_ptr=per["blocked_segment"].data_ptr(), blocked_vox_dev_ptr=per["blocked_vox"].data_ptr(), **kw)
    m.synchronize()
    out = {"offsets": o.cpu().numpy()}
    out.update({k: v.cpu().numpy() for k, v in box.items()})
    out.update({k: v.cpu().numpy() for k, v in per.items()})
    return out


def trimmed(r, pad=4):
    out = dict(r)
    total = int(r["offsets"][-1])
    for k in ("boxes", "boxes_pos", "stop", "entry"):
        assert len(r[k]) == total + pad and (np.abs(r[k][total:].astype(np.float64)) == 77).all(), k
        out[k] = r[k][:total]
    return out


def host_buffers(n, cap):
    from fiesta_amd._lib import CorridorResult
    a = {"offsets": np.full(n + 1, -77, np.int64), "boxes": np.full((cap, 6), -77, np.int32), "boxes_pos": np.full((cap, 6), -77.0),
         "stop": np.full((cap, 6), 77, np.uint8), "entry": np.full(cap, -77, np.int32), "status": np.full(n, -77, np.int32),
         "n_chain": np.full(n, -77, np.int32), "blocked_segment": np.full(n, -77, np.int32), "blocked_vox": np.full((n, 3), -77, np.int32)}
    return a, CorridorResult(*[a[k].ctypes.data for k in KEYS])


def raw_corridor(m, pts, off, res, lo, hi, max_grow, capacity):
    from fiesta_amd.esdf_map import _p
    blo, bhi = np.array(lo, np.int32), np.array(hi, np.int32)
    return m._lib.fiesta_hip_path_corridor(m._h, _p(blo), _p(bhi), _p(pts), len(pts), _p(off), len(off) - 1, 0.0, max_grow, 0, capacity, C.byref(res))


@pytest.mark.parametrize("store", ["dense", "hash"])
def test_capacity_nullable_outputs_and_variants(worlds, store):
    from fiesta_amd import corridor_model
    from fiesta_amd._lib import CorridorResult
    w = worlds(store)
    lo, hi = w.window(True)
    rp = w.reach_paths(26, True, 8)
    pts, off = rp["waypoints_vox"], rp["offsets"][:121].copy()                       # the first 120 paths
    pts = np.ascontiguousarray(pts[:off[-1]])
    n = len(off) - 1
    want = corridor_model(w.obs, w.occ, pts, off, lo=lo, hi=hi, max_grow=4, **w.kw)
    total = int(want["offsets"][-1])
    inner = int(want["offsets"][np.flatnonzero(np.diff(want["offsets"]) >= 3)[3]] + 1)      # the middle of a path's boxes
    assert 0 < inner < total
    for cap in (0, inner, total):
        a, res = host_buffers(n, total + 5)
        assert raw_corridor(w.m, pts, off, res, lo, hi, 4, cap) == 0
        d = device_corridor(w.m, pts, off, lo, hi, 4, capacity=cap, pad=5 + total - cap)
        for r, who in ((a, "host"), (d, "device")):
            for k in ("offsets", "status", "n_chain", "blocked_segment", "blocked_vox"):      # the true totals whatever the capacity
                assert np.array_equal(r[k], want[k]), (k, cap, who)
            for k in ("boxes", "boxes_pos", "stop", "entry"):
                assert np.array_equal(bits(r[k][:cap]), bits(want[k][:cap])) and (np.abs(r[k][cap:].astype(np.float64)) == 77).all(), (k, cap, who)
    # each nullable output asked for alone (offsets is required)
    for i, k in enumerate(KEYS[1:], 1):
        a, _ = host_buffers(n, total)
        res = CorridorResult(*[a[key].ctypes.data if j in (0, i) else None for j, key in enumerate(KEYS)])
        assert raw_corridor(w.m, pts, off, res, lo, hi, 4, total) == 0
        assert np.array_equal(bits(a[k]), bits(want[k])) and np.array_equal(a["offsets"], want["offsets"]), (store, k)
    # host and device variants, and the same call twice
    first = trimmed(device_corridor(w.m, pts, off, lo, hi, 4))
    assert_same(first, want, KEYS, f"{store} device")
    assert_same(trimmed(device_corridor(w.m, pts, off, lo, hi, 4)), first, KEYS, f"{store} device, again")
    assert_same(w.m.PathCorridor(pts, off, lo, hi, 4), want, KEYS, f"{store} host")
    assert w.m.PathCorridor(pts, off, lo, hi, 4, want_pos=False)["boxes_pos"] is None


@pytest.mark.parametrize("store", ["dense", "hash"])
def test_device_chain_equals_the_host_route(worlds, store):
    """reach_field_dev -> reach_paths_dev -> path_corridor_dev with nothing but sizes read back in between"""
    import torch
    w = worlds(store)
    lo, hi = w.window(True)
    rp = w.reach_paths(26, True, 4096)
    host = w.m.PathCorridor(rp["waypoints_vox"], rp["offsets"], lo, hi, 64, min_clearance=0.0)
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(77)
    tg = w.vox(rng.randint(np.array(BOX[0]) - 1, np.array(BOX[1]) + 2, (300, 3)))
    n = len(tg)
    sd, td = torch.tensor(w.vox(SEED), device=dev), torch.tensor(tg, device=dev)
    off = torch.full((n + 1,), -77, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    w.m.ReachFieldDevice(sd.data_ptr(), 1, lo, hi, connectivity=26)
    total = int(rp["offsets"][-1])                                                    # (the size of the waypoint buffer)
    vox = torch.full((total, 3), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    w.m.ReachPathsDevice(td.data_ptr(), n, off.data_ptr(), connectivity=26, shortcut=True, max_span=4096, capacity=total,
                         waypoints_vox_dev_ptr=vox.data_ptr())
    got = trimmed(device_corridor(w.m, None, None, lo, hi, 64, wp_ptr=vox.data_ptr(), off_ptr=off.data_ptr(), n_wp=total, n_paths=n))
    assert_same(got, host, KEYS, f"{store} device chain")
    assert host["offsets"][-1] > 200


@pytest.mark.parametrize("store", ["dense", "hash"])
def test_guarantees_on_the_gpu_output(worlds, store):
    """1 - 4 checked on what the library returned, against the map's dump and the chain rule, without the corridor model"""
    from fiesta_amd import corridor_chain
    from fiesta_amd.reach_model import reach_traversable
    w = worlds(store)
    lo, hi = w.window(True)
    wlo, whi = np.array(lo, np.int64), np.array(hi, np.int64)
    trav = reach_traversable(w.obs, w.occ)
    max_grow = 4

    def free(a, b):                                       # every voxel of the inclusive map-voxel box, which lies inside the dump's arrays
        a, b = np.asarray(a) - w.org, np.asarray(b) - w.org
        return bool(trav[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1].all())

    rp = w.reach_paths(26, False, 1)
    got = w.m.PathCorridor(rp["waypoints_vox"], rp["offsets"], lo, hi, max_grow)
    assert (got["status"] == OK).all() and got["offsets"][-1] > 2000
    boxes, stop = got["boxes"].astype(np.int64), got["stop"]
    assert (boxes[:, :3] >= wlo).all() and (boxes[:, 3:] <= whi).all() and (boxes[:, :3] <= boxes[:, 3:]).all()
    for k, (b, s) in enumerate(zip(boxes, stop)):
        assert free(b[:3], b[3:]), k                                                              # 1
        for f in range(6):                                                                        # 4
            a = f >> 1
            c = b[3 + a] + 1 if f & 1 else b[a] - 1
            if s[f] == 2:
                assert c < wlo[a] or c > whi[a], (k, f)
            elif s[f] == 1:
                sl, sh = b[:3].copy(), b[3:].copy()
                sl[a] = sh[a] = c
                assert wlo[a] <= c <= whi[a] and not free(sl, sh), (k, f)
            else:
                assert s[f] == 3, (k, f)
    grown_limit = 0
    for p in range(len(rp["offsets"]) - 1):
        a, b = got["offsets"][p], got["offsets"][p + 1]
        bx, entry = boxes[a:b], got["entry"][a:b]
        if b - a > 1:
            assert (np.maximum(bx[:-1, :3], bx[1:, :3]) <= np.minimum(bx[:-1, 3:], bx[1:, 3:])).all(), p   # 2
        pts = [tuple(int(c) for c in v) for v in rp["waypoints_vox"][rp["offsets"][p]:rp["offsets"][p + 1]]]
        if not pts:
            assert a == b
            continue
        chain = [pts[0]]
        for u, v in zip(pts[:-1], pts[1:]):
            if u != v:
                ca, cb = corridor_chain(u, v)
                chain += (ca if all(free(x, x) for x in ca) else cb)[1:]
        assert got["n_chain"][p] == len(chain) and entry[0] == 0 and (np.diff(entry) > 0).all()
        ch = np.array(chain)
        k = np.searchsorted(entry, np.arange(len(chain)), side="right") - 1
        assert ((bx[k, :3] <= ch) & (ch <= bx[k, 3:])).all(), p                                  # 3
        grown_limit += int((stop[a:b] == 3).sum())
    assert grown_limit > 0


def test_the_next_call_sees_a_new_obstacle(hip_lib):
    from fiesta_amd import free_box_model
    m = new_dense((20, 18, 40))
    m.SetOccupancyBox((0, 0, 0), (19, 17, 39), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    seed = [(10, 9, 20)]
    before = m.FreeBoxes(seed, max_grow=8)
    assert before["box"][0].tolist() == [2, 1, 12, 18, 17, 28] and before["stop"][0].tolist() == [3, 3, 3, 3, 3, 3]
    obstacle = (13, 9, 20)
    S = np.array([obstacle], np.int32)
    for _ in range(3):                                                               # three hits make an obstacle
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    after = m.FreeBoxes(seed, max_grow=8)
    b = after["box"][0]
    assert not all(b[c] <= obstacle[c] <= b[3 + c] for c in range(3)) and after["stop"][0][1] == 1 and b[3] == 12
    f = m.download_field(("d2", "occ"))
    want = free_box_model((f["d2"] >= 0).reshape(20, 18, 40), f["occ"].reshape(20, 18, 40) != 0, seed, max_grow=8, resolution=RES)
    assert_same(after, want, BOX_KEYS, "after the obstacle")
    cor = m.PathCorridor([(10, 9, 20), (16, 9, 20)], [0, 2], max_grow=2)
    assert cor["status"].tolist() == [BLOCKED] and cor["blocked_vox"].tolist() == [list(obstacle)] and cor["blocked_segment"].tolist() == [0]
    m.close()
