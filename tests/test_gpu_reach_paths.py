"""Reach paths on the GPU (fiesta_hip_reach_paths[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/reach_path_kernels.hpp).

The expected paths are always fiesta_amd.reach_paths_model (the header's definition in plain Python; tests/test_reach_paths_rule.py
checks it against literal loops) over the cost field of fiesta_amd.reach_model, fed from what the map itself reports through calls
that existed before -- download_field or download_hash, GetDistance -- never from the call under test.  Every comparison is exact
equality of every array: offsets, voxels, positions (f64 bits), status, number of moves.

The map is that of tests/test_gpu_reach.py, 48 x 40 x 72 voxels at 0.1 m: z is no multiple of 32, the reach tiles form a 3 x 3 x 3
grid, seven walls across x with alternating gaps make the paths turn; here one corridor also holds an enclosed pocket.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from scenarios import P_DEFAULT, all_voxels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.1
SHAPE = (48, 40, 72)
INF = 2 ** 31 - 1
THROUGH = 1
BOX = ((3, 2, 5), (44, 37, 66))     # unaligned z origin; the faces keep one row of every gap
SEED = [(4, 20, 36)]
POCKET = (21, 20, 30)               # free, inside a closed 3 x 3 x 3 shell: traversable and never reached
OK, OUTSIDE, BLOCKED, UNREACHED, BROKEN = range(5)
ERR_INVALID, ERR_STATE = 1, 4
KEYS = ("offsets", "waypoints_vox", "waypoints_pos", "status", "n_moves")
MODES = ((False, 4096), (True, 1), (True, 8), (True, 4096))     # (shortcut, max_span)


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
    """tests/test_gpu_reach.py's maze -- walls across x at every 6th x-plane, full height, with a gap 3 voxels wide that alternates
    between y = low and y = high -- and a closed shell around POCKET"""
    occ = np.zeros(shape, bool)
    for k, x in enumerate(range(6, shape[0], 6)):
        occ[x] = True
        if k % 2 == 0:
            occ[x, :3] = False
        else:
            occ[x, shape[1] - 3:] = False
    px, py, pz = POCKET
    occ[px - 1:px + 2, py - 1:py + 2, pz - 1:pz + 2] = True
    occ[POCKET] = False
    return occ


def dump(m, origin=(0, 0, 0), with_dist=False):
    """observed, occupied (and GetDistance of every voxel) of a dense map, from calls that existed before"""
    f = m.download_field(("d2", "occ"))
    dims = m.grid_size
    dist = m.GetDistance(all_voxels(dims) + np.asarray(origin, np.int32)).reshape(dims) if with_dist else None
    return (f["d2"] >= 0).reshape(dims), f["occ"].reshape(dims) != 0, dist


def want_paths(field, targets, conn, shortcut, span, origin=(0.0, 0.0, 0.0)):
    from fiesta_amd import reach_paths_model
    return reach_paths_model(field["cost"], field["box_lo"], targets, conn, 1 if shortcut else 0, span, origin, RES)


def assert_same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        diff = got[k] != want[k]
        bad = np.argwhere(diff.reshape(len(diff), -1).any(1)) if diff.size else np.zeros((0, 1), np.int64)
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} rows, first at {bad[:3].ravel().tolist()}: got " \
                              f"{got[k][bad[:3].ravel()].tolist()} want {want[k][bad[:3].ravel()].tolist()}"


def path_slices(r, idx):
    """the result restricted to the targets `idx` (a new CSR)"""
    off = r["offsets"]
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = {"offsets": np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in idx])]).astype(np.int64), "status": r["status"][idx],
           "n_moves": r["n_moves"][idx], "waypoints_vox": r["waypoints_vox"][rows], "waypoints_pos": r["waypoints_pos"][rows]}
    return out


def make_targets():
    """about 2000 seeded random voxels in and just around the box, then the specials: the seed itself, a wall voxel, a voxel outside
    the box, the pocket"""
    rng = np.random.RandomState(2024)
    lo, hi = np.array(BOX[0]), np.array(BOX[1])
    t = rng.randint(lo - 1, hi + 2, (2000, 3))
    special = np.array([SEED[0], (6, 20, 36), (1, 20, 36), POCKET])
    return np.concatenate([t, special]).astype(np.int32)


class Maze:
    """the map, its dump, the model's floods and paths; everything computed once and left unchanged"""

    def __init__(self):
        from fiesta_amd import reach_model
        self.m = new_dense()
        self.m.SetOccupancyBox((0, 0, 0), tuple(s - 1 for s in SHAPE), 0)
        self.m.UpdateOccupancy(True)
        self.m.UpdateESDF()
        walls = maze_walls()
        occupy(self.m, np.argwhere(walls))
        self.obs, self.occ, _ = dump(self.m)
        assert self.obs.all() and np.array_equal(self.occ, walls)
        self.targets = make_targets()
        self.field = {c: reach_model(self.obs, self.occ, SEED, lo=BOX[0], hi=BOX[1], connectivity=c) for c in (6, 26)}
        self.memo = {}

    def want(self, conn, shortcut, span):
        key = (conn, shortcut, span)
        if key not in self.memo:
            self.memo[key] = want_paths(self.field[conn], self.targets, conn, shortcut, span)
        return self.memo[key]

    def flood(self, conn):
        """leaves the flood of BOX in the map's scratch; returns the info"""
        info = self.m.ReachField(SEED, BOX[0], BOX[1], connectivity=conn, want_cost=False)
        assert info["box_lo"] == list(BOX[0]) and info["n_reached"] == self.field[conn]["n_reached"]
        return info


@pytest.fixture(scope="module")
def maze(hip_lib):
    z = Maze()
    yield z
    z.m.close()


@pytest.mark.parametrize("conn", [6, 26])
def test_serpentine_maze(maze, conn):
    m = maze.m
    maze.flood(conn)
    raw = maze.want(conn, False, 4096)
    n = len(maze.targets)
    assert raw["status"][-4:].tolist() == [OK, BLOCKED, OUTSIDE, UNREACHED] and raw["n_moves"][-4] == 0
    assert {OK, OUTSIDE, BLOCKED} <= set(raw["status"][:-4].tolist()) and (raw["status"] == OK).sum() > 1400
    assert raw["n_moves"].max() > 200                                   # through seven walls: far more moves than one window of 64
    for shortcut, span in MODES:
        want = maze.want(conn, shortcut, span)
        got = m.ReachPaths(maze.targets, connectivity=conn, shortcut=shortcut, max_span=span)
        print(f"maze, connectivity {conn}, shortcut {shortcut} span {span}: {want['offsets'][n]} waypoints, longest path {want['n_moves'].max()} moves")
        assert_same(got, want, f"maze {conn} {shortcut} {span}")
    assert_same(maze.want(conn, True, 1), raw, "max_span 1 is the raw path")
    tight, some = maze.want(conn, True, 4096), maze.want(conn, True, 8)
    assert tight["offsets"][n] < some["offsets"][n] < raw["offsets"][n]
    if conn == 6:
        # a segment of more than 64 moves: the wave's window of 64 voxels went on whole (with 6 moves, voxel steps = moves)
        seg = np.abs(np.diff(tight["waypoints_vox"].astype(np.int64), axis=0)).sum(1)
        inner = np.ones(len(seg), bool)
        o = tight["offsets"][1:-1]
        inner[o[(o > 0) & (o < len(seg) + 1)] - 1] = False     # (pairs that straddle two paths)
        assert seg[inner[:len(seg)]].max() > 64


def segments(got, conn):
    """(k, vox): rows k and k - 1 of the waypoints are the target-side and the seed-side end of one segment; with 26 moves only
    segments of more than one move -- a single diagonal move is a legal move of the flood, which needs only its two ends traversable
    (include/fiesta_hip.h), so it may cut a corner"""
    off, vox = got["offsets"], got["waypoints_vox"].astype(np.int64)
    inner = np.ones(len(vox), bool)
    inner[off[:-1][off[:-1] < len(vox)]] = False                     # (the first waypoint of a path ends no segment)
    k = np.flatnonzero(inner)
    if conn == 26:
        k = k[np.abs(vox[k] - vox[k - 1]).max(1) > 1]
    return k, vox


def test_segments_are_free_for_the_ray_query_and_feed_the_path_cost(maze, hip_lib):
    """the existing calls agree: every shortcut segment, walked from its target-side end as visible() walks it, is free of occupied,
    unknown and outside voxels for fiesta_hip_ray_query (dense map, clearance 0, not through unknown), and the path cost takes
    positions and offsets as they come.

    The ray query takes METRES and divides by the resolution; visible() walks from centre to centre in voxel units.  At 0.1 m the
    quotient is not always the centre: (40 + 0.5) * 0.1 / 0.1 = 40.49999999999999, and no f64 divides to 40.5 at all.  A start one
    ulp off the centre breaks the traversal's ties at voxel corners the other way, so the ray query then walks other voxels than
    visible() tested: in fiesta_amd.ray_query_model 3 of 11507 segments (6 moves) and 2 of 6554 (26 moves) of this map read a wall
    voxel, all exact diagonals from x = 40.  So the check has two halves: on the 0.1 m map every segment whose walk in metres
    (fiesta_amd.ray_walks, the ray query's definition) IS the centre-to-centre walk reads no hit, and that is all but a few per cent; on
    the same maze at 0.125 m, where every quotient is exact, EVERY segment reads no hit."""
    from fiesta_amd import ray_walks, reach_walk
    m = maze.m
    import fiesta_amd
    fine = fiesta_amd.ESDFMap((0, 0, 0), 0.125, tuple((s - 0.5) * 0.125 for s in SHAPE))
    assert fine.grid_size == SHAPE
    fine.SetParameters(*P_DEFAULT)
    fine.SetOriginalRange()
    fine.SetOccupancyBox((0, 0, 0), tuple(s - 1 for s in SHAPE), 0)
    fine.UpdateOccupancy(True)
    fine.UpdateESDF()
    occupy(fine, np.argwhere(maze.occ))
    for conn in (6, 26):
        want = maze.want(conn, True, 4096)
        maze.flood(conn)
        got = m.ReachPaths(maze.targets, connectivity=conn, shortcut=True, max_span=4096)
        assert_same(got, want, f"maze {conn}")
        k, vox = segments(got, conn)
        assert len(k) > 5000
        pos = got["waypoints_pos"]
        hit = m.RayQuery(pos[k], pos[k - 1], stop_mask=7)["hit_index"]
        centre = np.ones(len(k), bool)
        for i, w in enumerate(ray_walks(pos[k], pos[k - 1], RES)):
            e = reach_walk(vox[k[i]], vox[k[i] - 1])
            centre[i] = [tuple(v) for v in w.tolist()] == e[:-1] + [tuple(vox[k[i] - 1])]
        assert (hit[centre] == -1).all(), (conn, vox[k][centre & (hit != -1)][:3].tolist())
        assert (~centre).sum() * 10 < len(k)                                  # (1 % and 3 % in the model: ties at corners are rare)
        print(f"connectivity {conn}: {len(k)} segments, {(~centre).sum()} not walked from centre to centre at 0.1 m, {(hit != -1).sum()} of them hit")
        pc = m.PathCost(pos, got["offsets"], 0.05, 0.3)
        ok = got["status"] == OK
        assert (pc["n_samples"][ok] >= 1).all() and (pc["n_samples"][~ok] == 0).all() and np.isfinite(pc["cost"]).all()
        # 0.125 m: the same maze, the same field, the same voxels; every quotient is the centre
        fine.ReachField(SEED, BOX[0], BOX[1], connectivity=conn, want_cost=False)
        g2 = fine.ReachPaths(maze.targets, connectivity=conn, shortcut=True, max_span=4096)
        assert all(np.array_equal(g2[key], want[key]) for key in KEYS if key != "waypoints_pos")
        assert np.array_equal(g2["waypoints_pos"], (g2["waypoints_vox"].astype(np.float64) + 0.5) * 0.125)
        assert np.array_equal(g2["waypoints_pos"] / 0.125, g2["waypoints_vox"] + 0.5)
        k2, _ = segments(g2, conn)
        assert np.array_equal(k2, k)
        hit = fine.RayQuery(g2["waypoints_pos"][k], g2["waypoints_pos"][k - 1], stop_mask=7)["hit_index"]
        assert (hit == -1).all(), (conn, int((hit != -1).sum()))
        pc = fine.PathCost(g2["waypoints_pos"], g2["offsets"], 0.05, 0.3)
        assert (pc["n_samples"][ok] >= 1).all()
    fine.close()


def raw_call(m, targets, res, cost=None, lo=None, hi=None, n=None, conn=26, flags=0, span=1, capacity=0, dev=False):
    """the C call itself; cost / targets: numpy arrays (host variant) or device addresses (dev); returns the status"""
    from fiesta_amd.esdf_map import _p
    blo = None if lo is None else np.ascontiguousarray(lo, np.int32)
    bhi = None if hi is None else np.ascontiguousarray(hi, np.int32)
    if dev:
        fn, c, t = m._lib.fiesta_hip_reach_paths_dev, C.c_void_p(cost or None), C.c_void_p(targets or None)
    else:
        fn, c, t = m._lib.fiesta_hip_reach_paths, _p(cost), _p(targets)
    return fn(m._h, c, _p(blo), _p(bhi), t, (0 if targets is None else len(targets)) if n is None else n, conn, flags, span, capacity,
              None if res is None else C.byref(res))


def host_result(n, cap, fill=-77):
    from fiesta_amd._lib import ReachPathsResult
    a = {"offsets": np.full(n + 1, fill, np.int64), "waypoints_vox": np.full((cap, 3), fill, np.int32), "waypoints_pos": np.full((cap, 3), float(fill)),
         "status": np.full(n, fill, np.int32), "n_moves": np.full(n, fill, np.int32)}
    return a, ReachPathsResult(*[a[k].ctypes.data for k in KEYS])


def device_paths(m, targets, conn, shortcut, span, cost=None, box=None, capacity=None, pad=5):
    """ReachPathsDevice with torch tensors: a sizing call unless `capacity` is given; returns numpy arrays (waypoint arrays `pad` rows
    longer than the capacity, filled with -77) """
    import torch
    dev = torch.device("cuda", 0)
    n = len(targets)
    td = torch.tensor(np.ascontiguousarray(targets, np.int32), device=dev)
    cd = None if cost is None else torch.tensor(np.ascontiguousarray(cost, np.int32).reshape(-1), device=dev)
    off = torch.full((n + 1,), -77, dtype=torch.int64, device=dev)
    st = torch.full((n,), -77, dtype=torch.int32, device=dev)
    mv = torch.full((n,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kw = dict(cost_dev_ptr=0 if cd is None else cd.data_ptr(), box=box, connectivity=conn, shortcut=shortcut, max_span=span)
    if capacity is None:
        m.ReachPathsDevice(td.data_ptr(), n, off.data_ptr(), capacity=0, **kw)
        sync(m)
        capacity = int(off.cpu()[n])
    vox = torch.full((capacity + pad, 3), -77, dtype=torch.int32, device=dev)
    pos = torch.full((capacity + pad, 3), -77.0, dtype=torch.float64, device=dev)
    off.fill_(-77)
    torch.cuda.synchronize()
    m.ReachPathsDevice(td.data_ptr(), n, off.data_ptr(), capacity=capacity, waypoints_vox_dev_ptr=vox.data_ptr(),
                       waypoints_pos_dev_ptr=pos.data_ptr(), status_dev_ptr=st.data_ptr(), n_moves_dev_ptr=mv.data_ptr(), **kw)
    sync(m)
    return {"offsets": off.cpu().numpy(), "waypoints_vox": vox.cpu().numpy(), "waypoints_pos": pos.cpu().numpy(), "status": st.cpu().numpy(),
            "n_moves": mv.cpu().numpy()}


def sync(m):
    """the _dev variant only enqueues on the map's stream"""
    m.synchronize()


def trimmed(r, pad=5):
    out = dict(r)
    total = int(r["offsets"][-1])
    for k in ("waypoints_vox", "waypoints_pos"):
        assert len(r[k]) == total + pad and (r[k][total:] == -77).all(), k
        out[k] = r[k][:total]
    return out


def test_retained_and_explicit_fields(maze, hip_lib):
    import fiesta_amd
    import torch
    m, tg = maze.m, maze.targets[-300:]
    want = {c: path_slices(maze.want(c, True, 8), np.arange(len(maze.targets) - 300, len(maze.targets))) for c in (6, 26)}
    # a fresh map retains nothing
    fresh = new_dense((8, 8, 8))
    with pytest.raises(fiesta_amd.FiestaHipError) as e:
        fresh.ReachPaths([(1, 1, 1)])
    assert e.value.code == ERR_STATE
    a, res = host_result(1, 0)
    assert raw_call(fresh, np.array([[1, 1, 1]], np.int32), res, dev=False) == ERR_STATE and raw_call(fresh, 0, res, n=0, dev=True) == ERR_STATE
    fresh.close()
    for conn in (6, 26):
        field = m.ReachField(SEED, BOX[0], BOX[1], connectivity=conn)        # host variant: the map retains the field
        assert np.array_equal(field["cost"], maze.field[conn]["cost"])
        box = (field["box_lo"], field["box_hi"])
        assert_same(m.ReachPaths(tg, connectivity=conn, shortcut=True, max_span=8), want[conn], f"retained, host {conn}")
        assert_same(trimmed(device_paths(m, tg, conn, True, 8)), want[conn], f"retained, device {conn}")
        # a mismatch with the retained connectivity is refused, and the field stays
        with pytest.raises(fiesta_amd.FiestaHipError) as e:
            m.ReachPaths(tg, connectivity=32 - conn, shortcut=True, max_span=8)
        assert e.value.code == ERR_INVALID and "connectivity" in str(e.value)
        assert_same(m.ReachPaths(tg, connectivity=conn, shortcut=True, max_span=8), want[conn], f"retained after the refusal {conn}")
        # a _dev flood into the caller's array leaves nothing retained
        dev = torch.device("cuda", 0)
        cost_dev = torch.full((field["cost"].size,), -99, dtype=torch.int32, device=dev)
        sd = torch.tensor(SEED, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        m.ReachFieldDevice(sd.data_ptr(), 1, BOX[0], BOX[1], connectivity=conn, cost_dev_ptr=cost_dev.data_ptr())
        assert np.array_equal(cost_dev.cpu().numpy().reshape(field["cost"].shape), field["cost"])
        with pytest.raises(fiesta_amd.FiestaHipError) as e:
            m.ReachPaths(tg, connectivity=conn)
        assert e.value.code == ERR_STATE
        # ... the _dev variant reads that array in place and still retains nothing
        import fiesta_amd.esdf_map  # noqa: F401
        got = device_paths(m, tg, conn, True, 8, cost=field["cost"], box=box)
        assert_same(trimmed(got), want[conn], f"explicit, device {conn}")
        with pytest.raises(fiesta_amd.FiestaHipError) as e:
            m.ReachPaths(tg, connectivity=conn)
        assert e.value.code == ERR_STATE
        # a _dev flood without a cost array does retain
        m.ReachFieldDevice(sd.data_ptr(), 1, BOX[0], BOX[1], connectivity=conn)
        assert_same(m.ReachPaths(tg, connectivity=conn, shortcut=True, max_span=8), want[conn], f"retained by the device flood {conn}")
        # an empty-box flood leaves nothing retained
        m.ReachField(SEED, (5, 5, 5), (4, 9, 9), connectivity=conn)
        with pytest.raises(fiesta_amd.FiestaHipError) as e:
            m.ReachPaths(tg, connectivity=conn)
        assert e.value.code == ERR_STATE
        # the host variant with an explicit field uploads it: it is the retained field afterwards, with its connectivity
        assert_same(m.ReachPaths(tg, cost=field["cost"], box=box, connectivity=conn, shortcut=True, max_span=8), want[conn], f"explicit, host {conn}")
        assert_same(m.ReachPaths(tg, connectivity=conn, shortcut=True, max_span=8), want[conn], f"retained by the upload {conn}")
        a, res = host_result(len(tg), 0)
        assert raw_call(m, tg, res, conn=32 - conn) == ERR_INVALID


def test_capacity(maze):
    m, conn = maze.m, 26
    maze.flood(conn)
    idx = np.arange(len(maze.targets) - 200, len(maze.targets))
    tg = maze.targets[idx]
    for shortcut, span in ((False, 1), (True, 4096)):
        flags = 1 if shortcut else 0
        want = path_slices(maze.want(conn, shortcut, span), idx)
        total = int(want["offsets"][-1])
        inner = want["offsets"][np.flatnonzero(np.diff(want["offsets"]) >= 3)[3]] + 1     # the middle of a path
        assert 0 < inner < total
        for cap in (0, int(inner), total):
            a, res = host_result(len(tg), total + 7)
            assert raw_call(m, tg, res, conn=conn, flags=flags, span=span, capacity=cap) == 0
            for k in ("offsets", "status", "n_moves"):
                assert np.array_equal(a[k], want[k]), (k, cap)                         # the true totals whatever the capacity
            for k in ("waypoints_vox", "waypoints_pos"):
                assert np.array_equal(a[k][:cap], want[k][:cap]) and (a[k][cap:] == -77).all(), (k, cap)
            d = device_paths(m, tg, conn, shortcut, span, capacity=cap, pad=9)
            for k in ("offsets", "status", "n_moves"):
                assert np.array_equal(d[k], want[k]), (k, cap, "device")
            for k in ("waypoints_vox", "waypoints_pos"):
                assert np.array_equal(d[k][:cap], want[k][:cap]) and (d[k][cap:] == -77).all(), (k, cap, "device")
        # the sizing call may pass no waypoint arrays; positions or voxels alone
        from fiesta_amd._lib import ReachPathsResult
        off = np.full(len(tg) + 1, -77, np.int64)
        assert raw_call(m, tg, ReachPathsResult(off.ctypes.data, None, None, None, None), conn=conn, flags=flags, span=span) == 0
        assert np.array_equal(off, want["offsets"])
        vox = np.full((total, 3), -77, np.int32)
        assert raw_call(m, tg, ReachPathsResult(off.ctypes.data, vox.ctypes.data, None, None, None), conn=conn, flags=flags, span=span, capacity=total) == 0
        assert np.array_equal(vox, want["waypoints_vox"])
        assert m.ReachPaths(tg, connectivity=conn, shortcut=shortcut, max_span=span, want_pos=False)["waypoints_pos"] is None


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 513])
def test_batch_shape(maze, count):
    """raw mode takes a lane per target, shortcut mode a wave: the per-target results do not depend on the batch (257, 513: a second
    and a third trip of the 256 entries the offset scan takes at a time)"""
    m, conn = maze.m, 26
    maze.flood(conn)
    n = len(maze.targets)
    first_ok = 1000 + int(np.flatnonzero(maze.want(conn, False, 1)["status"][1000:] == OK)[0])
    idx = np.arange(first_ok, first_ok + count) if count == 1 else (np.arange(n - count, n) if count < 100 else np.arange(1000, 1000 + count))
    for shortcut, span in ((False, 1), (True, 4096)):
        want = path_slices(maze.want(conn, shortcut, span), idx)
        assert (want["status"] == OK).any()
        assert_same(m.ReachPaths(maze.targets[idx], connectivity=conn, shortcut=shortcut, max_span=span), want, f"{count} targets")
        assert_same(trimmed(device_paths(m, maze.targets[idx], conn, shortcut, span)), want, f"{count} targets, device")
    a, res = host_result(0, 0)
    assert raw_call(m, None, res, n=0, conn=conn) == 0 and a["offsets"].tolist() == [0]


def build_partial():
    """tests/test_gpu_reach.py's partial map: a free box with unobserved blocks -- a slab across x = 10 .. 13, a block in a far corner --
    and a wall at x = 30 whose only door is two voxels wide (y = 18, 19; z = 6 .. 40)"""
    m = new_dense()
    obs = np.ones(SHAPE, bool)
    obs[10:14] = False
    obs[40:, 30:, 50:] = False
    wall = np.zeros(SHAPE, bool)
    wall[30] = True
    wall[30, 18:20, 6:41] = False
    m.SetOccupancy(np.argwhere(obs & ~wall).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, np.argwhere(wall))
    return m, obs, wall


def test_clearance_and_unknown_floods(hip_lib):
    from fiesta_amd import reach_model
    m, obs0, wall = build_partial()
    obs, occ, dist = dump(m, with_dist=True)
    assert np.array_equal(obs, obs0) and np.array_equal(occ, wall)
    rng = np.random.RandomState(7)
    tg = np.concatenate([rng.randint(0, SHAPE, (400, 3)), [(12, 5, 5), (40, 19, 20), (30, 0, 0), (45, 35, 60)]]).astype(np.int32)
    before = m.download_field()
    seen = set()
    for seeds, clr, flags, conn in (([(20, 19, 20)], 0.25, 0, 26), ([(2, 5, 5)], 0.0, THROUGH, 26), ([(20, 19, 20)], 0.25, THROUGH, 6),
                                    ([(20, 19, 20)], 0.0, 0, 6)):
        field = reach_model(obs, occ, seeds, dist, min_clearance=clr, connectivity=conn, flags=flags)
        info = m.ReachField(seeds, min_clearance=clr, connectivity=conn, flags=flags, want_cost=False)
        assert info["n_reached"] == field["n_reached"] > 0
        for shortcut, span in ((False, 1), (True, 4096)):
            want = want_paths(field, tg, conn, shortcut, span)
            assert_same(m.ReachPaths(tg, connectivity=conn, shortcut=shortcut, max_span=span), want, f"partial {clr} {flags} {conn} {shortcut}")
            seen |= set(want["status"].tolist())
    assert seen == {OK, BLOCKED, UNREACHED}
    after = m.download_field()                                            # the call is read-only
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert not m.CheckUpdate()
    m.close()


HASH_SHIFT = np.array((-20, 8, -40), np.int64)      # the maze straddles tile faces and negative coordinates


def test_hash_block_map(hip_lib):
    import fiesta_amd
    from fiesta_amd import reach_model
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=200000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    walls = maze_walls()
    s = HASH_SHIFT
    m.SetOccupancy((all_voxels(SHAPE).astype(np.int64) + s).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, np.argwhere(walls) + s)
    # download_hash scattered into an array that covers the box: what no page holds is unknown
    lo, hi = s - 6, s + np.array(SHAPE) + 5
    h = m.download_hash()
    keep = np.all((h["vox"] >= lo) & (h["vox"] <= hi), axis=1)
    i = tuple((h["vox"][keep] - lo).T)
    obs, occ = np.zeros(tuple(hi - lo + 1), bool), np.zeros(tuple(hi - lo + 1), bool)
    obs[i], occ[i] = h["d2"][keep] >= 0, h["occ"][keep] != 0
    assert obs.sum() == np.prod(SHAPE) and occ.sum() == walls.sum()
    seed = [tuple(int(v) for v in s + (1, 20, 36))]
    rng = np.random.RandomState(3)
    tg = (rng.randint(-8, np.array(SHAPE) + 8, (500, 3)) + s).astype(np.int32)
    for flags, conn in ((0, 26), (THROUGH, 6)):
        field = reach_model(obs, occ, seed, lo=lo, hi=hi, connectivity=conn, flags=flags, origin_vox=lo)
        info = m.ReachField(seed, lo, hi, connectivity=conn, flags=flags, want_cost=False)
        assert info["box_lo"] == field["box_lo"] == [int(v) for v in lo] and info["n_reached"] == field["n_reached"]
        for shortcut, span in ((False, 1), (True, 16), (True, 4096)):
            want = want_paths(field, tg, conn, shortcut, span)
            assert {OK, OUTSIDE, BLOCKED} <= set(want["status"].tolist()) and want["waypoints_vox"].min() < 0
            assert_same(m.ReachPaths(tg, connectivity=conn, shortcut=shortcut, max_span=span), want, f"hash {flags} {conn} {shortcut} {span}")
        assert_same(trimmed(device_paths(m, tg, conn, True, 4096)), want, f"hash, device {conn}")
    m.close()


def test_shard_uses_global_coordinates(hip_lib):
    import fiesta_amd
    from fiesta_amd import reach_model
    gg = (32, 16, 16)
    sh = fiesta_amd.ESDFMap((0, 0, 0), RES, (15.5 * RES,) * 3, shard_lo=(16, 0, 0), global_grid=gg)
    sh.SetParameters(*P_DEFAULT)
    sh.SetOriginalRange()
    sh.SetOccupancyBox((16, 2, 2), (30, 13, 14), 0)
    sh.UpdateOccupancy(True)
    sh.UpdateESDF()
    occupy(sh, [(22, y, z) for y in range(2, 12) for z in range(2, 15)])      # a wall with a gap at y = 12, 13
    info = sh.shard_info()
    org = np.array(info["local_origin"])
    obs, occ, _ = dump(sh, org)
    seeds = [(18, 5, 5)]
    field = reach_model(obs, occ, seeds, origin_vox=org)
    got = sh.ReachField(seeds, want_cost=False)
    assert got["box_lo"] == field["box_lo"] == [int(v) for v in org] and got["n_reached"] == field["n_reached"] > 1000
    tg = np.argwhere(np.ones(tuple(info["local_dims"]), bool))[::7] + org
    for shortcut in (False, True):
        want = want_paths(field, tg, 26, shortcut, 4096)
        assert (want["n_moves"] > 12).any() and want["waypoints_vox"][:, 0].min() >= 16
        assert_same(sh.ReachPaths(tg, shortcut=shortcut), want, f"shard {shortcut}")
    sh.close()


def test_inconsistent_field_is_broken_and_errors_leave_the_map_usable(maze):
    import fiesta_amd
    m, conn = maze.m, 26
    field = maze.field[conn]
    box = (field["box_lo"], field["box_hi"])
    tg = maze.targets[-260:]
    inside = np.all((tg >= BOX[0]) & (tg <= BOX[1]), axis=1)
    sevens = np.full(field["cost"].shape, 7, np.int32)
    for shortcut in (False, True):
        r = m.ReachPaths(tg, cost=sevens, box=box, connectivity=conn, shortcut=shortcut, max_span=64)
        assert (r["status"][inside] == BROKEN).all() and (r["status"][~inside] == OUTSIDE).all() and inside.sum() > 200
        assert (r["offsets"] == 0).all() and (r["n_moves"] == -1).all() and len(r["waypoints_vox"]) == 0
        assert_same(r, want_paths({"cost": sevens, "box_lo": box[0]}, tg, conn, shortcut, 64), "sevens")
    # a field that is right except for one voxel on the way: the paths through it break, the others stand
    dented = field["cost"].copy()
    dented[tuple(np.array((4, 10, 36)) - BOX[0])] += 1
    for shortcut in (False, True):
        want = want_paths({"cost": dented, "box_lo": box[0]}, tg, conn, shortcut, 64)
        assert (want["status"] == BROKEN).any() and (want["status"] == OK).any()
        assert_same(m.ReachPaths(tg, cost=dented, box=box, connectivity=conn, shortcut=shortcut, max_span=64), want, "dented")
    # the next valid call is right
    idx = np.arange(len(maze.targets) - 260, len(maze.targets))
    want = path_slices(maze.want(conn, True, 4096), idx)
    assert_same(m.ReachPaths(tg, cost=field["cost"], box=box, connectivity=conn, shortcut=True, max_span=4096), want, "after the broken fields")
    # whole-call errors: nothing is written, the retained field stays
    a, res = host_result(len(tg), 10)
    from fiesta_amd._lib import ReachPathsResult
    c = np.ascontiguousarray(field["cost"])
    bad = [raw_call(m, tg, None), raw_call(m, tg, ReachPathsResult(None, None, None, None, None)), raw_call(m, tg, res, conn=18),
           raw_call(m, tg, res, flags=2), raw_call(m, tg, res, flags=1, span=0), raw_call(m, tg, res, n=-1), raw_call(m, tg, res, capacity=-1),
           raw_call(m, None, res, n=3), raw_call(m, tg, res, cost=c), raw_call(m, tg, res, lo=box[0], hi=box[1]),
           raw_call(m, tg, res, cost=c, lo=box[1], hi=box[0]), raw_call(m, tg, res, cost=c, lo=(0, 0, 0), hi=(1023, 1023, 256))]
    assert bad == [ERR_INVALID] * len(bad), bad
    assert all((a[k] == -77).all() for k in KEYS)
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.ReachPaths(tg, connectivity=18)
    with pytest.raises(ValueError):
        m.ReachPaths(tg, cost=c)
    assert_same(m.ReachPaths(tg, connectivity=conn, shortcut=True, max_span=4096), want, "after the errors")
    before = m.download_field()
    m.ReachPaths(tg, connectivity=conn)
    after = m.download_field()
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    """examples/reach_path.cpp: the C++ class's ReachPaths and GetPathCost on the scene of examples/reach.cpp, against the Python
    class and the model"""
    import json
    from test_cpp_reach import example_scene
    from fiesta_amd import reach_model
    exe = os.path.join(str(tmp_path), "reach_path")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "reach_path.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    robot = [(12, 20, 10)]
    fv, _ = m.GetFrontierVoxels()
    obs, occ, _ = dump(m)
    field = reach_model(obs, occ, robot, targets=fv)
    tc = field["target_cost"]
    ok = (tc >= 0) & (tc != INF) & (fv[:, 0] > 24)
    cand = fv[ok][tc[ok] == tc[ok].min()]
    goal = sorted(cand.tolist())[0]
    assert out["goal"] == goal and out["goal_cost"] == int(tc[ok].min())
    tg = [goal, (34, 19, 9)]
    from fiesta_amd import reach_paths_model
    raw = reach_paths_model(field["cost"], field["box_lo"], tg, 26, 0, 1, (-4.0, -4.0, 0.0), 0.2)
    tight = reach_paths_model(field["cost"], field["box_lo"], tg, 26, 1, 64, (-4.0, -4.0, 0.0), 0.2)
    assert out["n_moves"] == raw["n_moves"][0] > 5 and out["raw_waypoints"] == raw["offsets"][1] == out["n_moves"] + 1
    assert out["waypoints"] == tight["waypoints_vox"][:tight["offsets"][1]].tolist() and 2 <= len(out["waypoints"]) < out["raw_waypoints"]
    assert out["pocket_status"] == UNREACHED == raw["status"][1] and out["pocket_waypoints"] == 0
    m.ReachField(robot, want_cost=False)
    got = m.ReachPaths(tg, shortcut=True, max_span=64)
    assert_same(got, tight, "example scene")
    pc = m.PathCost(got["waypoints_pos"][:got["offsets"][1]], [0, got["offsets"][1]], 0.1, 0.6)
    assert out["path_cost"] == float(pc["cost"][0])
    m.close()
