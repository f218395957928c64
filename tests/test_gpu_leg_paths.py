"""Leg paths on the GPU (fiesta_hip_leg_paths[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/leg_path_kernels.hpp).

Two oracles, and every comparison is exact equality of every array (offsets, voxels, positions as f64 bits, status, moves, cost):
fiesta_amd.leg_paths_model (tests/test_leg_paths_rule.py holds it to literal properties) fed from the map's own dump through calls
that existed before, and -- sharing no new code -- the route that existed before: per source one ReachField(seeds=[source]) and
ReachPaths on its targets.

The scene is that of tests/test_gpu_reach_matrix.py (40 x 24 x 40 voxels at 0.1 m, the sources of tests/test_reach_matrix_rule.py: a
blocked, an unknown and an outside one, a voxel listed twice, the sealed pair 4 <-> 5); the maze is that of tests/test_gpu_reach.py
(48 x 40 x 72), whose descents between its far ends take more than 256 moves: several windows of 64 voxels.
"""
import ctypes as C

import numpy as np
import pytest

from scenarios import P_DEFAULT
from test_gpu_reach import RES, Model, maze_walls, new_dense, occupy
from test_gpu_reach import SHAPE as MAZE_SHAPE
from test_reach_matrix_rule import SCENE_SHAPE, SOURCES, scene

pytestmark = pytest.mark.gpu
INF = 2 ** 31 - 1
N = len(SOURCES)
OK, OUTSIDE, BLOCKED, UNREACHED, BROKEN, NO_SOURCE, BAD_INDEX = range(7)
ERR_INVALID, ERR_STATE = 1, 4
KEYS = ("offsets", "waypoints_vox", "waypoints_pos", "status", "n_moves", "cost")
INFO = ("box_lo", "box_hi", "connectivity", "n_sources")
MODES = ((False, 4096), (True, 8), (True, 4096))     # (shortcut, max_span)
PAIRS = np.array([(a, b) for a in range(N) for b in range(N)], np.int32)
FILL = -77


def assert_same(got, want, what="", keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        diff = got[k] != want[k]
        bad = np.argwhere(diff.reshape(len(diff), -1).any(1)) if diff.size else np.zeros((0, 1), np.int64)
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} rows, first at {bad[:3].ravel().tolist()}: got " \
                              f"{got[k][bad[:3].ravel()].tolist()} want {want[k][bad[:3].ravel()].tolist()}"


def device_legs(m, fr, to=None, to_vox=None, shortcut=False, span=4096, capacity=None, pad=5):
    """LegPathsDevice with torch tensors: a sizing call unless `capacity` is given; returns numpy arrays (waypoint arrays `pad` rows
    longer than the capacity, filled with FILL) and the info"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(fr)
    fd = torch.tensor(np.ascontiguousarray(fr, np.int32), device=dev)
    td = None if to is None else torch.tensor(np.ascontiguousarray(to, np.int32), device=dev)
    vd = None if to_vox is None else torch.tensor(np.ascontiguousarray(to_vox, np.int32).reshape(-1, 3), device=dev)
    off = torch.full((n + 1,), FILL, dtype=torch.int64, device=dev)
    per = {k: torch.full((n,), FILL, dtype=torch.int32, device=dev) for k in ("status", "n_moves", "cost")}
    torch.cuda.synchronize()
    kw = dict(to_dev_ptr=0 if td is None else td.data_ptr(), to_vox_dev_ptr=0 if vd is None else vd.data_ptr(), shortcut=shortcut, max_span=span)
    if capacity is None:
        m.LegPathsDevice(fd.data_ptr(), n, off.data_ptr(), capacity=0, **kw)
        m.synchronize()
        capacity = int(off.cpu()[n])
    vox = torch.full((capacity + pad, 3), FILL, dtype=torch.int32, device=dev)
    pos = torch.full((capacity + pad, 3), float(FILL), dtype=torch.float64, device=dev)
    off.fill_(FILL)
    torch.cuda.synchronize()
    info = m.LegPathsDevice(fd.data_ptr(), n, off.data_ptr(), capacity=capacity, waypoints_vox_dev_ptr=vox.data_ptr(),
                            waypoints_pos_dev_ptr=pos.data_ptr(), status_dev_ptr=per["status"].data_ptr(), n_moves_dev_ptr=per["n_moves"].data_ptr(),
                            cost_dev_ptr=per["cost"].data_ptr(), **kw)
    m.synchronize()                                                      # (the _dev variant only enqueues on the map's stream)
    out = {"offsets": off.cpu().numpy(), "waypoints_vox": vox.cpu().numpy(), "waypoints_pos": pos.cpu().numpy()}
    out.update({k: v.cpu().numpy() for k, v in per.items()}, **info)
    return out


def trimmed(r, pad=5):
    out = dict(r)
    total = int(r["offsets"][-1])
    for k in ("waypoints_vox", "waypoints_pos"):
        assert len(r[k]) == total + pad and (r[k][total:] == FILL).all(), k
        out[k] = r[k][:total]
    return out


def legs_model(model, sources, fr, to=None, to_vox=None, lo=None, hi=None, clearance=0.0, conn=26, flags=0, shortcut=False, span=4096):
    """leg_paths_model on the map's own dump; the floods are kept per batch (the tests share them and leave them unchanged)"""
    from fiesta_amd import leg_paths_model
    key = ("floods", np.asarray(sources).tobytes(), None if lo is None else tuple(int(v) for v in lo), None if hi is None else tuple(int(v) for v in hi),
           clearance, conn, flags)
    floods = model.memo.setdefault(key, {})
    return leg_paths_model(model.obs, model.occ, sources, fr, to, to_vox, model.dist, lo, hi, clearance, conn, flags, 1 if shortcut else 0, span,
                           model.origin, (0.0, 0.0, 0.0), RES, floods)


def old_route(m, sources, status, fr, targets, shortcut, span, **flood):
    """the route that existed before: one ReachField per source, ReachPaths on the targets of its legs; NO_SOURCE where the matrix
    call said the source is not OK (reach_field would flood nothing from it)"""
    fr, targets = np.asarray(fr), np.asarray(targets, np.int32).reshape(-1, 3)
    n = len(fr)
    out = {"status": np.full(n, NO_SOURCE, np.int32), "n_moves": np.full(n, -1, np.int32), "cost": np.full(n, -1, np.int32)}
    paths = [(np.zeros((0, 3), np.int32), np.zeros((0, 3)))] * n
    for s in sorted(set(fr.tolist())):
        if status[s] != 0:
            continue
        k = np.flatnonzero(fr == s)
        out["cost"][k] = m.ReachField([sources[s]], targets=targets[k], want_cost=False, **flood)["target_cost"]
        r = m.ReachPaths(targets[k], connectivity=flood.get("connectivity", 26), shortcut=shortcut, max_span=span)
        out["status"][k], out["n_moves"][k] = r["status"], r["n_moves"]
        for j, leg in enumerate(k):
            paths[leg] = (r["waypoints_vox"][r["offsets"][j]:r["offsets"][j + 1]], r["waypoints_pos"][r["offsets"][j]:r["offsets"][j + 1]])
    out["offsets"] = np.concatenate([[0], np.cumsum([len(p[0]) for p in paths])]).astype(np.int64)
    out["waypoints_vox"] = np.concatenate([p[0] for p in paths] + [np.zeros((0, 3), np.int32)]).astype(np.int32)
    out["waypoints_pos"] = np.concatenate([p[1] for p in paths] + [np.zeros((0, 3))]).astype(np.float64)
    return out


@pytest.fixture(scope="module")
def scene_map(hip_lib):
    m = new_dense(SCENE_SHAPE)
    obs, occ = scene()
    m.SetOccupancy(np.argwhere(obs & ~occ).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, np.argwhere(occ))
    model = Model.dense(m)
    assert np.array_equal(model.obs, obs) and np.array_equal(model.occ, occ)
    yield m, model
    m.close()


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("flags", [0, 1])
def test_scene_all_pairs(scene_map, conn, flags):
    m, model = scene_map
    fr, to = PAIRS[:, 0], PAIRS[:, 1]
    seen = set()
    for shortcut, span in MODES:
        mx = m.ReachMatrix(SOURCES, connectivity=conn, flags=flags)       # (the old route below floods in between: it changes nothing)
        assert mx["batches"] == 1
        want = legs_model(model, SOURCES, fr, to, conn=conn, flags=flags, shortcut=shortcut, span=span)
        got = m.LegPaths(fr, to=to, shortcut=shortcut, max_span=span)
        what = f"scene {conn} {flags} {shortcut} {span}"
        assert_same(got, want, what + ", host")
        assert all(got[k] == want[k] for k in INFO), (what, [got[k] for k in INFO])
        dev = device_legs(m, fr, to=to, shortcut=shortcut, span=span)
        assert_same(trimmed(dev), want, what + ", device")
        assert all(dev[k] == want[k] for k in INFO)
        # the cost column is the matrix entry, bit for bit
        assert np.array_equal(got["cost"], mx["cost"][fr, to])
        # ... and the voxels of the sites as to_vox give the same legs
        tv = np.array(SOURCES, np.int32)[to]
        assert_same(m.LegPaths(fr, to_vox=tv, shortcut=shortcut, max_span=span), want, what + ", to_vox")
        # independently: the route that existed before, one flood per source
        old = old_route(m, SOURCES, mx["source_status"], fr, tv, shortcut, span, connectivity=conn, flags=flags)
        assert_same(got, old, what + ", one flood per leg's source")
        # (the floods of the old route are reach_field's: the retained batch is still there)
        assert_same(m.LegPaths(fr, to=to, shortcut=shortcut, max_span=span), want, what + ", after the floods")
        seen |= set(got["status"].tolist())
        print(f"{what}: {got['offsets'][-1]} waypoints in {int((got['status'] == OK).sum())} legs, longest {got['n_moves'].max()} moves")
    assert seen == {OK, OUTSIDE, BLOCKED, UNREACHED, NO_SOURCE}
    bad = m.LegPaths([-1, N, 0, 0, 3], to=[0, 0, -1, N, N])
    assert bad["status"].tolist() == [BAD_INDEX] * 5 and (bad["cost"] == -1).all() and (bad["n_moves"] == -1).all() and bad["offsets"][-1] == 0
    assert_same(bad, legs_model(model, SOURCES, [-1, N, 0, 0, 3], [0, 0, -1, N, N], conn=conn, flags=flags), "bad indices")


def test_tour_legs(scene_map):
    """the legs of a tour are views into its order; their costs are the tour's leg costs; TourRoute is the three calls"""
    m, model = scene_map
    for closed in (False, True):
        mx = m.ReachMatrix(SOURCES)
        tour = m.SiteTour(mx["cost"], start=0, closed=closed, restarts=8)
        k = tour["n_visited"]
        order = tour["order"]
        assert 3 < k < N and (order[k:] == -1).all()
        legs = m.LegPaths(order[:k - 1], to=order[1:k], shortcut=True)
        assert (legs["status"] == OK).all() and np.array_equal(legs["cost"], tour["leg_cost"][1:k])
        assert_same(legs, legs_model(model, SOURCES, order[:k - 1], order[1:k], shortcut=True), f"tour, closed {closed}")
        # consecutive legs concatenate: the last waypoint of one is the first of the next, site by site
        first, last = legs["waypoints_vox"][legs["offsets"][:-1]], legs["waypoints_vox"][legs["offsets"][1:] - 1]
        assert np.array_equal(first, np.array(SOURCES, np.int32)[order[:k - 1]]) and np.array_equal(last, np.array(SOURCES, np.int32)[order[1:k]])
        route = m.TourRoute(SOURCES, start=0, closed=closed, restarts=8, shortcut=True)
        assert np.array_equal(route["order"], order) and np.array_equal(route["matrix"], mx["cost"])
        n_legs = k if closed else k - 1
        assert len(route["legs"]["from"]) == n_legs and np.array_equal(route["legs"]["from"][:k - 1], order[:k - 1])
        head = {key: (route["legs"][key][:legs["offsets"][-1]] if key.startswith("way") else route["legs"][key][:k - 1 + (key == "offsets")]) for key in KEYS}
        assert_same(head, legs, f"TourRoute, closed {closed}")
        if closed:
            assert route["legs"]["from"][-1] == order[k - 1] and route["legs"]["to"][-1] == order[0] == 0
            assert route["legs"]["cost"][-1] == tour["leg_cost"][0] and route["legs"]["status"][-1] == OK
            assert tuple(route["legs"]["waypoints_vox"][-1]) == SOURCES[0]
        assert int(route["legs"]["cost"].astype(np.int64).sum()) == tour["length"]


@pytest.fixture(scope="module")
def maze(hip_lib):
    m = new_dense()
    m.SetOccupancyBox((0, 0, 0), tuple(s - 1 for s in MAZE_SHAPE), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    walls = maze_walls()
    occupy(m, np.argwhere(walls))
    model = Model.dense(m, with_dist=False)
    assert model.obs.all() and np.array_equal(model.occ, walls)
    yield m, model
    m.close()


ENDS = [(1, 20, 36), (46, 20, 5), (25, 38, 70)]     # the maze's two far ends and a site half way


def test_maze_long_descents_and_batch_shapes(maze):
    m, model = maze
    conn = 6
    pairs = [(0, 1), (1, 0), (0, 2), (2, 1), (1, 1)]
    for shortcut, span in ((False, 4096), (True, 4096)):
        mx = m.ReachMatrix(ENDS, connectivity=conn)
        assert mx["batches"] == 1 and mx["fields"] == 3
        fr, to = [p[0] for p in pairs], [p[1] for p in pairs]
        want = legs_model(model, ENDS, fr, to, conn=conn, shortcut=shortcut, span=span)
        assert want["n_moves"][0] > 256 and want["n_moves"][4] == 0 and (want["status"] == OK).all()
        assert_same(m.LegPaths(fr, to=to, shortcut=shortcut, max_span=span), want, f"maze {shortcut}")
        assert_same(trimmed(device_legs(m, fr, to=to, shortcut=shortcut, span=span)), want, f"maze {shortcut}, device")
        old = old_route(m, ENDS, mx["source_status"], fr, np.array(ENDS, np.int32)[to], shortcut, span, connectivity=conn)
        assert_same(want, old, f"maze {shortcut}, one flood per source")
        per = [(want["waypoints_vox"][want["offsets"][j]:want["offsets"][j + 1]], want["waypoints_pos"][want["offsets"][j]:want["offsets"][j + 1]])
               for j in range(len(pairs))]
        # batches of 1, 63, 64, 65 and 257 legs (the pairs repeated): a leg does not depend on its batch
        for count in (1, 63, 64, 65, 257):
            idx = np.arange(count) % len(pairs)
            big = {"status": want["status"][idx], "n_moves": want["n_moves"][idx], "cost": want["cost"][idx],
                   "offsets": np.concatenate([[0], np.cumsum([len(per[j][0]) for j in idx])]).astype(np.int64),
                   "waypoints_vox": np.concatenate([per[j][0] for j in idx]), "waypoints_pos": np.concatenate([per[j][1] for j in idx])}
            f2, t2 = np.array(fr, np.int32)[idx], np.array(to, np.int32)[idx]
            assert_same(m.LegPaths(f2, to=t2, shortcut=shortcut, max_span=span), big, f"{count} legs")
            assert_same(trimmed(device_legs(m, f2, to=t2, shortcut=shortcut, span=span)), big, f"{count} legs, device")


def host_result(n, cap):
    from fiesta_amd._lib import LegPathsResult
    a = {"offsets": np.full(n + 1, FILL, np.int64), "waypoints_vox": np.full((cap, 3), FILL, np.int32), "waypoints_pos": np.full((cap, 3), float(FILL)),
         "status": np.full(n, FILL, np.int32), "n_moves": np.full(n, FILL, np.int32), "cost": np.full(n, FILL, np.int32)}
    return a, LegPathsResult(*[a[k].ctypes.data for k in KEYS])


def raw_call(m, fr, to, res, flags=0, span=1, capacity=0, info=None):
    from fiesta_amd.esdf_map import _p
    f, t = np.ascontiguousarray(fr, np.int32), np.ascontiguousarray(to, np.int32)
    return m._lib.fiesta_hip_leg_paths(m._h, _p(f), _p(t), None, len(f), flags, span, capacity, C.byref(res), None if info is None else C.byref(info))


def test_capacity(scene_map):
    m, model = scene_map
    m.ReachMatrix(SOURCES)
    fr, to = PAIRS[:, 0], PAIRS[:, 1]
    for shortcut, span in ((False, 1), (True, 4096)):
        want = legs_model(model, SOURCES, fr, to, shortcut=shortcut, span=span)
        total = int(want["offsets"][-1])
        inner = int(want["offsets"][np.flatnonzero(np.diff(want["offsets"]) >= 3)[3]] + 1)      # the middle of a leg
        assert 0 < inner < total
        for cap in (0, inner, total):
            a, res = host_result(len(fr), total + 7)
            assert raw_call(m, fr, to, res, flags=1 if shortcut else 0, span=span, capacity=cap) == 0
            d = device_legs(m, fr, to=to, shortcut=shortcut, span=span, capacity=cap, pad=9)
            for r, who in ((a, "host"), (d, "device")):
                for k in ("offsets", "status", "n_moves", "cost"):
                    assert np.array_equal(r[k], want[k]), (k, cap, who)             # the true totals whatever the capacity
                for k in ("waypoints_vox", "waypoints_pos"):                        # canaries after the last permitted entry
                    assert np.array_equal(r[k][:cap], want[k][:cap]) and (r[k][cap:] == FILL).all(), (k, cap, who)
    # the sizing call may pass nothing but offsets
    from fiesta_amd._lib import LegPathsResult
    off = np.full(len(fr) + 1, FILL, np.int64)
    assert raw_call(m, fr, to, LegPathsResult(off.ctypes.data, None, None, None, None, None), flags=1, span=4096) == 0
    assert np.array_equal(off, want["offsets"])
    assert m.LegPaths(fr, to=to, want_pos=False)["waypoints_pos"] is None


def test_retention(scene_map, hip_lib):
    import fiesta_amd
    from fiesta_amd._lib import LegPathsInfo, ReachMatrixResult
    m, model = scene_map
    fr, to = PAIRS[:, 0], PAIRS[:, 1]
    want = legs_model(model, SOURCES, fr, to, shortcut=True)

    def refused(mm, word):
        with pytest.raises(fiesta_amd.FiestaHipError) as e:
            mm.LegPaths([0], to=[0])
        assert e.value.code == ERR_STATE and word in str(e.value), str(e.value)
        a, res = host_result(1, 1)
        info = LegPathsInfo()
        info.n_sources = -5
        assert raw_call(mm, [0], [0], res, info=info) == ERR_STATE
        assert all((a[k] == FILL).all() for k in KEYS) and info.n_sources == -5                 # nothing is written
    # no matrix call yet
    fresh = new_dense((8, 8, 8))
    refused(fresh, "no reach_matrix call yet")
    fresh.close()
    # more sources than one batch holds; an empty box; no source
    assert m.ReachMatrix(SOURCES, max_fields=4)["batches"] == 3
    refused(m, "more than one batch")
    m.ReachMatrix(SOURCES, lo=(5, 5, 5), hi=(4, 9, 9))
    refused(m, "empty box")
    m.ReachMatrix(np.zeros((0, 3), np.int32))
    refused(m, "no source")
    # one batch again: retained; a matrix call refused by its argument checks leaves the batch usable
    assert m.ReachMatrix(SOURCES, max_fields=11)["batches"] == 1
    assert_same(m.LegPaths(fr, to=to, shortcut=True), want, "retained")
    src = np.ascontiguousarray(SOURCES, np.int32)
    res = ReachMatrixResult(None, None, None)
    assert m._lib.fiesta_hip_reach_matrix(m._h, None, None, src.ctypes.data_as(C.c_void_p), N, None, 0, 0.0, 18, 0, 0, C.byref(res), None) == ERR_INVALID
    assert m._lib.fiesta_hip_reach_matrix(m._h, None, None, src.ctypes.data_as(C.c_void_p), N, None, 0, 0.0, 26, 0, -1, C.byref(res), None) == ERR_INVALID
    assert_same(m.LegPaths(fr, to=to, shortcut=True), want, "after the refused matrix calls")
    # an interleaved ReachField / ReachPaths pair changes nothing, in either direction
    m.ReachField([SOURCES[1]], want_cost=False)
    before = m.ReachPaths(np.array(SOURCES, np.int32), shortcut=True)
    assert_same(m.LegPaths(fr, to=to, shortcut=True), want, "after a reach_field / reach_paths pair")
    after = m.ReachPaths(np.array(SOURCES, np.int32), shortcut=True)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a snapshot: a wall across the free space and an UpdateESDF after the matrix call change no output
    scratch = new_dense(SCENE_SHAPE)
    obs, occ = scene()
    scratch.SetOccupancy(np.argwhere(obs & ~occ).astype(np.int32), 0, want_ret=False)
    scratch.UpdateOccupancy(True)
    scratch.UpdateESDF()
    occupy(scratch, np.argwhere(occ))
    scratch.ReachMatrix(SOURCES)
    occupy(scratch, [(3, y, z) for y in range(24) for z in range(40)])
    assert_same(scratch.LegPaths(fr, to=to, shortcut=True), want, "snapshot")
    assert scratch.ReachMatrix(SOURCES)["cost"][0, 1] == INF              # (the map did change: the wall cuts source 0 off)
    scratch.close()
    # a second matrix call with other sources replaces the batch
    other = [SOURCES[9], SOURCES[1], SOURCES[0]]
    m.ReachMatrix(other, connectivity=6)
    got = m.LegPaths([0, 1, 2, 3], to=[1, 2, 0, 0])
    assert_same(got, legs_model(model, other, [0, 1, 2, 3], [1, 2, 0, 0], conn=6), "replaced")
    assert got["n_sources"] == 3 and got["connectivity"] == 6 and got["status"].tolist() == [OK, OK, OK, BAD_INDEX]
    # no legs: offsets[0] = 0 and the info
    none = m.LegPaths([], to=[])
    assert none["offsets"].tolist() == [0] and none["n_sources"] == 3 and none["box_hi"] == [39, 23, 39] and len(none["waypoints_vox"]) == 0
    dev = device_legs(m, np.zeros(0, np.int32), to=np.zeros(0, np.int32))
    assert dev["offsets"].tolist() == [0] and dev["n_sources"] == 3


def test_rectangular_form_retains_too(scene_map):
    m, model = scene_map
    lo, hi = (3, 2, 5), (37, 21, 36)
    cols, _ = m.GetFrontierVoxels()
    # ... and a voxel of the corridor of sources 9 and 10, one outside the array, a wall, one outside the box
    cols = np.concatenate([cols[::29], [(15, 12, 20), (50, 0, 0), (6, 12, 20), (2, 12, 20)]]).astype(np.int32)
    mx = m.ReachMatrix(SOURCES, targets=cols, lo=lo, hi=hi, min_clearance=0.25)
    assert mx["batches"] == 1 and mx["cost"].shape == (N, len(cols))
    fr = np.repeat(np.arange(N, dtype=np.int32), len(cols))
    tv = np.tile(cols, (N, 1))
    for shortcut, span in ((False, 1), (True, 4096)):
        want = legs_model(model, SOURCES, fr, to_vox=tv, lo=lo, hi=hi, clearance=0.25, shortcut=shortcut, span=span)
        got = m.LegPaths(fr, to_vox=tv, shortcut=shortcut, max_span=span)
        assert_same(got, want, f"columns {shortcut}")
        assert_same(trimmed(device_legs(m, fr, to_vox=tv, shortcut=shortcut, span=span)), want, f"columns {shortcut}, device")
        assert np.array_equal(got["cost"].reshape(N, len(cols)), mx["cost"]) and got["box_lo"] == list(lo) and got["box_hi"] == list(hi)
    assert {OK, OUTSIDE, BLOCKED, NO_SOURCE} <= set(got["status"].tolist())


HASH_SHIFT = np.array((-20, 8, -40), np.int64)      # the scene straddles tile faces and negative coordinates


def test_hash_block_map(hip_lib):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=200000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    obs, occ = scene()
    s = HASH_SHIFT
    m.SetOccupancy((np.argwhere(obs & ~occ) + s).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, np.argwhere(occ) + s)
    src = (np.array(SOURCES, np.int64) + s).astype(np.int32)
    top = s + np.array(SCENE_SHAPE)
    wide = Model.hashed(m, s - 2, top + 1)
    mx = m.ReachMatrix(src, lo=s, hi=top - 1)
    assert mx["batches"] == 1
    fr, to = PAIRS[:, 0], PAIRS[:, 1]
    want = legs_model(wide, src, fr, to, lo=s, hi=top - 1, shortcut=True)
    assert want["waypoints_vox"].min() < 0 and (want["status"] == OK).sum() > 30
    assert_same(m.LegPaths(fr, to=to, shortcut=True), want, "hash")
    assert_same(trimmed(device_legs(m, fr, to=to, shortcut=True)), want, "hash, device")
    m.close()


def small_map(kind, walls):
    """a 16^3 scene, all observed, `walls` occupied, on either store"""
    import fiesta_amd
    if kind == "dense":
        m = new_dense((16, 16, 16))
    else:
        m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=200000, mode="hash")
        m.SetParameters(*P_DEFAULT)
        m.SetOriginalRange()
    m.SetOccupancy(np.argwhere(~walls).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, np.argwhere(walls))
    return m


def same_bits(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)
        else:
            assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("kinds", [("dense", "hash"), ("hash", "dense")])
def test_retained_floods_belong_to_their_map(hip_lib, kinds):
    """Leg paths, reach paths, clusters, cluster splitting and the site tour are one function each for both stores, which reaches a
    map's scratch through a reference: what a map retained -- the reach matrix's batch, the reach field's cost field -- is still its
    own after another map, of the other store and alive at the same time, ran every such call on other sites in another box."""
    wall_a = np.zeros((16, 16, 16), bool)
    wall_a[8, 3:] = True                                     # a wall across x with a gap at low y
    wall_b = np.zeros((16, 16, 16), bool)
    wall_b[:, 6, :12] = True                                 # a wall across y with a gap at high z
    a, b = small_map(kinds[0], wall_a), small_map(kinds[1], wall_b)
    sites_a, box_a = [(2, 2, 2), (13, 13, 13), (2, 13, 8), (13, 2, 8)], ((0, 0, 0), (15, 15, 15))
    sites_b, box_b = [(1, 1, 1), (14, 14, 1), (5, 10, 14), (10, 1, 7)], ((1, 0, 0), (15, 14, 15))
    fr, to = [0, 1, 2, 3, 0], [1, 2, 3, 0, 2]
    targets = np.array([(13, 13, 13), (2, 13, 8), (9, 15, 0), (8, 8, 8)], np.int32)      # (the last one is a wall voxel)
    # map a: the floods, and what the calls read out of them
    assert a.ReachMatrix(sites_a, lo=box_a[0], hi=box_a[1], max_fields=4)["batches"] == 1
    legs = a.LegPaths(fr, to=to, shortcut=True)
    assert (legs["status"] == OK).all() and (np.diff(legs["offsets"]) >= 2).all()
    a.ReachField([sites_a[0]], lo=box_a[0], hi=box_a[1], want_cost=False)
    paths = a.ReachPaths(targets, shortcut=True)
    assert paths["status"].tolist() == [OK, OK, OK, BLOCKED] and paths["offsets"][-1] >= 6
    # map b: every call of the shared unit, and the floods that fill what they read
    mx = b.ReachMatrix(sites_b, lo=box_b[0], hi=box_b[1], max_fields=4)
    assert mx["batches"] == 1
    b.ReachField([sites_b[1]], lo=box_b[0], hi=box_b[1], want_cost=False)
    blobs = np.concatenate([np.argwhere(np.ones((4, 4, 4), bool)) + 1, np.argwhere(np.ones((4, 4, 4), bool)) + 10]).astype(np.int32)
    cl = b.ClusterVoxels(blobs)
    assert cl["size"].tolist() == [64, 64]
    assert b.SplitClusters(blobs, cl["offsets"], cl["members"], max_size=16)["n_parts"] == 8
    assert b.SiteTour(mx["cost"], start=0, restarts=4)["n_visited"] == 4
    legs_b, paths_b = b.LegPaths(fr, to=to, shortcut=True), b.ReachPaths(targets, shortcut=True)
    assert legs_b["waypoints_vox"].tobytes() != legs["waypoints_vox"].tobytes() and paths_b["status"].tolist() != paths["status"].tolist()
    # map a again, no new flood: the same bits
    same_bits(a.LegPaths(fr, to=to, shortcut=True), legs, f"leg paths on the {kinds[0]} map after the {kinds[1]} map's calls")
    same_bits(a.ReachPaths(targets, shortcut=True), paths, f"reach paths on the {kinds[0]} map after the {kinds[1]} map's calls")
    a.close()
    b.close()


def test_whole_chain_on_the_device(scene_map):
    """ReachMatrixDevice -> SiteTourDevice -> LegPathsDevice (from / to: views into the order array) -> PathCorridorDevice, against the
    same chain through the host calls"""
    import torch
    m, _ = scene_map
    dev = torch.device("cuda", 0)
    # the host chain
    mx = m.ReachMatrix(SOURCES)
    tour = m.SiteTour(mx["cost"], start=0, restarts=8)
    k = tour["n_visited"]
    legs = m.LegPaths(tour["order"][:k - 1], to=tour["order"][1:k], shortcut=True)
    corr = m.PathCorridor(legs["waypoints_vox"], legs["offsets"], max_grow=6)
    # the device chain: nothing but counts comes back
    sd = torch.tensor(SOURCES, dtype=torch.int32, device=dev)
    cost = torch.full((N * N,), FILL, dtype=torch.int32, device=dev)
    order = torch.full((N,), FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert m.ReachMatrixDevice(sd.data_ptr(), N, cost_dev_ptr=cost.data_ptr())["batches"] == 1
    assert m.SiteTourDevice(cost.data_ptr(), N, N, start=0, restarts=8, order_dev_ptr=order.data_ptr())["n_visited"] == k
    n_legs = k - 1
    off = torch.full((n_legs + 1,), FILL, dtype=torch.int64, device=dev)
    m.LegPathsDevice(order.data_ptr(), n_legs, off.data_ptr(), to_dev_ptr=order.data_ptr() + 4, shortcut=True)
    m.synchronize()
    total = int(off.cpu()[-1])
    assert total == legs["offsets"][-1]
    vox = torch.full((total, 3), FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.LegPathsDevice(order.data_ptr(), n_legs, off.data_ptr(), to_dev_ptr=order.data_ptr() + 4, shortcut=True, capacity=total,
                     waypoints_vox_dev_ptr=vox.data_ptr())
    coff = torch.full((n_legs + 1,), FILL, dtype=torch.int64, device=dev)
    cst = torch.full((n_legs,), FILL, dtype=torch.int32, device=dev)
    m.PathCorridorDevice(vox.data_ptr(), total, off.data_ptr(), n_legs, coff.data_ptr(), max_grow=6, status_dev_ptr=cst.data_ptr())
    m.synchronize()
    n_boxes = int(coff.cpu()[-1])
    boxes = torch.full((n_boxes, 6), FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    m.PathCorridorDevice(vox.data_ptr(), total, off.data_ptr(), n_legs, coff.data_ptr(), max_grow=6, capacity=n_boxes, boxes_dev_ptr=boxes.data_ptr())
    m.synchronize()
    assert np.array_equal(order.cpu().numpy(), tour["order"]) and np.array_equal(off.cpu().numpy(), legs["offsets"])
    assert np.array_equal(vox.cpu().numpy(), legs["waypoints_vox"])
    assert np.array_equal(coff.cpu().numpy(), corr["offsets"]) and np.array_equal(cst.cpu().numpy(), corr["status"])
    assert np.array_equal(boxes.cpu().numpy(), corr["boxes"]) and n_boxes >= n_legs > 3
