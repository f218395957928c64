"""The reach matrix on the GPU (fiesta_hip_reach_matrix[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/reach_matrix_kernels.hpp).

The expected matrix is always fiesta_amd.reach_matrix_model (one reach_model flood per usable source; tests/test_reach_matrix_rule.py
holds it to that) fed from what the map itself reports through calls that existed before -- download_field / download_hash and
GetDistance -- never from the call under test; and, row by row, the single-source ReachField call.  Costs are integers and the
fixed point is unique: every comparison is exact equality of whole arrays, no tolerance, no excluded entry.

The scene is 40 x 24 x 40 voxels at 0.1 m: a 3 x 2 x 2 grid of reach tiles (16 x 16 x 32) with a short last z-word.
"""
import ctypes as C

import numpy as np
import pytest

from scenarios import P_DEFAULT, all_voxels
from test_gpu_reach import RES, Model, maze_walls, new_dense, occupy
from test_gpu_reach import SHAPE as MAZE_SHAPE
from test_reach_matrix_rule import SCENE_SHAPE, SOURCES, expected_status, scene

pytestmark = pytest.mark.gpu
INF = 2 ** 31 - 1
INFO_KEYS = ("box_lo", "box_hi", "n_traversable", "n_sources_used")
ARRAYS = ("cost", "source_status", "source_reached")


def matrix_model(model, sources, targets=None, lo=None, hi=None, clearance=0.0, conn=26, flags=0):
    """reach_matrix_model on the map's own dump; results are kept (the tests share them and leave them unchanged)"""
    from fiesta_amd import reach_matrix_model
    key = ("matrix", np.asarray(sources).tobytes(), None if targets is None else np.asarray(targets).tobytes(),
           None if lo is None else tuple(int(v) for v in lo), None if hi is None else tuple(int(v) for v in hi), clearance, conn, flags)
    if key not in model.memo:
        model.memo[key] = reach_matrix_model(model.obs, model.occ, sources, targets, model.dist, lo, hi, clearance, conn, flags, model.origin)
    return model.memo[key]


def assert_same(got, want, what=""):
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {len(bad)} entries of {k} differ, first at {bad[:3].tolist()}: got " \
                              f"{[int(got[k][tuple(b)]) for b in bad[:3]]} want {[int(want[k][tuple(b)]) for b in bad[:3]]}"
    for k in INFO_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])


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
def test_scene_whole_array(scene_map, conn, flags):
    m, model = scene_map
    want = matrix_model(model, SOURCES, conn=conn, flags=flags)
    got = m.ReachMatrix(SOURCES, connectivity=conn, flags=flags)
    print(f"scene, connectivity {conn}, flags {flags}: {got['fields']} fields, {got['batches']} batches, {got['rounds']} rounds, "
          f"{got['tile_visits']} tile visits")
    assert_same(got, want, f"scene {conn} {flags}")
    assert got["source_status"].tolist() == expected_status(flags)
    assert np.array_equal(got["cost"], got["cost"].T)
    assert got["box_lo"] == [0, 0, 0] and got["box_hi"] == [39, 23, 39] and got["fields"] == 11 and got["batches"] == 1
    assert 0 < got["rounds"] <= got["tile_visits"] <= got["rounds"] * 12 * 11


def test_clipped_box_with_clearance(scene_map):
    m, model = scene_map
    lo, hi = (3, 2, 5), (37, 21, 36)
    want = matrix_model(model, SOURCES, lo=lo, hi=hi, clearance=0.25)
    got = m.ReachMatrix(SOURCES, lo=lo, hi=hi, min_clearance=0.25)
    assert_same(got, want, "clipped box, clearance 0.25")
    assert [got["source_status"][s] for s in (0, 1, 2, 7, 8)] == [1] * 5 and (got["source_status"] == 0).any()
    assert got["n_traversable"] < matrix_model(model, SOURCES, lo=lo, hi=hi)["n_traversable"]       # the clearance bites


def test_batch_width_changes_nothing(scene_map):
    m, model = scene_map
    want = matrix_model(model, SOURCES)
    for B in (1, 2, 3, 4, 11, 0):
        got = m.ReachMatrix(SOURCES, max_fields=B)
        assert_same(got, want, f"max_fields {B}")
        if B > 0:
            assert got["batches"] == -(-11 // B) and got["fields"] == min(B, 11), (B, got["batches"], got["fields"])
        else:
            assert got["batches"] == 1 and got["fields"] == 11


def test_rectangular_form(scene_map):
    m, model = scene_map
    cols, _ = m.GetFrontierVoxels()
    assert len(cols) > 100
    want = matrix_model(model, SOURCES, targets=cols)
    got = m.ReachMatrix(SOURCES, targets=cols, max_fields=4)
    assert got["cost"].shape == (11, len(cols))
    assert_same(got, want, "frontier voxels as columns")
    for s in np.flatnonzero(got["source_status"] == 0):
        assert np.array_equal(got["cost"][s], m.ReachField([SOURCES[s]], targets=cols, want_cost=False)["target_cost"]), s
    assert (got["cost"][0] >= 0).all() and (got["cost"][0] < INF).any()


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


def test_maze_in_batches(maze):
    m, model = maze
    free = np.argwhere(~model.occ)
    src = free[np.random.RandomState(7).choice(len(free), 32, replace=False)].astype(np.int32)
    src = np.concatenate([src, np.array([(6, 20, 36)], np.int32)])              # ... and one wall voxel
    got = m.ReachMatrix(src, max_fields=8)
    assert got["batches"] == 5 and got["fields"] == 8 and got["n_sources_used"] == 32
    single_rounds = 0
    for s in range(33):
        r = m.ReachField(src[s:s + 1], targets=src, want_cost=False)
        single_rounds += r["rounds"]
        if s < 32:
            assert np.array_equal(got["cost"][s], r["target_cost"]), s
            assert got["source_reached"][s] == r["n_reached"] == got["n_traversable"]
    assert (got["cost"][32] == -1).all() and got["source_status"].tolist() == [0] * 32 + [2] and got["source_reached"][32] == 0
    assert np.array_equal(got["cost"], got["cost"].T)
    for s in (0, 13, 31):
        assert np.array_equal(got["cost"][s], model(src[s:s + 1], targets=src)["target_cost"]), s
    print(f"maze: {got['rounds']} rounds in 5 batches against {single_rounds} in 33 single calls; {got['tile_visits']} tile visits")
    assert 0 < got["rounds"] < single_rounds


def test_device_variant(scene_map):
    import torch
    m, _ = scene_map
    dev = torch.device("cuda", 0)
    cols = np.array([(1, 1, 1), (38, 22, 38), (6, 12, 20), (50, 0, 0), (33, 11, 11)], np.int32)
    for targets in (None, cols):
        host = m.ReachMatrix(SOURCES, targets=targets, connectivity=6)
        n, nc = host["cost"].shape
        cost = torch.full((n * nc + 16,), -99, dtype=torch.int32, device=dev)
        status = torch.full((n + 4,), -99, dtype=torch.int32, device=dev)
        reached = torch.full((n + 4,), -99, dtype=torch.int64, device=dev)
        sd = torch.tensor(SOURCES, dtype=torch.int32, device=dev)
        td = None if targets is None else torch.tensor(cols, device=dev)
        torch.cuda.synchronize()
        info = m.ReachMatrixDevice(sd.data_ptr(), n, 0 if td is None else td.data_ptr(), 0 if td is None else len(cols), connectivity=6,
                                   max_fields=3, cost_dev_ptr=cost.data_ptr(), source_status_dev_ptr=status.data_ptr(),
                                   source_reached_dev_ptr=reached.data_ptr())
        c, s, r = cost.cpu().numpy(), status.cpu().numpy(), reached.cpu().numpy()   # (the call has synchronised with the map's stream)
        assert np.array_equal(c[:n * nc].reshape(n, nc), host["cost"]) and (c[n * nc:] == -99).all()
        assert (c[:n * nc] != -99).all()
        assert np.array_equal(s[:n], host["source_status"]) and (s[n:] == -99).all()
        assert np.array_equal(r[:n], host["source_reached"]) and (r[n:] == -99).all()
        assert all(info[k] == host[k] for k in INFO_KEYS) and info["batches"] == 4 and info["fields"] == 3
    # no output at all: the info alone
    info = m.ReachMatrixDevice(sd.data_ptr(), n, connectivity=6)
    assert all(info[k] == host[k] for k in INFO_KEYS) and info["rounds"] > 0


HASH_SHIFT = np.array((-20, 8, -40), np.int64)      # the scene straddles tile faces and negative coordinates


def raw_call(m, lo, hi, sources, n_sources=None, targets=None, n_targets=None, clearance=0.0, conn=26, flags=0, max_fields=0, res=None, info=None,
             dev=False):
    """the C call itself; returns the status"""
    from fiesta_amd.esdf_map import _p
    blo = None if lo is None else np.ascontiguousarray(lo, np.int32)
    bhi = None if hi is None else np.ascontiguousarray(hi, np.int32)
    s = None if sources is None else np.ascontiguousarray(sources, np.int32).reshape(-1, 3)
    t = None if targets is None else np.ascontiguousarray(targets, np.int32).reshape(-1, 3)
    fn = m._lib.fiesta_hip_reach_matrix_dev if dev else m._lib.fiesta_hip_reach_matrix
    return fn(m._h, _p(blo), _p(bhi), _p(s), (0 if s is None else len(s)) if n_sources is None else n_sources, _p(t),
              (0 if t is None else len(t)) if n_targets is None else n_targets, float(clearance), int(conn), int(flags), int(max_fields),
              None if res is None else C.byref(res), None if info is None else C.byref(info))


def _result(cost=None, status=None, reached=None):
    from fiesta_amd._lib import ReachMatrixResult
    return ReachMatrixResult(*[None if a is None else a.ctypes.data for a in (cost, status, reached)])


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
    wide = Model.hashed(m, s - 24, top + 7)
    # the scene's own box; a box around it, unaligned in z, that straddles tiles without a page along x (unknown there) -- with
    # fewer sources: the model's floods through unknown space are the slow ones
    few = src[[0, 1, 8, 4]]
    for lo, hi, sources, flags, conn, clr in ((s, top - 1, src, 0, 26, 0.0), (s, top - 1, src, 0, 6, 0.25), (s - (19, 3, 3), top + 2, few, 1, 26, 0.0),
                                              (s - (19, 3, 3), top + 2, few, 0, 6, 0.0)):
        want = matrix_model(wide, sources, lo=lo, hi=hi, clearance=clr, conn=conn, flags=flags)
        got = m.ReachMatrix(sources, lo=lo, hi=hi, min_clearance=clr, connectivity=conn, flags=flags, max_fields=4)
        assert_same(got, want, f"hash box {lo} {hi} flags {flags} conn {conn} clearance {clr}")
        if flags:                          # around the scene the unknown space is a short cut past the walls, when asked for
            assert 0 < got["cost"][0, 1] < 200 and got["source_status"].tolist() == [0, 0, 1, 0]
        elif len(sources) == 4:
            assert got["cost"][0, 1] > 300 and got["source_status"].tolist() == [0, 0, 1, 0]
    # a hash-block map has no outside: the box is mandatory, and bounded
    assert raw_call(m, None, None, src, res=_result()) == 1
    assert raw_call(m, (0, 0, 0), (1023, 1023, 256), src, res=_result()) == 1
    assert_same(m.ReachMatrix(src, lo=s, hi=top - 1), matrix_model(wide, src, lo=s, hi=top - 1), "after the errors")
    m.close()


def test_retained_field_is_left_alone(scene_map):
    m, _ = scene_map
    targets = np.array([(38, 12, 20), (9, 1, 3), (33, 11, 11), (6, 12, 20), (15, 16, 31)], np.int32)
    m.ReachField([SOURCES[0]], want_cost=False)                                  # (the map retains this field)
    before = m.ReachPaths(targets, shortcut=True)
    m.ReachMatrix(SOURCES[1:], max_fields=3)
    m.ReachMatrix(SOURCES, lo=(3, 2, 5), hi=(37, 21, 36), connectivity=6)
    after = m.ReachPaths(targets, shortcut=True)
    assert before["offsets"][-1] > 10
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_empty_cases(scene_map):
    m, model = scene_map
    none = m.ReachMatrix(np.zeros((0, 3), np.int32))
    assert none["cost"].shape == (0, 0) and none["fields"] == 0 and none["batches"] == 0 and none["rounds"] == 0
    assert none["n_traversable"] == int((model.obs & ~model.occ).sum()) and none["box_lo"] == [0, 0, 0] and none["box_hi"] == [39, 23, 39]
    empty = m.ReachMatrix(SOURCES, lo=(5, 5, 5), hi=(4, 9, 9))
    assert_same(empty, matrix_model(model, SOURCES, lo=(5, 5, 5), hi=(4, 9, 9)), "empty box")
    assert (empty["cost"] == -1).all() and (empty["source_status"] == 1).all() and not empty["source_reached"].any()
    assert all(empty[k] == 0 for k in ("n_traversable", "n_sources_used", "fields", "batches", "rounds", "tile_visits"))
    assert empty["box_lo"] == [0, 0, 0] and empty["box_hi"] == [0, 0, 0]
    one = m.ReachMatrix([SOURCES[2]])
    assert one["cost"].tolist() == [[0]] and one["fields"] == 1 and one["batches"] == 1
    assert_same(one, matrix_model(model, [SOURCES[2]]), "one source")
    cols = m.ReachMatrix(SOURCES, targets=np.zeros((0, 3), np.int32))           # a matrix without columns: statuses and counts alone
    assert cols["cost"].shape == (11, 0) and np.array_equal(cols["source_status"], matrix_model(model, SOURCES)["source_status"])


def test_errors_leave_the_map_usable(scene_map):
    import fiesta_amd
    from fiesta_amd._lib import ReachMatrixInfo
    m, model = scene_map
    want = matrix_model(model, SOURCES[:3])
    cost = np.full((3, 3), -77, np.int32)
    status = np.full(3, -77, np.int32)
    res, info = _result(cost, status), ReachMatrixInfo()
    info.rounds = -5
    src = SOURCES[:3]
    many, cols = np.zeros((2 ** 15, 3), np.int32), np.zeros((2 ** 14, 3), np.int32)
    for dev in (False, True):
        calls = [lambda: raw_call(m, None, None, src, clearance=np.nan, res=res, info=info, dev=dev),
                 lambda: raw_call(m, (0, 0, 0), None, src, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, (5, 5, 5), src, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, src, conn=18, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, src, flags=2, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, src, max_fields=-1, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, src, n_sources=-1, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, src, targets=src, n_targets=-1, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, None, n_sources=3, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, src, targets=None, n_targets=2, res=res, info=info, dev=dev),
                 lambda: raw_call(m, None, None, many, targets=cols, res=_result(), info=info, dev=dev),     # 2^29 entries, cost NULL
                 lambda: raw_call(m, None, None, src, res=None, info=info, dev=dev)]
        for k, call in enumerate(calls):
            assert call() == 1, (dev, k)                       # FIESTA_HIP_ERR_INVALID
            assert np.array_equal(m.ReachMatrix(src)["cost"], want["cost"]), k     # ... and the map still answers a valid call
        assert "result" in fiesta_amd._lib.last_error()
    assert (cost == -77).all() and (status == -77).all() and info.rounds == -5   # nothing launched, nothing written
    with pytest.raises(ValueError):
        m.ReachMatrix(src, lo=(0, 0, 0))
    # every pointer of the result may be null, and so may the info
    assert raw_call(m, None, None, src, res=_result()) == 0
    assert raw_call(m, None, None, src, res=res, info=info) == 0
    assert np.array_equal(cost, want["cost"]) and np.array_equal(status, want["source_status"]) and info.n_sources_used == 3
    assert_same(m.ReachMatrix(src), want, "after the errors")
