"""The site tour on the GPU (fiesta_hip_site_tour[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/tour_kernels.hpp).

The expected result is always fiesta_amd.tour_model (tests/test_tour_rule.py holds it to the optimum on small matrices and to the
contract's sentences).  Everything is an integer and every tie has a rule: every comparison is exact equality of whole arrays,
no tolerance, no excluded entry.  Sizes: 13 (one wave holds a row of moves), 65 (a tour crosses a wave), 128 (the last size whose
matrix lives in LDS), 129 and 200 (the matrix read from global memory), 1 and 2 (nothing to search).
"""
import ctypes as C

import numpy as np
import pytest

from test_tour_rule import FIXTURES, INF, check_valid, skip_scene

pytestmark = pytest.mark.gpu
ARRAYS = ("order", "site_status", "leg_cost", "restart_length")
INFO = ("n_visited", "length", "best_restart", "nn_length", "moves", "capped")
_memo = {}


def model(cost, **kw):
    """tour_model, kept (the tests share the results and leave them unchanged)"""
    from fiesta_amd import tour_model
    key = (cost.tobytes(), cost.shape, tuple(sorted(kw.items())))
    if key not in _memo:
        _memo[key] = tour_model(cost, **kw)
    return _memo[key]


def assert_same(got, want, what=""):
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {len(bad)} entries of {k} differ, first at {bad[:3].tolist()}: got {got[k][bad[:3]].tolist()} " \
                              f"want {want[k][bad[:3]].tolist()}"
    for k in INFO:
        assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.fixture(scope="module")
def tmap(hip_lib):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, (1.6, 1.6, 1.6))     # the call reads no voxel: any map will do
    yield m
    m.close()


@pytest.mark.parametrize("kind,m,closed,R", [("points", 13, False, 32), ("points", 13, True, 32), ("random", 13, False, 32), ("random", 13, True, 32),
                                             ("points", 65, False, 8), ("random", 65, True, 8), ("points", 128, True, 8), ("random", 128, False, 8)])
def test_equal_to_the_model(tmap, kind, m, closed, R):
    cost = FIXTURES[kind](m, 3)
    want = model(cost, closed=closed, restarts=R, seed=12345)
    got = tmap.SiteTour(cost, closed=closed, restarts=R, seed=12345)
    print(f"{kind} m={m} closed={closed}: length {got['length']} (nearest neighbour {got['nn_length']}), {got['moves']} moves in {R} restarts")
    assert_same(got, want, f"{kind} {m} {closed}")
    assert got["capped"] == 0 and got["moves"] > 0
    check_valid(cost, got, 0, closed)


@pytest.mark.parametrize("kind,m,closed", [("random", 129, True), ("points", 200, False)])
def test_matrix_in_global_memory(tmap, kind, m, closed):
    cost = FIXTURES[kind](m, 5)
    want = model(cost, closed=closed, restarts=4, seed=77)
    got = tmap.SiteTour(cost, closed=closed, restarts=4, seed=77)
    assert np.array_equal(got["restart_length"], want["restart_length"])
    assert got["capped"] == 0
    check_valid(cost, got, 0, closed)                       # a permutation from the start, the legs, and no improving move left
    assert_same(got, want, f"{kind} {m}")


def test_start_and_cap(tmap):
    cost = FIXTURES["points"](40, 9)
    for kw in (dict(start=17, closed=True, restarts=5, seed=2), dict(start=39, restarts=3, seed=2 ** 64 - 1, max_moves=1),
               dict(restarts=1), dict(restarts=2, seed=1, max_moves=3)):
        got = tmap.SiteTour(cost, **kw)
        assert_same(got, model(cost, **kw), str(kw))
    assert model(cost, start=39, restarts=3, seed=2 ** 64 - 1, max_moves=1)["capped"] > 0


@pytest.mark.parametrize("closed", [False, True])
def test_costs_near_the_top_of_int32(tmap, closed):
    """every entry between 2^30 and 2^31 - 2: a delta is a sum of six of them and a length of m, both far above an int32"""
    c = np.random.default_rng(12).integers(2 ** 30, 2 ** 31 - 1, (24, 24))
    c = np.minimum(c, c.T)
    np.fill_diagonal(c, 0)
    cost = c.astype(np.int32)
    kw = dict(closed=closed, restarts=6, seed=3)
    want = model(cost, **kw)
    assert want["length"] > 2 ** 33 and want["moves"] > 10
    assert_same(tmap.SiteTour(cost, **kw), want, "large costs")


@pytest.mark.parametrize("closed", [False, True])
def test_tiny_tours(tmap, closed):
    cost = FIXTURES["random"](6, 8)
    for n in (1, 2, 3):
        c = np.ascontiguousarray(cost[:n, :n])
        got = tmap.SiteTour(c, closed=closed, restarts=3, seed=4)
        assert_same(got, model(c, closed=closed, restarts=3, seed=4), f"n = {n}")
        if n < 3:
            assert got["moves"] == 0 and got["order"].tolist() == list(range(n))
    # m = 1 and 2 inside a larger matrix: the start reaches nothing / one site
    c = np.full((5, 5), INF, np.int32)
    np.fill_diagonal(c, 0)
    got = tmap.SiteTour(c, start=3, closed=closed)
    assert got["order"].tolist() == [3, -1, -1, -1, -1] and got["n_visited"] == 1 and got["length"] == 0
    assert_same(got, model(c, start=3, closed=closed), "alone")
    c[1, 3] = c[3, 1] = 9
    got = tmap.SiteTour(c, start=3, closed=closed)
    assert got["order"].tolist() == [3, 1, -1, -1, -1] and got["length"] == (18 if closed else 9)
    assert_same(got, model(c, start=3, closed=closed), "a pair")


def raw_call(m, cost, n, ld, start, flags, R, seed, max_moves, outs, info=None, dev=False):
    """the C call itself on host arrays or device pointers; returns the status"""
    from fiesta_amd._lib import TourResult
    ptr = (lambda a: None if a is None else a.data_ptr()) if dev else (lambda a: None if a is None else a.ctypes.data)
    res = TourResult(*[ptr(a) for a in outs])
    fn = m._lib.fiesta_hip_site_tour_dev if dev else m._lib.fiesta_hip_site_tour
    return fn(m._h, C.c_void_p(ptr(cost)), n, ld, start, flags, R, seed, max_moves, C.byref(res), None if info is None else C.byref(info))


def test_skipped_sites_and_the_error_word(tmap):
    import torch
    import fiesta_amd
    from fiesta_amd._lib import TourInfo
    cost = skip_scene()
    for kw in (dict(start=3, restarts=4, seed=1), dict(start=6, closed=True, restarts=2), dict(start=2)):
        got = tmap.SiteTour(cost, **kw)
        assert_same(got, model(cost, **kw), str(kw))
    assert tmap.SiteTour(cost, start=3)["site_status"].tolist() == [0, 0, 1, 0, 0, 1, 1, 0, 0]
    # the two errors among visited sites are found on the device: status 1, and nothing is written -- host and device variant
    no_conn, asym = cost.copy(), cost.copy()
    no_conn[1, 7] = no_conn[7, 1] = INF
    asym[0, 8] += 1
    dev = torch.device("cuda", 0)
    for bad, word in ((no_conn, "connection"), (asym, "symmetric")):
        outs = [np.full(9, -77, np.int32) for _ in range(3)] + [np.full(4, -77, np.int64)]
        info = TourInfo()
        info.moves = -5
        assert raw_call(tmap, bad, 9, 9, 3, 0, 4, 1, 0, outs, info) == 1
        assert word in fiesta_amd._lib.last_error()
        assert all((a == -77).all() for a in outs) and info.moves == -5
        douts = [torch.full((9,), -77, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.full((4,), -77, dtype=torch.int64, device=dev)]
        dcost = torch.tensor(bad, device=dev)
        torch.cuda.synchronize()
        assert raw_call(tmap, dcost, 9, 9, 3, 0, 4, 1, 0, douts, info, dev=True) == 1
        assert word in fiesta_amd._lib.last_error()
        assert all((a.cpu().numpy() == -77).all() for a in douts) and info.moves == -5
        # ... and the map still answers; among SKIPPED sites neither rule holds
        assert_same(tmap.SiteTour(cost, start=3, restarts=4, seed=1), model(cost, start=3, restarts=4, seed=1), "after the error")
    assert tmap.SiteTour(no_conn, start=6)["n_visited"] == 2 and tmap.SiteTour(asym, start=5, closed=True)["order"][:2].tolist() == [5, 6]
    # every pointer of the result may be null, and so may the result and the info
    assert raw_call(tmap, cost, 9, 9, 3, 0, 4, 1, 0, [None] * 4) == 0
    info = TourInfo()
    assert tmap._lib.fiesta_hip_site_tour(tmap._h, C.c_void_p(cost.ctypes.data), 9, 9, 3, 0, 4, 1, 0, None, C.byref(info)) == 0
    assert info.n_visited == 6 and info.length == model(cost, start=3, restarts=4, seed=1)["length"]


def test_host_variant_with_a_leading_dimension(tmap):
    cost = FIXTURES["random"](21, 6)
    wide = np.full((21, 32), -9, np.int32)
    wide[:, :21] = cost
    kw = dict(start=4, closed=True, restarts=6, seed=31)
    got = tmap.SiteTour(wide, **kw)
    assert_same(got, model(cost, **kw), "ld = 32")
    assert_same(got, model(wide, **kw), "the model on the wide matrix")
    last = np.concatenate([wide[:20].reshape(-1), cost[20]])          # the last row may end after n entries
    outs = [np.empty(21, np.int32) for _ in range(3)] + [np.empty(6, np.int64)]
    assert raw_call(tmap, last, 21, 32, 4, 1, 6, 31, 0, outs) == 0
    assert all(np.array_equal(a, got[k]) for a, k in zip(outs, ARRAYS))


def wall_scene_maps():
    """test_reach_matrix_rule's scene on a dense and on a hash-block map, with the sources as each map sees them"""
    import fiesta_amd
    from scenarios import P_DEFAULT
    from test_gpu_reach import RES, new_dense, occupy
    from test_gpu_reach_matrix import HASH_SHIFT
    from test_reach_matrix_rule import SCENE_SHAPE, SOURCES, scene
    obs, occ = scene()
    d = new_dense(SCENE_SHAPE)
    d.SetOccupancy(np.argwhere(obs & ~occ).astype(np.int32), 0, want_ret=False)
    d.UpdateOccupancy(True)
    d.UpdateESDF()
    occupy(d, np.argwhere(occ))
    yield d, np.array(SOURCES, np.int32), None, None
    d.close()
    h = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=200000, mode="hash")
    h.SetParameters(*P_DEFAULT)
    h.SetOriginalRange()
    s = HASH_SHIFT
    h.SetOccupancy((np.argwhere(obs & ~occ) + s).astype(np.int32), 0, want_ret=False)
    h.UpdateOccupancy(True)
    h.UpdateESDF()
    occupy(h, np.argwhere(occ) + s)
    yield h, (np.array(SOURCES, np.int64) + s).astype(np.int32), s, s + np.array(SCENE_SHAPE) - 1
    h.close()


def test_device_variant_fed_by_the_reach_matrix(hip_lib):
    import torch
    dev = torch.device("cuda", 0)
    seen = []
    for m, src, lo, hi in wall_scene_maps():
        n, R = len(src), 5
        sd = torch.tensor(src, device=dev)
        dcost = torch.full((n * n,), -99, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        m.ReachMatrixDevice(sd.data_ptr(), n, lo=lo, hi=hi, cost_dev_ptr=dcost.data_ptr())
        outs = [torch.full((n + 4,), -99, dtype=torch.int32, device=dev) for _ in range(3)]
        lens = torch.full((R + 4,), -99, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        info = m.SiteTourDevice(dcost.data_ptr(), n, n, start=1, closed=True, restarts=R, seed=8, order_dev_ptr=outs[0].data_ptr(),
                                site_status_dev_ptr=outs[1].data_ptr(), leg_cost_dev_ptr=outs[2].data_ptr(), restart_length_dev_ptr=lens.data_ptr())
        cost = dcost.cpu().numpy().reshape(n, n)                   # (the call has synchronised with the map's stream)
        want = model(cost, start=1, closed=True, restarts=R, seed=8)
        for a, k in zip(outs + [lens], ARRAYS):
            a = a.cpu().numpy()
            assert np.array_equal(a[:len(want[k])], want[k]) and (a[len(want[k]):] == -99).all(), k
        assert all(info[k] == want[k] for k in INFO)
        # the scene's sites: 3 and 6 blocked, 8 outside, 4 and 5 sealed in their box
        assert want["site_status"].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 0] and want["n_visited"] == 6
        # no output at all: the info alone; and the host variant on the downloaded matrix
        assert m.SiteTourDevice(dcost.data_ptr(), n, n, start=1, closed=True, restarts=R, seed=8) == info
        assert_same(m.SiteTour(cost, start=1, closed=True, restarts=R, seed=8), want, "host variant")
        seen.append(cost)
    assert len(seen) == 2 and np.array_equal(seen[0], seen[1])


def test_retained_field_is_left_alone(hip_lib):
    from test_reach_matrix_rule import SOURCES
    m, src, _, _ = next(wall_scene_maps())
    targets = np.array([(38, 12, 20), (9, 1, 3), (33, 11, 11), (6, 12, 20), (15, 16, 31)], np.int32)
    m.ReachField([SOURCES[0]], want_cost=False)                                  # (the map retains this field)
    before = m.ReachPaths(targets, shortcut=True)
    cost = m.ReachMatrix(src)["cost"]
    m.SiteTour(cost, restarts=8)
    m.SiteTour(FIXTURES["points"](150, 1), restarts=2, closed=True)
    after = m.ReachPaths(targets, shortcut=True)
    assert before["offsets"][-1] > 10
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    m.close()
