"""Corridor bounds on the device (fiesta_hip_corridor_bounds[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/bounds_kernels.hpp).

The model is fiesta_amd.corridor_bounds_model (tests/test_bounds_rule.py holds it to fiesta_amd.corridor_bounds and to literal
loops).  Every output is compared bit for bit: `bounds` as int64 views, `ok` and `box` exactly.  The call reads no voxel, so any tiny
map serves; both stores run, because each hands its own stream and scratch to the one function of planner.hip.  Then the real chain on the
reach example's scene: the class method against fiesta_amd.corridor_bounds, and reach paths -> corridors -> bounds -> refinement all
on the device against the route that computes the bounds on the host.
"""
import ctypes as C

import numpy as np
import pytest

from test_bounds_rule import bits, boxes_pos, walk
from test_gpu_path_cost import hash_map_scene
from test_gpu_path_queries import dense_map
from test_gpu_refine import flagged_paths

pytestmark = pytest.mark.gpu
# 0 .. 3: no, one, a few steps; 63 .. 66, 127 .. 130: one and two chunks of 64 lanes +- 2; 1025, 5003: many chunks, the carry
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 130, 1025, 5003]
BOXES = [0, 1, 2, 63, 64, 65]                # a path's box count: none, one, a search of one step, of six and seven steps
SENTINEL, GUARD = -7, 5
INSET = 0.25 * 2.0 ** -20
SPECIAL = ("edge", "skipped", "first_outside", "blocked", "invalid")


def make_batch(seed=11):
    """two paths per entry of LENGTHS with box counts cycling through BOXES (every count meets a short and a long path), then one
    path of each special kind, all in shuffled order.  Returns (waypoints_vox, offsets, corridor, special: kind -> path index)"""
    rng = np.random.RandomState(seed)
    paths, bxs, ents, status = [], [], [], []
    for k, m in enumerate(LENGTHS + LENGTHS):
        v = walk(rng, m, (6, 26, "long")[k % 3])
        nb = BOXES[(k + (3 if k < len(LENGTHS) else 2)) % len(BOXES)]    # (1025 and 5003 waypoints: 63, 64 and 64, 65 boxes)
        chain = int(np.abs(np.diff(v, axis=0)).sum()) if m > 1 else 0
        if chain + 2 >= nb - 1 > 0:                                      # distinct entries: a 6-connected walk skips no box
            e = np.sort(rng.choice(np.arange(1, chain + 3), nb - 1, replace=False))
        else:
            e = np.sort(rng.randint(1, max(2, chain + 3), max(nb - 1, 0)))
        e = np.concatenate([[0], e])[:nb]
        lo = (v.min(axis=0) if m else np.zeros(3, np.int64)) - rng.randint(0, 4, (nb, 3))
        hi = (v.max(axis=0) if m else np.zeros(3, np.int64)) + rng.randint(0, 4, (nb, 3))
        if k % 4 == 1:                                                   # small boxes: empty intersections, first waypoints outside
            lo = v[rng.randint(0, max(m, 1), nb) % max(m, 1)] - rng.randint(0, 3, (nb, 3)) if m else lo
            hi = lo + rng.randint(0, 6, (nb, 3))
        paths.append(v), bxs.append(np.concatenate([lo, hi], axis=1).reshape(nb, 6)), ents.append(e), status.append(0 if k % 5 else 2)
    line = np.stack([np.arange(130), np.zeros(130, np.int64), np.zeros(130, np.int64)], axis=1)
    # a box change exactly at a chunk edge: c_i = i, box 1 entered at waypoint 64
    paths.append(line), bxs.append(np.array([[-1, -1, -1, 70, 1, 1], [-2, -1, 0, 140, 2, 1]])), ents.append([0, 64]), status.append(0)
    # a skipped box: the chain index jumps from 4 to 8 over the box entered at 5
    paths.append(np.array([[0, 0, 0], [4, 0, 0], [8, 0, 0], [9, 0, 0]]))
    bxs.append(np.array([[0, 0, 0, 4, 1, 1], [4, 0, 0, 5, 0, 0], [5, 0, 0, 9, 0, 0]])), ents.append([0, 5, 6]), status.append(0)
    # a diagonal first move out of the first box: w_0 is not in the box w_1 changes to
    paths.append(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]])), bxs.append(np.array([[0, 0, 0, 1, 1, 1], [1, 1, 1, 5, 5, 5]])), ents.append([0, 3])
    status.append(0)
    # BLOCKED: the waypoints run on past the last box
    paths.append(line[:20] + 3), bxs.append(np.array([[3, 3, 3, 8, 3, 3], [8, 3, 3, 10, 4, 4]])), ents.append([0, 5]), status.append(2)
    # INVALID: the corridor call made no box
    paths.append(line[:10] - 5), bxs.append(np.zeros((0, 6), np.int64)), ents.append([]), status.append(1)
    order = rng.permutation(len(paths))
    special = {kind: int(np.nonzero(order == len(paths) - len(SPECIAL) + j)[0][0]) for j, kind in enumerate(SPECIAL)}
    paths, bxs, ents, status = ([x[i] for i in order] for x in (paths, bxs, ents, status))
    off = np.concatenate([[0], np.cumsum([len(v) for v in paths])]).astype(np.int64)
    bx = np.concatenate(bxs).astype(np.int32).reshape(-1, 6)
    cor = {"offsets": np.concatenate([[0], np.cumsum([len(b) for b in bxs])]).astype(np.int64), "boxes": bx, "boxes_pos": boxes_pos(bx),
           "entry": np.concatenate([np.asarray(e, np.int64) for e in ents]).astype(np.int32), "status": np.array(status, np.int32)}
    return np.concatenate(paths).astype(np.int32).reshape(-1, 3), off, cor, special


@pytest.fixture(scope="module")
def batch():
    """the batch and the model's answers, computed once: (wv, off, cor, special, {void_broken: model})"""
    import fiesta_amd
    wv, off, cor, special = make_batch()
    want = {vb: fiesta_amd.corridor_bounds_model(wv, off, cor, INSET, void_broken=vb) for vb in (False, True)}
    return wv, off, cor, special, want


@pytest.fixture(scope="module", params=["dense", "hash"])
def store(request, hip_lib):
    m = dense_map(16, obstacles=10, seed=3)[0] if request.param == "dense" else hash_map_scene()[0]
    yield m
    m.close()


def host_call(m, wv, off, cor, inset, flags, n_boxes=None, outputs=("bounds", "ok", "box"), expect=0):
    """fiesta_hip_corridor_bounds through ctypes, every output pre-filled with the sentinel"""
    from fiesta_amd._lib import BoundsResult
    n, nw = len(off) - 1, len(wv)
    out = {"bounds": np.full((nw, 6), float(SENTINEL)), "ok": np.full(n, SENTINEL, np.int32), "box": np.full(nw, SENTINEL, np.int64)}
    res = BoundsResult(*[out[k].ctypes.data if k in outputs else None for k in ("bounds", "ok", "box")])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb = len(cor["entry"]) if n_boxes is None else n_boxes
    st = m._lib.fiesta_hip_corridor_bounds(m._h, p(wv), nw, p(off), n, p(cor["offsets"]), p(cor["boxes"]), p(cor["boxes_pos"]), p(cor["entry"]),
                                           p(cor["status"]), nb, inset, flags, C.byref(res))
    assert st == expect, st
    return out


def device_call(m, wv, off, cor, inset, void_broken, n_boxes=None, outputs=("bounds", "ok", "box")):
    """fiesta_hip_corridor_bounds_dev on torch tensors; every output has GUARD extra rows and is pre-filled with the sentinel"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    n, nw = len(off) - 1, len(wv)
    nb = len(cor["entry"]) if n_boxes is None else n_boxes
    t = {"wv": up(wv, np.int32), "off": up(off, np.int64), "boff": up(cor["offsets"], np.int64), "boxes": up(cor["boxes"][:nb], np.int32),
         "pos": up(cor["boxes_pos"][:nb], np.float64), "entry": up(cor["entry"][:nb], np.int32), "status": up(cor["status"], np.int32)}
    outs = {"bounds": torch.full((nw + GUARD, 6), float(SENTINEL), dtype=torch.float64, device=dev),
            "ok": torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=dev),
            "box": torch.full((nw + GUARD,), SENTINEL, dtype=torch.int64, device=dev)}
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the copies and fills above must have landed)
    ptr = {k: (outs[k].data_ptr() if k in outputs else 0) for k in outs}
    m.CorridorBoundsDevice(t["wv"].data_ptr(), nw, t["off"].data_ptr(), n, t["boff"].data_ptr(), t["boxes"].data_ptr(), t["pos"].data_ptr(),
                           t["entry"].data_ptr(), t["status"].data_ptr(), nb, inset=inset, void_broken=void_broken, bounds_dev_ptr=ptr["bounds"],
                           ok_dev_ptr=ptr["ok"], box_dev_ptr=ptr["box"])
    m.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    for k, rows in (("bounds", nw), ("ok", n), ("box", nw)):              # the guard rows stay untouched
        assert (got[k][rows:] == SENTINEL).all(), k
        got[k] = got[k][:rows]
    return got


def assert_equals_model(got, want, what):
    a, b = bits(got["bounds"]), bits(want["bounds"])
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{what} bounds: {len(bad)} entries differ, first {bad[:3].tolist()}: {got['bounds'][tuple(bad[0])]!r} vs {want['bounds'][tuple(bad[0])]!r}"
    for k in ("ok", "box"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries differ, first {bad[:5]}: {got[k][bad[:5]]} vs {want[k][bad[:5]]}"


def test_the_synthetic_batch_equals_the_model(store, batch):
    wv, off, cor, special, want = batch
    lens, nbs = np.diff(off), np.diff(cor["offsets"])
    assert set(LENGTHS) <= set(lens.tolist()) and set(BOXES) <= set(nbs.tolist())
    plain = want[False]
    # the batch holds what it was made for: the special paths behave as named, and there are whole paths with intersections
    o = off[special["edge"]]
    assert plain["ok"][special["edge"]] == 1 and plain["box"][o + 63] + 1 == plain["box"][o + 64]
    assert (bits(plain["bounds"][o + 63]) != bits(plain["bounds"][o + 62])).any()
    for kind in ("skipped", "first_outside", "blocked", "invalid"):
        assert plain["ok"][special[kind]] == 0, kind
    assert cor["status"][special["skipped"]] == 0 and cor["status"][special["first_outside"]] == 0
    assert np.isnan(plain["bounds"][off[special["invalid"]]:off[special["invalid"] + 1]]).all()
    assert not np.isnan(plain["bounds"][off[special["blocked"]]:off[special["blocked"] + 1]]).any()
    assert plain["ok"][lens == 5003].any() and plain["ok"][lens == 1025].any() and 8 <= plain["ok"].sum() <= len(lens) - 8
    for void_broken in (False, True):
        what = f"void_broken={void_broken}"
        assert_equals_model(host_call(store, wv, off, cor, INSET, int(void_broken)), want[void_broken], "host, " + what)
        assert_equals_model(device_call(store, wv, off, cor, INSET, void_broken), want[void_broken], "device, " + what)
    broken = np.repeat(plain["ok"] == 0, lens)
    assert np.isnan(want[True]["bounds"][broken]).all() and not np.isnan(plain["bounds"][broken]).all()
    # the class method, and its default inset
    cls = store.CorridorBounds(wv, off, cor, inset=INSET, void_broken=True)
    assert_equals_model(cls, want[True], "class")
    import fiesta_amd
    dflt = store.CorridorBounds(wv[:off[3]], off[:4], {k: (v[:4] if k == "offsets" else v[:3] if k == "status" else v) for k, v in cor.items()})
    assert_equals_model(dflt, fiesta_amd.corridor_bounds_model(wv[:off[3]], off[:4], dict(cor, offsets=cor["offsets"][:4], status=cor["status"][:3]),
                                                               store.resolution * 2.0 ** -20), "class, default inset")


def test_broken_device_offsets_and_a_truncated_corridor(store, batch):
    import fiesta_amd
    wv, off, cor, special, _ = batch
    n = len(off) - 1
    bad = off.copy()
    bad[5], bad[6] = off[6], off[5]                         # waypoint offsets that decrease
    bad[12] = len(wv) + 5                                   # ... that leave the range
    bad[20] = -3
    boff = cor["offsets"].copy()
    boff[9], boff[10] = cor["offsets"][10], cor["offsets"][9]   # a decreasing box range
    n_boxes = int(cor["offsets"][n - 4])                    # a truncated corridor: the last paths' boxes are not there
    bad_cor = dict(cor, offsets=boff)
    flagged = flagged_paths(bad, len(wv))
    bad_box = (boff[:-1] < 0) | (boff[1:] < boff[:-1]) | (boff[1:] > n_boxes)
    assert 3 <= flagged.sum() <= 8 and 2 <= bad_box.sum() <= 8 and not (flagged | bad_box)[[0, 1, 2]].any()
    for void_broken in (False, True):
        want = fiesta_amd.corridor_bounds_model(wv, bad, bad_cor, INSET, void_broken=void_broken, n_boxes=n_boxes, device_offsets=True)
        got = device_call(store, wv, bad, bad_cor, INSET, void_broken, n_boxes=n_boxes)
        assert_equals_model(got, want, f"device, broken offsets, void_broken={void_broken}")
        assert (got["ok"][flagged | bad_box] == 0).all()
        owned = np.zeros(len(wv), bool)
        for p in np.nonzero(~(flagged | bad_box))[0]:
            owned[bad[p]:bad[p + 1]] = True
        assert (~owned).sum() >= 10 and np.isnan(got["bounds"][~owned]).all() and (got["box"][~owned] == -1).all()
    # the host variant refuses each of them as a whole call, and writes nothing
    for o, c, nb in ((bad, cor, None), (off, bad_cor, None), (off, cor, n_boxes)):
        out = host_call(store, wv, o, c, INSET, 0, n_boxes=nb, expect=1)
        assert all((v == SENTINEL).all() for v in out.values())


def test_null_outputs_are_not_written(store, batch):
    wv, off, cor, _, want = batch
    for only in ("bounds", "ok", "box"):
        for got in (host_call(store, wv, off, cor, INSET, 0, outputs=(only,)), device_call(store, wv, off, cor, INSET, False, outputs=(only,))):
            for k in ("bounds", "ok", "box"):
                if k == only:
                    assert np.array_equal(bits(got[k]) if k == "bounds" else got[k], bits(want[False][k]) if k == "bounds" else want[False][k]), (only, k)
                else:
                    assert (got[k] == SENTINEL).all(), (only, k)


def test_whole_call_errors_leave_the_map_usable(store, batch):
    from fiesta_amd._lib import BoundsResult
    wv, off, cor, _, want = batch
    q = np.array([[0.35, 0.45, 0.55]])
    before = store.GetDistWithGradTrilinear(q)[0][0]
    for kw in (dict(inset=float("nan")), dict(inset=-0.5), dict(inset=float("inf")), dict(flags=2), dict(flags=-1), dict(n_boxes=-1)):
        out = host_call(store, wv, off, cor, kw.get("inset", INSET), kw.get("flags", 0), n_boxes=kw.get("n_boxes"), expect=1)
        assert all((v == SENTINEL).all() for v in out.values()), kw
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = (p(wv), len(wv), p(off), len(off) - 1, p(cor["offsets"]), p(cor["boxes"]), p(cor["boxes_pos"]), p(cor["entry"]), p(cor["status"]),
            len(cor["entry"]), INSET, 0)
    for fn in (store._lib.fiesta_hip_corridor_bounds, store._lib.fiesta_hip_corridor_bounds_dev):
        assert fn(store._h, *args, None) == 1                           # result NULL
        none = C.byref(BoundsResult(None, None, None))
        # (every call below is refused before anything is launched: the host arrays never reach the _dev entry's kernels)
        for k in (0, 2, 4, 5, 6, 7, 8):                                 # each input NULL while its count is > 0
            assert fn(store._h, *args[:k], None, *args[k + 1:], none) == 1, k
        for k in (1, 3, 9):                                             # each count negative
            assert fn(store._h, *args[:k], -1, *args[k + 1:], none) == 1, k
    # n_paths = 0 touches nothing (not even the fill)
    ok = np.full(4, SENTINEL, np.int32)
    b = np.full((len(wv), 6), float(SENTINEL))
    res = BoundsResult(b.ctypes.data, ok.ctypes.data, None)
    assert store._lib.fiesta_hip_corridor_bounds(store._h, *args[:3], 0, *args[4:], C.byref(res)) == 0
    assert (ok == SENTINEL).all() and (b == SENTINEL).all()
    assert store.GetDistWithGradTrilinear(q)[0][0] == before
    assert_equals_model(host_call(store, wv, off, cor, INSET, 0), want[False], "after the errors")


PAR = dict(margin=0.8, w_obstacle=1.0, w_smooth=2.0, alpha=0.02, max_step=0.05, tolerance=0.0, iterations=24)


@pytest.mark.parametrize("shortcut", [False, True])
def test_the_chain_on_the_device_equals_the_host_bounds_route(hip_lib, shortcut):
    """reach paths -> corridors (a window that cuts some of them short) -> bounds -> refinement.  The class method equals
    fiesta_amd.corridor_bounds bit for bit; the chain that never leaves the device (VOID_BROKEN) refines the ok paths to the same
    bits as the route through the host function, and returns every other path INVALID and unmoved"""
    import torch
    import fiesta_amd
    from test_cpp_reach import example_scene
    m = example_scene()
    inset = 0.2 * 2.0 ** -20
    fv, _ = m.GetFrontierVoxels()
    fv = np.array(sorted(fv.tolist()), np.int32)
    m.ReachField([(12, 20, 10)], want_cost=False)
    paths = m.ReachPaths(fv, shortcut=shortcut)
    wv, w, off = paths["waypoints_vox"], paths["waypoints_pos"], paths["offsets"]
    win = dict(lo=(0, 0, 0), hi=(39, 39, 13), max_grow=8)
    cor = m.PathCorridor(wv, off, **win)
    bounds, ok = fiesta_amd.corridor_bounds(wv, off, cor, inset=inset)
    assert (~ok).sum() >= 1 and ok.sum() >= 100
    assert not np.signbit(cor["boxes_pos"][cor["boxes_pos"] == 0]).any()
    for got in (m.CorridorBounds(wv, off, cor, inset=inset), m.CorridorBounds(wv, off, cor)):   # (0.2 * 2^-20 is the default here)
        assert np.array_equal(bits(got["bounds"]), bits(bounds)) and np.array_equal(got["ok"] != 0, ok)
        assert ((got["box"] >= 0) == ~np.isnan(bounds).any(axis=1)).all()
    host = m.PathRefine(w, off, bounds, **PAR)
    # the same chain without leaving the device; the buffer sizes are the host route's totals
    dev = torch.device("cuda", 0)
    n, nw, nb = len(fv), len(wv), len(cor["entry"])
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    t_fv = torch.from_numpy(fv).to(dev)
    d_off, d_wv, d_w = z(n + 1, torch.int64), z((nw, 3), torch.int32), z((nw, 3), torch.float64)
    d_boff, d_boxes, d_pos, d_entry, d_status = z(n + 1, torch.int64), z((nb, 6), torch.int32), z((nb, 6), torch.float64), z(nb, torch.int32), z(n, torch.int32)
    d_bounds, d_ok = z((nw, 6), torch.float64), z(n, torch.int32)
    d_out, d_rstatus = z((nw, 3), torch.float64), z(n, torch.int32)
    torch.cuda.synchronize()
    m.ReachPathsDevice(t_fv.data_ptr(), n, d_off.data_ptr(), shortcut=shortcut, capacity=nw, waypoints_vox_dev_ptr=d_wv.data_ptr(),
                       waypoints_pos_dev_ptr=d_w.data_ptr())
    m.PathCorridorDevice(d_wv.data_ptr(), nw, d_off.data_ptr(), n, d_boff.data_ptr(), capacity=nb, boxes_dev_ptr=d_boxes.data_ptr(),
                         boxes_pos_dev_ptr=d_pos.data_ptr(), entry_dev_ptr=d_entry.data_ptr(), status_dev_ptr=d_status.data_ptr(), **win)
    m.CorridorBoundsDevice(d_wv.data_ptr(), nw, d_off.data_ptr(), n, d_boff.data_ptr(), d_boxes.data_ptr(), d_pos.data_ptr(), d_entry.data_ptr(),
                           d_status.data_ptr(), nb, void_broken=True, bounds_dev_ptr=d_bounds.data_ptr(), ok_dev_ptr=d_ok.data_ptr())
    m.PathRefineDevice(d_w.data_ptr(), nw, d_off.data_ptr(), n, d_bounds.data_ptr(), out={"waypoints": d_out.data_ptr(), "status": d_rstatus.data_ptr()},
                       **PAR)
    m.synchronize()
    assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_ok.cpu().numpy() != 0, ok)
    refined, rstatus = d_out.cpu().numpy(), d_rstatus.cpu().numpy()
    rows_ok = np.repeat(ok, np.diff(off))
    assert np.array_equal(bits(refined[rows_ok]), bits(host["waypoints"][rows_ok])) and (rstatus[ok] == 0).all()
    if not shortcut:                                                   # (raw staircases: the refinement did move them)
        assert (host["waypoints"][rows_ok] != w[rows_ok]).sum() > 100
    # a broken corridor of at most two waypoints has no interior bounds row to read: nothing can move, and nothing says INVALID
    inner = ~ok & (np.diff(off) > 2)
    assert (inner.sum() >= 1 or shortcut) and (rstatus[inner] == fiesta_amd.REFINE_INVALID).all()
    print(f"shortcut={shortcut}: {ok.sum()} of {len(ok)} corridors whole, {inner.sum()} broken ones with an interior waypoint")
    assert np.array_equal(bits(refined[~rows_ok]), bits(w[~rows_ok]))
    m.close()
