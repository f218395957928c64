"""Path refinement on the device (fiesta_hip_path_refine[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/refine_kernels.hpp).

The model is fiesta_amd.path_refine_model over GetDistWithGradTrilinear on the same map (the header's formulas in numpy;
tests/test_refine_rule.py checks it against a literal loop and against central differences).  Everything but `cost` is compared bit
for bit (floats as int64 views); `cost` within (n + 16) * 2^-52 * A of the model's (cost_n, cost_abs), NaN exactly where the model
has NaN: the terms are bit-identical, only the order of their sum differs.  Then the whole chain -- reach paths, corridors,
corridor_bounds, refinement -- is checked without the model: the refined polylines of whole corridors stay in observed free voxels.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_path_cost import hash_map_scene
from test_gpu_path_queries import dense_map, wall_map

pytestmark = pytest.mark.gpu
# 0 .. 6: no, one, a few interior waypoints; 63 .. 66: a wave's lanes; 126 .. 130: the split between a wave and a work-group per path
# (kRefineWaveMax = 128) +- 2; 255 .. 258: the work-group's lanes; 1023, 1024: the cap; 1025: INVALID
LENGTHS = [0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 66, 126, 127, 128, 129, 130, 255, 256, 257, 258, 1023, 1024, 1025]
PAR = dict(margin=0.45, w_obstacle=1.0, w_smooth=0.5, alpha=0.05, max_step=0.03)
SENTINEL = -7
FLOATS, INTS = ("waypoints", "last_move", "min_dist"), ("iterations", "n_below", "status")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def make_batch(lo, hi, seed):
    """one path per entry of LENGTHS (twice: a rough walk and a nearly straight line), then a path with a NaN waypoint and one whose
    bounds (see make_bounds) hold lo > hi.  Every fourth path lies outside the box [lo, hi] (a dense map's outside), every seventh
    starts inside and walks out of it."""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    paths = []
    for k, n in enumerate(LENGTHS + LENGTHS + [7, 6]):
        start = lo + (0.15 + 0.7 * rng.rand(3)) * (hi - lo)
        if k % 2 == 0:   # rough: the smoothness term moves it for many iterations
            pts = start + np.cumsum(rng.randn(n, 3) * (0.08 if n < 200 else 0.02), axis=0)
        else:            # a line with a little noise: only obstacles move it
            pts = start + np.arange(n)[:, None] * (rng.randn(3) * 0.5 / max(n, 8)) + rng.randn(n, 3) * 1e-4
        if k % 4 == 3:
            pts = pts + (hi - lo) * 3.0
        if k % 7 == 5 and n:
            pts = pts + np.linspace(0, 1, n)[:, None] * (hi - lo)
        paths.append(pts.reshape(-1, 3))
    paths[-2][3, 1] = np.nan
    order = rng.permutation(len(paths))
    paths = [paths[i] for i in order]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    special = {"nan": int(np.nonzero(order == len(order) - 2)[0][0]), "lo_gt_hi": int(np.nonzero(order == len(order) - 1)[0][0])}
    return np.concatenate(paths), off, special


def make_bounds(w, off, special, kind, seed):
    if kind == "none":
        return None
    rng = np.random.RandomState(seed)
    c = np.nan_to_num(w)
    b = np.concatenate([c - rng.rand(*w.shape) * 0.12, c + rng.rand(*w.shape) * 0.12], axis=1)
    if kind == "mixed":
        b[rng.rand(len(w)) < 0.3, 0] = -np.inf
        b[rng.rand(len(w)) < 0.3, 4] = np.inf
        b[rng.rand(len(w)) < 0.2] = [-np.inf] * 3 + [np.inf] * 3
        pin = rng.rand(len(w)) < 0.1
        b[pin, :3], b[pin, 3:] = c[pin], c[pin]
        b[off[:-1][np.diff(off) > 0]] = np.nan            # the rows of the ends are not read
    p = special["lo_gt_hi"]
    b[off[p] + 2, 2], b[off[p] + 2, 5] = 1.0, 0.5
    return b


def flagged_paths(off, n_wp):
    """the device variant's offset rule (path clearance's): a path is valid iff its start is in range and is the running maximum of
    the in-range entries before it, and its end lies in [start, n_waypoints]"""
    off = np.asarray(off, np.int64)
    o0, o1 = off[:-1], off[1:]
    run = np.maximum.accumulate(np.where((o0 >= 0) & (o0 <= n_wp), o0, np.iinfo(np.int64).min))
    return ~((o0 >= 0) & (o0 == run) & (o1 >= o0) & (o1 <= n_wp))


def expected(m, w, off, b, par, device_offsets=False):
    """the model's answer for the batch; with device_offsets the paths the offset rule flags are INVALID, the others are refined
    over the ranges they name, and every row outside them keeps the input"""
    import fiesta_amd
    n_paths = len(off) - 1
    flagged = flagged_paths(off, len(w)) if device_offsets else np.zeros(n_paths, bool)
    keep = np.nonzero(~flagged)[0]
    rows = np.concatenate([np.arange(off[p], off[p + 1]) for p in keep] + [np.zeros(0, np.int64)]).astype(np.int64)
    sub_off = np.concatenate([[0], np.cumsum(off[keep + 1] - off[keep])]).astype(np.int64)
    sub = fiesta_amd.path_refine_model(m.GetDistWithGradTrilinear, w[rows], sub_off, None if b is None else b[rows], **par)
    out = {"waypoints": w.copy(), "cost": np.full((n_paths, 2), np.nan), "last_move": np.full(n_paths, np.nan), "iterations": np.full(n_paths, -1, np.int32),
           "n_below": np.full(n_paths, -1, np.int64), "min_dist": np.full(n_paths, np.nan), "status": np.ones(n_paths, np.int32),
           "cost_n": np.zeros((n_paths, 2), np.int64), "cost_abs": np.zeros((n_paths, 2))}
    out["waypoints"][rows] = sub["waypoints"]
    for k in ("cost", "last_move", "iterations", "n_below", "min_dist", "status", "cost_n", "cost_abs"):
        out[k][keep] = sub[k]
    return out


def assert_equals_model(got, want, what):
    for k in FLOATS:
        a, b = bits(got[k]), bits(want[k])
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries differ, first {bad[:3].tolist()}: {np.asarray(got[k])[tuple(bad[0])]!r} vs {want[k][tuple(bad[0])]!r}"
    for k in INTS:
        bad = np.nonzero(np.asarray(got[k]).astype(np.int64) != want[k])[0]
        assert len(bad) == 0, f"{what} {k}: paths {bad[:5]} differ: {np.asarray(got[k])[bad[:5]]} vs {want[k][bad[:5]]}"
    a, b = np.asarray(got["cost"], np.float64), want["cost"]
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what} cost: NaN pattern differs"
    lim = (want["cost_n"] + 16.0) * 2.0 ** -52 * want["cost_abs"]
    err = np.where(np.isnan(b), 0.0, np.abs(a - b))
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{what}: cost, worst error / bound {np.nanmax(np.where(lim > 0, err / lim, 0.0), initial=0.0):.3g}")
    bad = np.argwhere(err > lim)
    assert len(bad) == 0, f"{what} cost: {len(bad)} entries beyond the bound, first {bad[:3].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def host_call(m, w, off, b, par, in_place=False):
    """fiesta_hip_path_refine through ctypes, every output pre-filled with the sentinel"""
    from fiesta_amd._lib import RefineParams, RefineResult, check
    from fiesta_amd.esdf_map import REFINE_FIELDS
    w = np.ascontiguousarray(w, np.float64).copy()
    n = len(off) - 1
    out = {name: np.full((n if per == "path" else len(w),) + shape, SENTINEL, dt) for name, dt, per, shape in REFINE_FIELDS}
    if in_place:
        out["waypoints"] = w
    res = RefineResult(*[out[name].ctypes.data for name, _, _, _ in REFINE_FIELDS])
    p = RefineParams(par["margin"], par["w_obstacle"], par["w_smooth"], par["alpha"], par["max_step"], par["tolerance"], par["iterations"], 0)
    check(m._lib.fiesta_hip_path_refine(m._h, w.ctypes.data_as(C.c_void_p), len(w), off.ctypes.data_as(C.c_void_p), n,
                                        None if b is None else b.ctypes.data_as(C.c_void_p), C.byref(p), C.byref(res)))
    return out


def device_call(m, w, off, b, par, in_place=False):
    """fiesta_hip_path_refine_dev on torch tensors; every output pre-filled with the sentinel"""
    import torch
    from fiesta_amd.esdf_map import REFINE_FIELDS
    dev = torch.device("cuda", 0)
    tdt = {np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32}
    wt, ot = torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(dev)
    bt = None if b is None else torch.from_numpy(np.ascontiguousarray(b, np.float64)).to(dev)
    outs = {name: torch.full(((len(off) - 1) if per == "path" else len(w),) + shape, SENTINEL, dtype=tdt[dt], device=dev)
            for name, dt, per, shape in REFINE_FIELDS}
    if in_place:
        outs["waypoints"] = wt
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the copies and fills above must have landed)
    m.PathRefineDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, 0 if bt is None else bt.data_ptr(),
                       out={k: v.data_ptr() for k, v in outs.items()}, **par)
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.fixture(scope="module", params=["dense", "hash"])
def store(request, hip_lib):
    if request.param == "dense":
        m, _ = dense_map(48, obstacles=160, seed=3)
        lo, hi = (0.0, 0.0, 0.0), (4.8, 4.8, 4.8)
    else:
        m, _ = hash_map_scene()
        lo, hi = (-2.0, -2.0, -1.0), (4.0, 3.0, 2.0)
    w, off, special = make_batch(lo, hi, 5)
    yield m, w, off, special
    m.close()


CASES = [(0, 0.0, "finite"), (1, 0.0, "none"), (2, 0.0, "mixed"), (17, 0.0, "finite"), (17, 0.0, "none"), (17, 0.0, "mixed"),
         (17, 0.001, "none"), (17, 0.001, "mixed")]


def test_the_length_boundaries_equal_the_model(store):
    m, w, off, special = store
    lens = np.diff(off)
    for iterations, tol, kind in CASES:
        par = dict(PAR, iterations=iterations, tolerance=tol)
        b = make_bounds(w, off, special, kind, 9)
        want = expected(m, w, off, b, par)
        what = f"{iterations} iterations, tolerance {tol}, bounds {kind}"
        inv = want["status"] == 1
        assert inv[special["nan"]] and inv[lens == 1025].all() and inv[special["lo_gt_hi"]] == (kind != "none")
        assert inv.sum() == 3 + (kind != "none")
        assert_equals_model(host_call(m, w, off, b, par), want, "host: " + what)
        assert_equals_model(device_call(m, w, off, b, par), want, "device: " + what)
        moving = ~inv & (lens > 2)
        if iterations == 17 and tol == 0.0 and kind == "none":
            assert (np.abs(want["waypoints"] - w)[np.isfinite(w).all(axis=1)] > 0.05).any() and (want["n_below"][~inv] > 0).any()
            assert (want["iterations"][moving] == 17).all()
        if tol > 0:   # some paths stop early, some run all the way
            its = want["iterations"][moving]
            assert (its < 17).sum() >= 5 and (its == 17).sum() >= 5, its


def test_device_offsets_in_place_and_path_order(store):
    m, w, off, special = store
    par = dict(PAR, iterations=6, tolerance=0.0)
    b = make_bounds(w, off, special, "mixed", 9)
    good = device_call(m, w, off, b, par)
    # in place: result.waypoints is the input pointer
    for call in (host_call, device_call):
        same = call(m, w, off, b, par, in_place=True)
        for k in FLOATS + INTS + ("cost",):
            assert np.array_equal(bits(same[k]) if same[k].dtype == np.float64 else same[k], bits(good[k]) if good[k].dtype == np.float64 else good[k]), (call.__name__, k)
    # broken device offsets: a swapped pair, entries out of range, a shifted boundary; the flagged paths are INVALID, the others exact
    n = len(off) - 1
    bad = off.copy()
    bad[5], bad[6] = off[6], off[5]
    bad[20] = len(w) + 5
    bad[30] = -3
    bad[40] = off[40] + 2                                   # path 39 grows by two rows, path 40 starts two rows late
    flagged = flagged_paths(bad, len(w))
    in_valid = np.zeros(len(w), bool)
    for p in np.nonzero(~flagged)[0]:
        in_valid[bad[p]:bad[p + 1]] = True
    assert (~in_valid).sum() >= 10                          # rows that belong to no valid path: they must come back as they went in
    assert 3 <= flagged.sum() <= 12 and not flagged[39] and not flagged[0]
    want = expected(m, w, bad, b, par, device_offsets=True)
    got = device_call(m, w, bad, b, par)
    assert_equals_model(got, want, "device, broken offsets")
    assert (got["status"][flagged] == 1).all() and np.array_equal(bits(got["waypoints"][~in_valid]), bits(w[~in_valid]))
    # the same batch in another order of paths: the same bits per path, cost included (its order of summation follows the length)
    perm = np.random.RandomState(2).permutation(n)
    rows = np.concatenate([np.arange(off[p], off[p + 1]) for p in perm]).astype(np.int64)
    off2 = np.concatenate([[0], np.cumsum(np.diff(off)[perm])]).astype(np.int64)
    other = device_call(m, w[rows], off2, b[rows], par)
    assert np.array_equal(bits(other["waypoints"]), bits(good["waypoints"][rows]))
    for k in ("cost", "last_move", "min_dist"):
        assert np.array_equal(bits(other[k]), bits(good[k][perm])), k
    for k in INTS:
        assert np.array_equal(other[k], good[k][perm]), k
    # and through the Python class
    cls = m.PathRefine(w, off, b, **par)
    for k in FLOATS + ("cost",):
        assert np.array_equal(bits(cls[k]), bits(good[k])), k


def test_a_wall_pushes_a_path_away_and_optional_outputs(hip_lib):
    """a straight path along a wall, inside the margin: every interior waypoint moves away from the wall, J falls; NULL outputs are
    not written; n_paths = 0 does nothing"""
    from fiesta_amd._lib import RefineParams, RefineResult
    m = wall_map(32, 0.1, wall_y=10)
    w = np.stack([np.linspace(0.6, 2.6, 21), np.full(21, 1.35), np.full(21, 1.6)], axis=1)
    off = np.array([0, 21], np.int64)
    par = dict(margin=0.6, w_obstacle=1.0, w_smooth=0.2, alpha=0.05, max_step=0.05, tolerance=0.0, iterations=20)
    got = m.PathRefine(w, off, None, **par)
    assert got["status"][0] == 0 and got["iterations"][0] == 20 and got["cost"][0, 1] < 0.5 * got["cost"][0, 0]
    assert (got["waypoints"][1:-1, 1] > w[1:-1, 1] + 0.05).all() and np.array_equal(bits(got["waypoints"][[0, -1]]), bits(w[[0, -1]]))
    assert got["min_dist"][0] == m.GetDistWithGradTrilinear(w[:1])[0][0]           # the ends stay closest
    cost = np.full((1, 2), -7.0)
    res = RefineResult(None, cost.ctypes.data, None, None, None, None, None)
    p = RefineParams(*[par[k] for k in ("margin", "w_obstacle", "w_smooth", "alpha", "max_step", "tolerance", "iterations")], 0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert m._lib.fiesta_hip_path_refine(m._h, vp(w), 21, vp(off), 1, None, C.byref(p), C.byref(res)) == 0
    assert np.array_equal(bits(cost), bits(got["cost"]))
    cost[:] = -7.0
    assert m._lib.fiesta_hip_path_refine(m._h, vp(w), 0, vp(np.zeros(1, np.int64)), 0, None, C.byref(p), C.byref(res)) == 0
    assert (cost == -7.0).all()
    assert m._lib.fiesta_hip_path_refine(m._h, vp(w), 21, vp(off), 1, None, C.byref(RefineParams(0.6, 1.0, 0.2, 0.0, 0.05, 0.0, 20, 0)), C.byref(res)) == 1
    assert m.GetDistWithGradTrilinear(w[:1])[0][0] > 0                              # the map stays usable
    m.close()


def test_refined_corridor_paths_stay_in_observed_free_space(hip_lib):
    """reach paths -> corridors -> corridor_bounds -> refinement on a partially observed map, without the model: for every path whose
    corridor is whole (`ok`), every voxel that path clearance's sample rule visits along the REFINED polyline, at a step of half a
    voxel, is observed and free"""
    import fiesta_amd
    from test_cpp_reach import example_scene
    m = example_scene()                                     # one view cone, a wall, a pillar; everything else never observed
    res, origin = 0.2, np.array([-4.0, -4.0, 0.0])
    fv, _ = m.GetFrontierVoxels()
    fv = np.array(sorted(fv.tolist()), np.int32)
    m.ReachField([(12, 20, 10)], want_cost=False)
    paths = m.ReachPaths(fv)                                 # raw: one waypoint per move
    # the corridor window cuts the map at z = 13: the paths that climb above it are BLOCKED there, their corridors are not whole
    cor = m.PathCorridor(paths["waypoints_vox"], paths["offsets"], lo=(0, 0, 0), hi=(39, 39, 13), max_grow=8)
    bounds, ok = fiesta_amd.corridor_bounds(paths["waypoints_vox"], paths["offsets"], cor)
    assert (~ok).sum() >= 1 and ok.sum() >= 100
    off, w = paths["offsets"], paths["waypoints_pos"]
    got = m.PathRefine(w, off, bounds, margin=0.8, w_obstacle=1.0, w_smooth=2.0, alpha=0.02, max_step=0.05, iterations=64)
    assert (got["status"] == 0).all()
    f = m.download_field(("d2", "occ"))
    free = ((f["d2"] >= 0) & (f["occ"] == 0)).reshape(m.grid_size)
    keep = np.repeat(ok, np.diff(off))
    sub_off = np.concatenate([[0], np.cumsum(np.diff(off)[ok])]).astype(np.int64)
    pos, ns = fiesta_amd.path_samples(got["waypoints"][keep], sub_off, 0.5 * res)
    vox = np.floor((pos - origin) / res).astype(np.int64)
    assert (ns >= 0).all() and (vox >= 0).all() and (vox < m.grid_size).all()
    bad = ~free[vox[:, 0], vox[:, 1], vox[:, 2]]
    assert len(pos) > 10 * ok.sum() and not bad.any(), f"{bad.sum()} of {len(pos)} samples in voxels that are not observed free, first at {pos[bad][:3]}"
    ends = np.zeros(len(w), bool)
    ends[off[:-1][np.diff(off) > 0]] = ends[off[1:][np.diff(off) > 0] - 1] = True
    assert ((got["waypoints"] >= bounds[:, :3]) & (got["waypoints"] <= bounds[:, 3:]))[~ends].all()
    assert np.array_equal(bits(got["waypoints"][ends]), bits(w[ends]))
    moved = np.abs(got["waypoints"] - w).max(axis=1)
    far = np.zeros(len(ok))
    np.maximum.at(far, np.repeat(np.arange(len(ok)), np.diff(off)), moved)
    print(f"{ok.sum()} of {len(ok)} corridors whole; the largest move on a whole one {far[ok].max():.3f} m; J {np.nansum(got['cost'][:, 0]):.4g} -> {np.nansum(got['cost'][:, 1]):.4g}")
    assert far[ok].max() > res                               # some path in a whole corridor moved by more than a voxel
    m.close()
