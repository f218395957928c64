"""The rule of fiesta_hip_view_coverage on the CPU: fiesta_amd.view_coverage_model (the definition the device call has to reproduce
bit for bit) against a literal per-pair restatement over the EXISTING ray_query_model, the inclusive field-of-view and range
boundaries, OMNI, the tie rule of best_view, min_visible, the ring form, the whole-call errors (they need no device), and the
resource usage of the built kernels."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE, OCC, UNK, OUT = 0, 1, 2, 4
RES = 0.25                       # a power of two: voxel centres, their differences and products are exact


def literal(obs, occ, origin, vox, pos, dirs, group, offsets, members, n_eff, sensor, omni):
    """the contract once more, pair by pair in Python floats; a pair is visible iff the ray query pos -> centre with
    stop_mask = block_mask has hit_index == -1 or hit_vox == the target"""
    from fiesta_amd import ray_query_model
    V, n, G = len(pos), len(vox), len(offsets) - 1
    org = np.asarray(origin, np.float64)
    own = ray_query_model(obs, occ, origin, RES, pos, pos, 7)                    # W = [the view's voxel]
    finite = np.isfinite(pos).all(1)
    usable = [bool(finite[v] and own["n_visited"][v] == 1 and own["hit_index"][v] == -1 and 0 <= group[v] < n_eff) for v in range(V)]
    pairs, S, E = [], [], []
    for v in range(V):
        if not usable[v]:
            continue
        for m in members[offsets[group[v]]:offsets[group[v] + 1]]:
            if not 0 <= m < n:
                pairs.append((v, -1, False))
                continue
            p = [(float(vox[m][c]) + 0.5) * RES + float(org[c]) for c in range(3)]
            q0, q1, q2 = (p[c] - float(pos[v][c]) for c in range(3))
            d2 = q0 * q0 + q1 * q1 + q2 * q2
            ok = sensor["min_range"] * sensor["min_range"] <= d2 <= sensor["max_range"] * sensor["max_range"]
            if ok and omni:
                h = math.sqrt(q0 * q0 + q1 * q1)
                ok = abs(q2) <= (sensor["tan_v"] * h if not (math.isinf(sensor["tan_v"]) and h == 0) else math.nan)
            elif ok:
                dx, dy = float(dirs[v][0]), float(dirs[v][1])
                fwd, lat = q0 * dx + q1 * dy, q1 * dx - q0 * dy
                ok = fwd > 0 and abs(lat) <= sensor["tan_h"] * fwd and abs(q2) <= sensor["tan_v"] * fwd
            pairs.append((v, int(m), ok))
            if ok:
                S.append(pos[v]), E.append(p)
    rq = ray_query_model(obs, occ, origin, RES, np.array(S).reshape(-1, 3), np.array(E).reshape(-1, 3), sensor["block_mask"])
    want = {"n_in_view": np.where(usable, 0, -1).astype(np.int32), "n_visible": np.where(usable, 0, -1).astype(np.int32),
            "cover_count": np.zeros(n, np.int32), "first_view": np.full(n, -1, np.int32), "best_view": np.full(G, -1, np.int64),
            "best_count": np.zeros(G, np.int32), "n_usable": sum(usable), "n_pairs": len(pairs), "pairs_in_view": len(S), "pairs_visible": 0}
    k = 0
    for v, m, ok in pairs:
        if not ok:
            continue
        want["n_in_view"][v] += 1
        seen = rq["n_visited"][k] >= 1 and (rq["hit_index"][k] == -1 or rq["hit_vox"][k].tolist() == list(vox[m]))
        k += 1
        if seen:
            want["n_visible"][v] += 1
            want["cover_count"][m] += 1
            want["pairs_visible"] += 1
            if want["first_view"][m] < 0:
                want["first_view"][m] = v
    for g in range(G):
        for v in range(V):
            if usable[v] and group[v] == g and want["n_visible"][v] >= sensor["min_visible"] and want["n_visible"][v] > want["best_count"][g]:
                want["best_view"][g], want["best_count"][g] = v, want["n_visible"][v]
    return want


def assert_equal(got, want, what=""):
    for k, w in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(w)), (what, k, got[k], w)


def random_scene(seed):
    rng = np.random.default_rng(seed)
    shape = (14, 12, 10)
    origin = (-1.0, 0.5, -0.25)                                                  # whole voxels: a target's walk voxel is its map voxel
    obs = rng.random(shape) < 0.8
    obs[5:8, :, :] &= rng.random((3,) + shape[1:]) < 0.5
    occ = obs & (rng.random(shape) < 0.08)
    ov = np.array([-1, 0, -1])                                                   # targets beyond the array too
    vox = rng.integers(ov, np.array(shape) + 1, (90, 3))
    V = 40
    pos = np.asarray(origin) + rng.random((V, 3)) * np.array(shape) * RES * 1.1 - 0.1
    free = np.argwhere(obs & ~occ)
    pos[:30] = np.asarray(origin) + (free[rng.integers(0, len(free), 30)] + rng.random((30, 3))) * RES     # most views stand in free space
    pos[3, 1], pos[4, 0] = np.nan, np.inf
    ang = rng.random(V) * 2 * np.pi
    dirs = np.stack([np.cos(ang), np.sin(ang)], 1)
    offsets = np.array([0, 30, 30, 75, 100])
    members = rng.integers(0, len(vox), 100)
    members[[5, 40]] = [-1, len(vox)]                                            # out of range: no pair
    group = rng.integers(0, 4, V)
    group[[7, 8]] = [-1, 4]
    return obs, occ, origin, vox, pos, dirs, group, offsets, members


@pytest.mark.parametrize("omni", (False, True))
@pytest.mark.parametrize("block_mask", (1, 3, 7))
def test_model_against_a_literal_restatement_over_the_ray_query_model(block_mask, omni):
    from fiesta_amd import view_coverage_model
    obs, occ, origin, vox, pos, dirs, group, offsets, members = random_scene(11)
    # the precondition of "hit_vox == the target": the walk ends in the target's own map voxel
    from fiesta_amd import ray_query_model
    c = (vox + 0.5) * RES + np.asarray(origin)
    assert (ray_query_model(np.zeros_like(obs), occ, origin, RES, c, c, 7)["hit_vox"] == vox).all()
    sensor = dict(min_range=0.3, max_range=2.2, tan_h=math.tan(math.radians(50)), tan_v=math.tan(math.radians(35)), block_mask=block_mask,
                  min_visible=2)
    for n_eff in (4, 3):
        got = view_coverage_model(obs, occ, origin, RES, vox, pos=pos, dir=None if omni else dirs, group=group, offsets=offsets, members=members,
                                  n_groups_effective=n_eff, omni=omni, **sensor)
        want = literal(obs, occ, origin, vox, pos, dirs, group, offsets, members, n_eff, sensor, omni)
        assert_equal(got, want, (block_mask, omni, n_eff))
        assert got["n_usable"] >= 15 and 0 < got["pairs_visible"] < got["pairs_in_view"] < got["n_pairs"]
        assert (got["view_class"][[3, 4]] == 0).all() and set(np.unique(got["view_class"])) >= {FREE, OCC, UNK}
    # more blockers, fewer visible pairs
    vis = [view_coverage_model(obs, occ, origin, RES, vox, pos=pos, dir=dirs, group=group, offsets=offsets, members=members,
                               **dict(sensor, block_mask=b))["pairs_visible"] for b in (0, 1, 3, 7)]
    assert vis[0] > vis[1] > vis[2] >= vis[3]


def open_room(shape=(16, 16, 16)):
    return np.ones(shape, bool), np.zeros(shape, bool)


def centre(v):
    return (np.asarray(v, np.float64) + 0.5) * RES


def test_field_of_view_and_range_boundaries_are_inclusive():
    from fiesta_amd import view_coverage_model
    obs, occ = open_room()
    at = np.array([4, 8, 8])
    offs = [(3, 3, 0), (3, -3, 0), (3, 4, 0), (3, 0, 3), (3, 0, -3), (3, 0, 4), (0, 0, 0), (-3, 0, 0), (0, 3, 0), (4, 0, 0), (5, 0, 0), (2, 0, 0)]
    vox = at + np.array(offs)
    r = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre(at)], dir=[(1.0, 0.0)], tan_h=1.0, tan_v=1.0, want_pairs=True)
    #            |lat| == fwd, twice; beyond; |q2| == fwd, twice; beyond; own voxel (fwd == 0); behind; abeam; ahead x3
    assert r["pairs"][:, 3].tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1]
    assert r["n_in_view"].tolist() == [7] and r["n_visible"].tolist() == [7] and r["cover_count"].tolist() == r["pairs"][:, 3].tolist()
    # the range: 4 voxels of 0.25 m are exactly 1.0 m
    near = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre(at)], dir=[(1.0, 0.0)], tan_h=1.0, tan_v=1.0, min_range=1.0, max_range=1.0,
                               want_pairs=True)
    assert near["pairs"][:, 2].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0] and near["n_visible"].tolist() == [1]
    # a diagonal forward vector that is exact in binary: (0.6, 0.8) is not, (1, 0) rotated by 90 degrees is
    side = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre(at)], dir=[(0.0, 1.0)], tan_h=1.0, tan_v=0.0, want_pairs=True)
    assert side["pairs"][:, 3].tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0]          # tan_v = 0: only q2 == 0 passes


def test_omni():
    from fiesta_amd import view_coverage_model
    obs, occ = open_room()
    at = np.array([8, 8, 8])
    offs = [(3, 0, 3), (-3, 0, 3), (0, -3, -3), (3, 0, 4), (0, 0, 3), (0, 0, 0), (2, 2, 0), (-5, 1, 1)]
    vox = at + np.array(offs)
    r = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre(at)], omni=True, tan_v=1.0, want_pairs=True)
    assert r["pairs"][:, 3].tolist() == [1, 1, 1, 0, 0, 1, 1, 1]      # all around; straight up is outside any cone; the own voxel: 0 <= 0
    up = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre(at)], omni=True, tan_v=math.inf, want_pairs=True)
    assert up["pairs"][:, 3].tolist() == [1, 1, 1, 1, 0, 0, 1, 1]     # inf * 0 is NaN: the comparison fails
    with pytest.raises(ValueError):
        view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre(at)], tan_v=1.0)           # no dir without omni


def test_blockers_and_the_untested_last_voxel():
    from fiesta_amd import view_coverage_model
    obs, occ = open_room()
    occ[8, 4:12, 4:12] = True                  # a wall
    obs[2, 11:14, 8] = False                   # an unobserved bar, end on
    obs[2, 3, 8] = False                       # an unknown target in the open
    at = np.array([2, 8, 8])
    vox = np.array([[12, 8, 8], [8, 8, 8], [2, 11, 8], [2, 12, 8], [2, 3, 8], [3, 8, 12]])
    out = {b: view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre(at)], omni=True, block_mask=b) for b in (0, 1, 2, 3)}
    assert out[0]["cover_count"].tolist() == [1, 1, 1, 1, 1, 1]
    assert out[1]["cover_count"].tolist() == [0, 1, 1, 1, 1, 1]       # behind the wall; the wall's own voxel is a target: never tested
    assert out[2]["cover_count"].tolist() == [1, 1, 1, 0, 1, 1]       # (2, 12, 8) lies behind unknown (2, 11, 8), which itself is seen
    assert out[3]["cover_count"].tolist() == [0, 1, 1, 0, 1, 1]       # the unknown target in the open is seen
    # a view in an occupied or unknown voxel, or too close to the wall, is unusable
    dist = np.full(obs.shape, 1.0)
    dist[7, 8, 8] = 0.25
    r = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=[centre((8, 8, 8)), centre((2, 12, 8)), centre((7, 8, 8)), centre((2, 8, 8)), centre((-1, 3, 3))],
                            omni=True, min_clearance=0.3, dist=dist)
    assert r["view_class"].tolist() == [OCC, UNK, FREE, FREE, OUT] and r["n_visible"].tolist() == [-1, -1, -1, 5, -1] and r["n_usable"] == 1


def test_best_view_ties_and_min_visible():
    from fiesta_amd import view_coverage_model
    obs, occ = open_room()
    vox = np.array([[8, 8, 8], [9, 8, 8], [10, 8, 8], [8, 3, 3], [8, 4, 3]])
    offsets, members = [0, 3, 5, 5], [0, 1, 2, 3, 4]
    pos = [centre(p) for p in ((2, 8, 8), (9, 2, 8), (9, 14, 8), (4, 8, 8), (2, 3, 3), (2, 3, 3))]
    dirs = [(1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (1.0, 0.0), (1.0, 0.0)]
    group = [0, 0, 0, 0, 1, 2]
    kw = dict(pos=pos, dir=dirs, group=group, offsets=offsets, members=members, tan_h=0.5, tan_v=0.5)
    r = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, max_range=1.6, **kw)
    # view 0 is 6 to 8 voxels away (1.5, 1.75, 2.0 m): one target in range; views 1 and 2 mirror each other and see all three; view 3 too
    assert r["n_visible"].tolist() == [1, 3, 3, 3, 2, 0]
    assert r["best_view"].tolist() == [1, 4, -1] and r["best_count"].tolist() == [3, 2, 0]        # the lowest index among equals
    assert r["first_view"].tolist() == [0, 1, 1, 4, 4] and r["cover_count"].tolist() == [4, 3, 3, 1, 1]
    rev = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, max_range=1.6, **dict(kw, pos=pos[::-1], dir=dirs[::-1], group=group[::-1]))
    assert rev["best_view"].tolist() == [2, 1, -1]                                                # views 3, 2, 1 sit at 2, 3, 4 now
    three = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, max_range=1.6, min_visible=3, **kw)
    assert three["best_view"].tolist() == [1, -1, -1] and three["best_count"].tolist() == [3, 0, 0]
    four = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, max_range=1.6, min_visible=4, **kw)
    assert four["best_view"].tolist() == [-1, -1, -1] and four["n_visible"].tolist() == r["n_visible"].tolist()
    with pytest.raises(ValueError):
        view_coverage_model(obs, occ, (0, 0, 0), RES, vox, min_visible=0, **kw)


def test_ring_form_is_the_explicit_form_of_its_expansion():
    from fiesta_amd import view_coverage_model, view_ring
    ring = view_ring([0.75, 1.5], 8, [0.0, 0.5])
    assert ring.shape == (32, 5) and ring[0].tolist() == [0.75, 0.0, 0.0, -1.0, -0.0]
    assert np.allclose(ring[8 + 2], [0.0, 0.75, 0.5, 0.0, -1.0], atol=1e-15) and ring[16, 0] == 1.5
    assert np.allclose(np.hypot(ring[:, 3], ring[:, 4]), 1.0) and np.allclose(ring[:, :2], -ring[:, 3:] * np.hypot(ring[:, 0], ring[:, 1])[:, None])
    obs, occ = open_room()
    occ[8, 6:10, :] = True
    rng = np.random.default_rng(3)
    vox = rng.integers(2, 14, (40, 3))
    offsets = [0, 25, 40]
    cen = np.array([centre((6, 8, 8)) + 0.01, centre((11, 7, 6)) - 0.02])
    a = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, centroid=cen, ring=ring, offsets=offsets, tan_h=1.0, tan_v=1.0, max_range=2.0)
    pos = (cen[:, None, :] + ring[None, :, :3]).reshape(-1, 3)
    b = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=pos, dir=np.tile(ring[:, 3:], (2, 1)), group=np.repeat([0, 1], 32), offsets=offsets,
                            tan_h=1.0, tan_v=1.0, max_range=2.0)
    assert_equal(a, b)
    assert a["n_usable"] > 20 and a["pairs_visible"] > 50 and (a["best_view"] // 32).tolist() == [0, 1]
    with pytest.raises(ValueError):
        view_coverage_model(obs, occ, (0, 0, 0), RES, vox, pos=pos, centroid=cen, ring=ring, omni=True)


def test_whole_call_errors_need_no_device():
    """every whole-call error is found before the map handle is touched"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd._lib import ViewInfo, ViewResult, ViewSensor, ViewSet
    lib = fiesta_amd.load()
    vox = np.zeros((4, 3), np.int32)
    buf = np.zeros(16)
    p, d = vox.ctypes.data, buf.ctypes.data
    info, res = ViewInfo(), ViewResult()
    info.n_pairs = 77
    nan, inf = math.nan, math.inf

    def views(**kw):
        return ViewSet(**dict(dict(pos=d, dir=d, group=None, n_views=2, centroid=None, ring=None, n_ring=0), **kw))

    def sensor(**kw):
        return ViewSensor(**dict(dict(min_range=0.0, max_range=5.0, tan_h=1.0, tan_v=inf, min_clearance=0.0, block_mask=3, flags=0, min_visible=1), **kw))
    ring = dict(pos=None, dir=None, centroid=d, ring=d, n_ring=2)
    cases = [(dict(v=None), "views or sensor"), (dict(s=None), "views or sensor"), (dict(inf=None), "info is null"),
             (dict(n=-1), "entry count"), (dict(n=2 ** 24 + 1), "entry count"), (dict(G=-1), "group count"), (dict(G=2 ** 24 + 1), "group count"),
             (dict(nm=-1, mem=d), "member count"), (dict(nm=2 ** 24 + 1, mem=d), "member count"), (dict(vox=None), "vox is null"),
             (dict(v=views(centroid=d, ring=d)), "exactly one view form"), (dict(v=views(pos=None)), "exactly one view form"),
             (dict(v=views(n_views=-1)), "view count"), (dict(v=views(n_views=2 ** 24 + 1)), "view count"),
             (dict(v=views(dir=None)), "dir is null"), (dict(v=views(**dict(ring, ring=None))), "ring form"),
             (dict(v=views(**dict(ring, n_ring=-1))), "ring form"), (dict(v=views(**dict(ring, n_ring=2 ** 23)), off=d, G=3), "view count"),
             (dict(s=sensor(min_range=-1.0)), "range"), (dict(s=sensor(max_range=nan)), "range"), (dict(s=sensor(min_range=nan)), "range"),
             (dict(s=sensor(min_range=6.0)), "range"), (dict(s=sensor(tan_h=-0.1)), "tangents"), (dict(s=sensor(tan_v=nan)), "tangents"),
             (dict(s=sensor(min_clearance=nan)), "min_clearance"), (dict(s=sensor(block_mask=8)), "block_mask"),
             (dict(s=sensor(block_mask=-1)), "block_mask"), (dict(s=sensor(flags=2)), "flag"), (dict(s=sensor(min_visible=0)), "min_visible")]
    for name, extra in (("fiesta_hip_view_coverage", ()), ("fiesta_hip_view_coverage_dev", (None,))):
        fn = getattr(lib, name)
        for kw, word in cases:
            a = dict(dict(vox=p, n=4, off=None, mem=None, G=1, nm=0, v=views(), s=sensor(), inf=C.byref(info)), **kw)
            st = fn(None, a["vox"], a["n"], a["off"], a["mem"], a["G"], *extra, a["nm"], C.byref(a["v"]) if a["v"] is not None else None,
                    C.byref(a["s"]) if a["s"] is not None else None, C.byref(res), a["inf"])
            assert st == 1, (name, word, st)                                 # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
        # everything in order but the handle: the argument checks come first and pass (OMNI excuses a missing dir)
        # ... and n_members is ignored without members
        for nm in (0, -1, 2 ** 24 + 1):
            st = fn(None, p, 4, None, None, 1, *extra, nm, C.byref(views(dir=None)), C.byref(sensor(flags=1)), C.byref(res), C.byref(info))
            assert st == 1 and "null map handle" in lib.fiesta_hip_last_error().decode()
    assert info.n_pairs == 77


def test_view_kernels_use_no_scratch_and_do_not_spill():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_view_" in k}
    # (the two translation units' copies carry the same name; the view pass and the pair kernel have one instance per map kind)
    for kernel, copies in (("k_view_setup", 1), ("k_view_init", 1), ("k_view_ring", 1), ("k_view_pass", 2), ("k_view_scan", 1), ("k_view_pairs", 2),
                           ("k_view_finish", 1), ("k_view_groups", 1)):
        assert sum(kernel in k for k in res) == copies, (kernel, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
