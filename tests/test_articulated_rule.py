"""CPU side of the articulated body queries (fiesta_hip_articulated_query, include/fiesta_hip.h): the definition.

fiesta_amd.articulated_query_model is the model the GPU tests compare the kernel with, so it must be the header's rule.  Here it is
checked against a literal triple loop over configurations, frames and spheres (Python floats, one operation per line of the header),
against fiesta_amd.body_query_model where the two must agree (one frame; every frame at the same pose), its per-frame derivatives
against central differences of its own cost on a smooth analytic field, empty frames, invalid frame poses, every argument error and
the grouping helper.  Pure Python but for the last test, which needs the built library to look the two symbols up.
"""
import math

import numpy as np
import pytest

from fiesta_amd.articulated_model import articulated_query_model, group_spheres_by_frame
from fiesta_amd.body_model import body_query_model

from test_body_rule import C0, point_field, random_body, random_poses, rotated

EXACT = ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "frame_clearance", "sphere_clearance")
SUMS = ("cost", "frame_cost", "frame_grad")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_bits(got, want, keys, what=""):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{what} {k}: bits differ"


def assert_within(a, b, n, A, what=""):
    """|a - b| <= (n + 16) * 2^-52 * A, NaN exactly where b has it"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    lim = (np.asarray(n, np.float64) + 16.0) * 2.0 ** -52 * np.asarray(A, np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), what
    err = np.where(np.isnan(b), 0.0, np.abs(a - b))
    assert np.all(err <= lim), (what, float(err.max()))


def assert_sums(got, model, what=""):
    assert_within(got["cost"], model["cost"], model["cost_n"], model["cost_abs"], what + " cost")
    assert_within(got["frame_cost"], model["frame_cost"], model["frame_cost_n"], model["frame_cost_abs"], what + " frame_cost")
    assert_within(got["frame_grad"], model["frame_grad"], model["frame_grad_n"][:, :, None], model["frame_grad_abs"], what + " frame_grad")


def rotation_of(pose):
    """the header's pose rule for one pose in Python floats: (R, p) or None for an invalid pose"""
    px, py, pz, qw, qx, qy, qz = (float(v) for v in pose)
    if not all(math.isfinite(v) for v in (px, py, pz, qw, qx, qy, qz)):
        return None
    s = ((qw * qw + qx * qx) + qy * qy) + qz * qz
    if not s > 0:
        return None
    k = 2.0 / s
    if not math.isfinite(k):
        return None
    xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
    R = [[1.0 - k * (yy + zz), k * (xy - wz), k * (xz + wy)],
         [k * (xy + wz), 1.0 - k * (xx + zz), k * (yz - wx)],
         [k * (xz - wy), k * (yz + wx), 1.0 - k * (xx + yy)]]
    return R, (px, py, pz)


def loop_model(query, spheres, frame, F, poses, margin):
    """the header's rule, configuration by configuration, frame by frame, sphere by sphere; the sums in sphere order"""
    N, K = len(poses), len(spheres)
    out = {"min_clearance": np.full(N, np.nan), "min_sphere": np.full(N, -1, np.int32), "min_pos": np.full((N, 3), np.nan),
           "min_grad": np.full((N, 3), np.nan), "n_below": np.full(N, -1, np.int32), "cost": np.full(N, np.nan),
           "frame_clearance": np.full((N, F), np.nan), "frame_cost": np.full((N, F), np.nan), "frame_grad": np.zeros((N, F, 6)),
           "sphere_clearance": np.full((N, K), np.nan)}
    for n in range(N):
        tfs = [rotation_of(poses[n, f]) for f in range(F)]
        if any(tf is None for tf in tfs):
            continue
        best, best_i, nb, cost = None, -1, 0, 0.0
        for f in range(F):
            R, p = tfs[f]
            fmin, fcost, fgrad = math.inf, 0.0, [0.0] * 6
            for i in range(K):
                if frame[i] != f:
                    continue
                cx, cy, cz, r = (float(v) for v in spheres[i])
                a = [(R[c][0] * cx + R[c][1] * cy) + R[c][2] * cz for c in range(3)]
                x = [p[c] + a[c] for c in range(3)]
                d, g = query(np.array([x]))
                d, g = float(d[0]), [float(v) for v in g[0]]
                si = d - r
                if si < margin:
                    e = margin - si
                    phi, psi = e * e, -2.0 * e
                    gam = [psi * g[c] for c in range(3)]
                    nb += 1
                else:
                    phi, gam = 0.0, [0.0, 0.0, 0.0]
                t = [a[1] * gam[2] - a[2] * gam[1], a[2] * gam[0] - a[0] * gam[2], a[0] * gam[1] - a[1] * gam[0]]
                cost = cost + phi
                fcost = fcost + phi
                for c in range(3):
                    fgrad[c] = fgrad[c] + gam[c]
                    fgrad[3 + c] = fgrad[3 + c] + t[c]
                fmin = min(fmin, si)
                out["sphere_clearance"][n, i] = si
                if best is None or si < best or (si == best and i < best_i):
                    best, best_i = si, i
                    out["min_pos"][n], out["min_grad"][n] = x, g
            out["frame_clearance"][n, f], out["frame_cost"][n, f], out["frame_grad"][n, f] = fmin, fcost, fgrad
        out["min_clearance"][n], out["min_sphere"][n], out["n_below"][n], out["cost"][n] = best, best_i, nb, cost
    return out


def frames_for(rng, K, F):
    """a non-decreasing frame index per sphere, frames of uneven size, some possibly empty"""
    return np.sort(rng.randint(0, F, K)).astype(np.int32)


def frame_poses(rng, N, F, spread=0.3):
    return random_poses(rng, N * F, spread).reshape(N, F, 7)


@pytest.mark.parametrize("K,F", [(1, 1), (3, 2), (8, 8), (70, 5)])
def test_model_equals_the_literal_loop(K, F):
    rng = np.random.RandomState(K + F)
    sph, frm, poses = random_body(rng, K), frames_for(rng, K, F), frame_poses(rng, 30, F)
    poses[7, F - 1, 3:] = 0.0           # a zero quaternion in the last frame
    poses[11, 0, 1] = np.nan
    for margin in (2.6, 0.0, 50.0):   # some spheres below, none, all
        got, want = articulated_query_model(point_field, sph, frm, F, poses, margin), loop_model(point_field, sph, frm, F, poses, margin)
        assert_bits(got, want, EXACT, f"K {K} F {F} margin {margin}")
        assert_sums(want, got, f"K {K} F {F} margin {margin}")
        ok = ~np.isnan(want["cost"])
        assert ok.sum() == 28 and (got["cost_n"] == K).all() and np.array_equal(got["frame_cost_n"][0], np.bincount(frm, minlength=F))
        assert np.array_equal(got["frame_grad_n"], got["frame_cost_n"]) and np.all(got["frame_grad_abs"][ok] >= np.abs(got["frame_grad"][ok]))
    assert want["n_below"][ok].min() == K and got["cost"][ok].min() > 0     # margin 50: every sphere is below


def test_one_frame_is_the_rigid_model():
    rng = np.random.RandomState(21)
    for K in (1, 5, 70):
        sph, poses = random_body(rng, K), random_poses(rng, 40)
        poses[3, 3:] = 0.0
        rigid = body_query_model(point_field, sph, poses, 2.6)
        got = articulated_query_model(point_field, sph, np.zeros(K, np.int32), 1, poses[:, None, :], 2.6)
        assert_bits(got, rigid, ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "sphere_clearance"), f"K {K}")
        assert np.array_equal(bits(got["frame_clearance"][:, 0]), bits(rigid["min_clearance"]))
        assert_within(got["cost"], rigid["cost"], K, rigid["cost_abs"], "cost")
        assert_within(got["frame_cost"][:, 0], rigid["cost"], K, rigid["cost_abs"], "frame_cost")
        assert_within(got["frame_grad"][:, 0], rigid["grad"], K, rigid["grad_abs"], "frame_grad")
        assert np.nanmax(rigid["cost"]) > 0


def test_every_frame_at_the_same_pose_is_the_rigid_model():
    rng = np.random.RandomState(22)
    K, F = 40, 6
    sph, frm, poses = random_body(rng, K), frames_for(rng, K, F), random_poses(rng, 25)
    rigid = body_query_model(point_field, sph, poses, 2.6)
    got = articulated_query_model(point_field, sph, frm, F, np.repeat(poses[:, None, :], F, axis=1), 2.6)
    assert_bits(got, rigid, ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "sphere_clearance"))
    assert np.array_equal(bits(got["frame_clearance"].min(axis=1)), bits(rigid["min_clearance"]))
    assert_within(got["frame_grad"].sum(axis=1), rigid["grad"], K, rigid["grad_abs"], "sum of frame_grad")
    assert_within(got["frame_cost"].sum(axis=1), rigid["cost"], K, rigid["cost_abs"], "sum of frame_cost")
    assert_within(got["cost"], rigid["cost"], K, rigid["cost_abs"], "cost")
    assert np.abs(rigid["grad"]).max() > 0.1


def test_frame_grad_agrees_with_central_differences_of_the_cost():
    """One frame's position or rotation perturbed, the others fixed: only that frame's spheres move, each exactly as a rigid body's
    do, so the bound of test_body_rule.py's derivative test holds with the same step h and the same tolerance (written for K moving
    spheres and a cost of K terms; here at most K move and the cost has K terms)."""
    rng = np.random.RandomState(5)
    K, F, margin, h = 8, 3, 5.0, 1e-5
    E = margin + 0.2 - 2.0
    tol = h * h / 6.0 * K * (9.0 + 6.5 * E) + (K + 16) * 2.0 ** -52 * K * E * E / h
    assert tol < 1e-7
    sph, frm = random_body(rng, K), np.array([0, 0, 0, 1, 1, 2, 2, 2], np.int32)
    poses = frame_poses(rng, 6, F, spread=0.15)
    assert np.linalg.norm(C0) - 1.0 - np.sqrt(3) * 0.15 >= 2.0
    base = articulated_query_model(point_field, sph, frm, F, poses, margin)
    assert (base["n_below"] == K).all()
    worst = 0.0
    for n in range(len(poses)):
        for f in range(F):
            for c in range(3):
                u = np.zeros(3)
                u[c] = h
                four = np.repeat(poses[n][None], 4, axis=0)
                four[0, f, :3] += u
                four[1, f, :3] -= u
                four[2, f], four[3, f] = rotated(poses[n, f], u), rotated(poses[n, f], -u)
                both = articulated_query_model(point_field, sph, frm, F, four, margin)["cost"]
                for fd, an in (((both[0] - both[1]) / (2 * h), base["frame_grad"][n, f, c]),
                               ((both[2] - both[3]) / (2 * h), base["frame_grad"][n, f, 3 + c])):
                    worst = max(worst, abs(fd - an))
                    assert abs(fd - an) <= tol, (n, f, c, fd, an, tol)
    print(f"worst |central difference - frame_grad| {worst:.3g}, tolerance {tol:.3g}")
    assert np.abs(base["frame_grad"]).min() > 1e-4      # against an empty test: the derivatives are far from 0


def test_empty_frames_first_in_the_middle_and_last():
    rng = np.random.RandomState(6)
    sph, frm, F = random_body(rng, 3), np.array([1, 1, 3], np.int32), 5
    poses = frame_poses(rng, 9, F)
    r = articulated_query_model(point_field, sph, frm, F, poses, 50.0)
    for f in (0, 2, 4):
        assert np.all(r["frame_clearance"][:, f] == np.inf) and not r["frame_cost"][:, f].any() and not r["frame_grad"][:, f].any()
        assert not r["frame_cost_n"][:, f].any() and not r["frame_grad_abs"][:, f].any()
    assert np.all(np.isfinite(r["frame_clearance"][:, [1, 3]])) and np.all(r["frame_cost"][:, [1, 3]] > 0)
    assert_bits(r, loop_model(point_field, sph, frm, F, poses, 50.0), EXACT + SUMS)


def invalid_patterns():
    good = np.array([0.1, -0.2, 0.3, 0.5, -0.5, 0.5, 0.5])
    out = []
    for slot, bad in ((0, np.nan), (2, np.inf), (3, -np.inf), (6, np.nan)):
        p = good.copy()
        p[slot] = bad
        out.append((f"slot {slot} {bad}", p))
    out.append(("zero quaternion", np.array([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 0.0])))
    out.append(("s underflows to 0", np.array([0.1, -0.2, 0.3, 1e-200, 0.0, 0.0, 1e-200])))
    out.append(("k overflows", np.array([0.1, -0.2, 0.3, 1e-160, 0.0, 0.0, 0.0])))
    return out


@pytest.mark.parametrize("what,pose", invalid_patterns(), ids=[w for w, _ in invalid_patterns()])
@pytest.mark.parametrize("frame", [0, 1, 2])
def test_one_invalid_frame_voids_its_configuration_only(what, pose, frame):
    """frame 1 owns no sphere: its pose counts all the same"""
    rng = np.random.RandomState(9)
    sph, frm, F = random_body(rng, 5), np.array([0, 0, 2, 2, 2], np.int32), 3
    good = frame_poses(rng, 4, F)
    alone = articulated_query_model(point_field, sph, frm, F, good, 3.0)
    spoilt = good[1].copy()
    spoilt[frame] = pose
    poses = np.stack([good[0], spoilt, good[1], good[2], spoilt, good[3]])
    r = articulated_query_model(point_field, sph, frm, F, poses, 3.0)
    keep = [0, 2, 3, 5]
    assert_bits({k: r[k][keep] for k in EXACT + SUMS}, alone, EXACT + SUMS, what)
    for n in (1, 4):
        assert np.isnan(r["min_clearance"][n]) and np.isnan(r["cost"][n]) and np.isnan(r["min_pos"][n]).all() and np.isnan(r["min_grad"][n]).all()
        assert np.isnan(r["sphere_clearance"][n]).all() and np.isnan(r["frame_clearance"][n]).all() and np.isnan(r["frame_cost"][n]).all()
        assert r["min_sphere"][n] == -1 and r["n_below"][n] == -1 and not r["frame_grad"][n].any()


def test_the_argument_rules():
    sph = np.array([[0.3, 0.0, 0.0, 0.1], [0.0, 0.2, 0.0, 0.05]])
    frm = np.array([0, 1], np.int32)
    one = np.array([[[0, 0, 0, 1.0, 0, 0, 1.0], [0.5, 0, 0, 1.0, 0, 0, 0]]])
    articulated_query_model(point_field, sph, frm, 2, one, 1.0)
    bad = [(np.zeros((0, 4)), np.zeros(0, np.int32), 2, one, 1.0),                       # n_spheres 0
           (np.zeros((1025, 4)), np.zeros(1025, np.int32), 2, one, 1.0),                 # n_spheres 1025
           (sph[:1], frm[:1], 0, np.zeros((1, 0, 7)), 1.0),                              # n_frames 0
           (sph, frm, 65, np.tile(one[:, :1], (1, 65, 1)), 1.0),                         # n_frames 65
           ([[0, 0, 0, -0.1], [0, 0, 0, 0.1]], frm, 2, one, 1.0),                        # a negative radius
           ([[np.nan, 0, 0, 0.1], [0, 0, 0, 0.1]], frm, 2, one, 1.0),                    # a centre that is not finite
           ([[0, 0, 0, np.inf], [0, 0, 0, 0.1]], frm, 2, one, 1.0),                      # a radius that is not finite
           (sph, [0, 2], 2, one, 1.0),                                                   # a frame index past the last frame
           (sph, [-1, 0], 2, one, 1.0),                                                  # a negative frame index
           (sph, [1, 0], 2, one, 1.0),                                                   # not grouped by frame
           (sph, frm, 2, one, np.nan), (sph, frm, 2, one, np.inf)]                       # margin
    for args in bad:
        with pytest.raises(ValueError):
            articulated_query_model(point_field, *args)
    with pytest.raises(ValueError, match="frame index"):
        articulated_query_model(point_field, sph, [0, 2], 2, one, 1.0)
    with pytest.raises(ValueError, match="not grouped by frame"):
        articulated_query_model(point_field, sph, [1, 0], 2, one, 1.0)
    empty = articulated_query_model(point_field, sph, frm, 2, np.zeros((0, 2, 7)), 1.0)
    assert empty["cost"].shape == (0,) and empty["frame_grad"].shape == (0, 2, 6) and empty["frame_clearance"].shape == (0, 2)
    assert empty["sphere_clearance"].shape == (0, 2)


def test_group_spheres_by_frame_is_stable_and_its_order_maps_results_back():
    rng = np.random.RandomState(12)
    K, F = 23, 4
    sph, frm = random_body(rng, K), rng.randint(0, F, K).astype(np.int32)
    assert np.any(np.diff(frm) < 0)
    with pytest.raises(ValueError):
        articulated_query_model(point_field, sph, frm, F, frame_poses(rng, 1, F), 1.0)
    gs, gf, order = group_spheres_by_frame(sph, frm)
    assert np.all(np.diff(gf) >= 0) and np.array_equal(gs, sph[order]) and np.array_equal(gf, frm[order])
    assert sorted(order.tolist()) == list(range(K))
    for f in range(F):
        assert np.all(np.diff(order[gf == f]) > 0)          # stable: a frame's spheres keep their order
    poses = frame_poses(rng, 10, F)
    r = articulated_query_model(point_field, gs, gf, F, poses, 2.6)
    back = np.empty_like(r["sphere_clearance"])
    back[:, order] = r["sphere_clearance"]
    for j in range(K):                                       # sphere j of the caller's table, asked alone
        alone = articulated_query_model(point_field, sph[j:j + 1], frm[j:j + 1], F, poses, 2.6)
        assert np.array_equal(bits(back[:, j]), bits(alone["sphere_clearance"][:, 0])), j
    assert np.array_equal(back[np.arange(10), order[r["min_sphere"]]], r["min_clearance"])


def test_both_symbols_are_declared_and_bound():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    lib = fiesta_amd.load()
    declared = _lib.declared_symbols()
    text = open(_lib.HEADER_PATH).read()
    for name in ("fiesta_hip_articulated_query", "fiesta_hip_articulated_query_dev"):
        assert name in declared and name in lib._fiesta_signatures and hasattr(lib, name)
        assert f"int {name}(fiesta_hip_map *m, const double *spheres, const int32_t *sphere_frame, int32_t n_spheres" in text
    assert "#define FIESTA_HIP_BODY_MAX_FRAMES 64" in text and fiesta_amd.BODY_MAX_FRAMES == 64
    assert [f[0] for f in _lib.ArticulatedResult._fields_] == [n for n, _, _ in fiesta_amd.esdf_map.ARTICULATED_FIELDS]
    assert lib.fiesta_hip_version() == 101
