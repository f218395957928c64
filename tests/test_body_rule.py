"""CPU side of the body queries (fiesta_hip_body_query, include/fiesta_hip.h): the definition.

fiesta_amd.body_query_model is the model the GPU tests compare the kernel with, so it must be the header's rule.  Here it is checked
against a literal double loop over poses and spheres (Python floats, one operation per line of the header), its derivatives against
central differences of its own cost on a smooth analytic field, its rotation for orthonormality, the tie rule of min_sphere and
every invalid-pose pattern.  Pure Python: nothing built is needed.
"""
import math

import numpy as np
import pytest

from fiesta_amd.body_model import body_query_model, body_rotation

EXACT = ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "sphere_clearance")
C0 = np.array([3.0, 1.2, -0.7])      # the analytic field: the distance to this point


def point_field(pos):
    """d = |x - C0| and its gradient, for an (M, 3) batch"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    v = pos - C0
    d = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return d, v / d[:, None]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_bits(got, want, keys, what=""):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{what} {k}: bits differ"


def loop_model(query, spheres, poses, margin):
    """the header's rule, pose by pose and sphere by sphere, in Python floats; the sums in sphere order"""
    N, K = len(poses), len(spheres)
    out = {"min_clearance": np.full(N, np.nan), "min_sphere": np.full(N, -1, np.int32), "min_pos": np.full((N, 3), np.nan),
           "min_grad": np.full((N, 3), np.nan), "n_below": np.full(N, -1, np.int32), "cost": np.full(N, np.nan), "grad": np.zeros((N, 6)),
           "sphere_clearance": np.full((N, K), np.nan)}
    for n in range(N):
        px, py, pz, qw, qx, qy, qz = (float(v) for v in poses[n])
        if not all(math.isfinite(v) for v in (px, py, pz, qw, qx, qy, qz)):
            continue
        s = ((qw * qw + qx * qx) + qy * qy) + qz * qz
        if not s > 0:
            continue
        k = 2.0 / s
        if not math.isfinite(k):
            continue
        xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
        R = [[1.0 - k * (yy + zz), k * (xy - wz), k * (xz + wy)],
             [k * (xy + wz), 1.0 - k * (xx + zz), k * (yz - wx)],
             [k * (xz - wy), k * (yz + wx), 1.0 - k * (xx + yy)]]
        p = (px, py, pz)
        best, best_i, nb, cost, grad = None, -1, 0, 0.0, [0.0] * 6
        for i in range(K):
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
            for c in range(3):
                grad[c] = grad[c] + gam[c]
                grad[3 + c] = grad[3 + c] + t[c]
            out["sphere_clearance"][n, i] = si
            if best is None or si < best:
                best, best_i = si, i
                out["min_pos"][n], out["min_grad"][n] = x, g
        out["min_clearance"][n], out["min_sphere"][n], out["n_below"][n], out["cost"][n], out["grad"][n] = best, best_i, nb, cost, grad
    return out


def random_body(rng, K, reach=1.0):
    c = rng.randn(K, 3)
    c *= (reach * rng.rand(K) / np.linalg.norm(c, axis=1))[:, None]
    return np.concatenate([c, rng.rand(K, 1) * 0.2], axis=1)


def random_poses(rng, N, spread=0.3):
    q = rng.randn(N, 4) * np.exp(rng.uniform(-2, 2, (N, 1)))
    return np.concatenate([rng.uniform(-spread, spread, (N, 3)), q], axis=1)


@pytest.mark.parametrize("K", [1, 3, 8, 70])
def test_model_equals_the_literal_loop(K):
    rng = np.random.RandomState(K)
    sph, poses = random_body(rng, K), random_poses(rng, 40)
    poses[7, 3:] = 0.0           # a zero quaternion
    poses[11, 1] = np.nan
    for margin in (2.6, 0.0, 50.0):   # some spheres below, none, all
        got, want = body_query_model(point_field, sph, poses, margin), loop_model(point_field, sph, poses, margin)
        assert_bits(got, want, EXACT + ("cost", "grad"), f"K {K} margin {margin}")
        ok = ~np.isnan(want["cost"])
        assert ok.sum() == 38 and (got["cost_n"] == K).all() and (got["grad_n"] == K).all()
        assert np.all(got["cost_abs"][ok] == got["cost"][ok]) and np.all(got["grad_abs"][ok] >= np.abs(got["grad"][ok]))
    assert 0 < want["n_below"][ok].min() == K and got["cost"][ok].min() > 0     # margin 50: every sphere is below


def rotated(pose, theta):
    """the pose after R <- exp([theta]x) R: the quaternion of the rotation vector theta times the pose's"""
    ang = float(np.linalg.norm(theta))
    w, v = (1.0, np.zeros(3)) if ang == 0 else (math.cos(ang / 2), math.sin(ang / 2) * np.asarray(theta) / ang)
    qw, q = pose[3], pose[4:7]
    out = np.array(pose, np.float64)
    out[3] = w * qw - v @ q
    out[4:7] = w * q + qw * v + np.cross(v, q)
    return out


def test_grad_agrees_with_central_differences_of_the_cost():
    """On the field d = |x - C0| with every sphere below the margin the cost is smooth: f = sum e^2, e = margin + r - rho(x).  Along a
    unit translation, or a unit rotation of a sphere at |a| <= A = 1 from the body origin, the path x(tau) has |x'|, |x''|, |x'''| <= 1,
    so |rho'| <= 1, |rho''| <= 1 / rho + 1, |rho'''| <= 3 / rho + 3 / rho^2 + 1, and with rho >= 2 (|C0| - A - |p| >= 2) and
    e <= E = margin + 0.2 - 2:  |f'''| <= 6 * 1.5 + 2 * E * 3.25 per sphere.  A central difference of step h is off by at most
    h^2 / 6 * K * that, plus the rounding of two costs of K terms of at most E^2 each, 2 * (K + 16) * 2^-52 * K * E^2 / (2 h)."""
    rng = np.random.RandomState(5)
    K, margin, h = 8, 5.0, 1e-5
    E = margin + 0.2 - 2.0
    tol = h * h / 6.0 * K * (9.0 + 6.5 * E) + (K + 16) * 2.0 ** -52 * K * E * E / h
    assert tol < 1e-7            # (the derivatives themselves are of order 10)
    sph, poses = random_body(rng, K), random_poses(rng, 12, spread=0.15)
    assert np.linalg.norm(C0) - 1.0 - np.sqrt(3) * 0.15 >= 2.0
    base = body_query_model(point_field, sph, poses, margin)
    assert (base["n_below"] == K).all()
    worst = 0.0
    for n in range(len(poses)):
        for c in range(3):
            u = np.zeros(3)
            u[c] = h
            plus, minus = poses[n].copy(), poses[n].copy()
            plus[:3] += u
            minus[:3] -= u
            both = body_query_model(point_field, sph, np.stack([plus, minus, rotated(poses[n], u), rotated(poses[n], -u)]), margin)["cost"]
            for fd, an in (((both[0] - both[1]) / (2 * h), base["grad"][n, c]), ((both[2] - both[3]) / (2 * h), base["grad"][n, 3 + c])):
                worst = max(worst, abs(fd - an))
                assert abs(fd - an) <= tol, (n, c, fd, an, tol)
    print(f"worst |central difference - grad| {worst:.3g}, tolerance {tol:.3g}")
    assert np.abs(base["grad"]).min() > 1e-3      # against an empty test: the derivatives are far from 0


def test_rotation_is_orthonormal_to_8_ulp():
    rng = np.random.RandomState(2)
    q = rng.randn(4000, 4)
    q *= (10.0 ** rng.uniform(-3, 3, 4000) / np.linalg.norm(q, axis=1))[:, None]
    norms = np.linalg.norm(q, axis=1)
    assert norms.min() < 2e-3 and norms.max() > 500
    R, valid = body_rotation(np.concatenate([np.zeros((4000, 3)), q], axis=1))
    assert valid.all()
    err = np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max()
    print(f"worst |R R^T - I| entry: {err / 2.0 ** -52:.2f} ulp")
    assert err <= 8 * 2.0 ** -52
    assert np.all(np.abs(np.linalg.det(R) - 1.0) <= 8 * 2.0 ** -52)


def test_ties_name_the_lowest_sphere():
    """every sphere on one plane parallel to a wall, identity rotation: all clearances tie; also after permuting the table"""
    def wall(pos):
        pos = np.asarray(pos, np.float64).reshape(-1, 3)
        return pos[:, 1] - 1.05, np.tile([0.0, 1.0, 0.0], (len(pos), 1))
    rng = np.random.RandomState(3)
    K = 130
    sph = np.stack([rng.uniform(-0.7, 0.7, K), np.full(K, 0.25), rng.uniform(-0.7, 0.7, K), np.full(K, 0.1)], 1)
    poses = np.array([[3.0, 2.6, 3.0, 1.0, 0, 0, 0], [1.0, 4.0, 2.0, 7.5, 0, 0, 0]])
    for table in (sph, sph[rng.permutation(K)], sph[::-1]):
        r = body_query_model(wall, table, poses, 0.5)
        assert np.all(r["sphere_clearance"] == r["sphere_clearance"][:, :1]) and np.all(r["min_sphere"] == 0)
        assert np.array_equal(r["min_pos"], poses[:, :3] + table[0, :3])
    # one sphere strictly closer: it wins wherever it stands
    sph[77, 1] = 0.2
    assert np.all(body_query_model(wall, sph, poses, 0.5)["min_sphere"] == 77)


def invalid_patterns():
    good = np.array([0.1, -0.2, 0.3, 0.5, -0.5, 0.5, 0.5])
    out = []
    for slot in range(7):
        for bad in (np.nan, np.inf, -np.inf):
            p = good.copy()
            p[slot] = bad
            out.append((f"slot {slot} {bad}", p))
    out.append(("zero quaternion", np.array([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 0.0])))
    out.append(("s underflows to 0", np.array([0.1, -0.2, 0.3, 1e-200, 0.0, 0.0, 1e-200])))
    out.append(("k overflows", np.array([0.1, -0.2, 0.3, 1e-160, 0.0, 0.0, 0.0])))
    return out


@pytest.mark.parametrize("what,pose", invalid_patterns(), ids=[w for w, _ in invalid_patterns()])
def test_invalid_pose_reports_its_pattern_and_leaves_its_neighbours_alone(what, pose):
    rng = np.random.RandomState(9)
    sph, good = random_body(rng, 5), random_poses(rng, 4)
    alone = body_query_model(point_field, sph, good, 3.0)
    poses = np.stack([good[0], pose, good[1], good[2], pose, good[3]])
    r = body_query_model(point_field, sph, poses, 3.0)
    keep = [0, 2, 3, 5]
    assert_bits({k: r[k][keep] for k in EXACT + ("cost", "grad")}, alone, EXACT + ("cost", "grad"), what)
    for n in (1, 4):
        assert np.isnan(r["min_clearance"][n]) and np.isnan(r["cost"][n]) and np.isnan(r["min_pos"][n]).all() and np.isnan(r["min_grad"][n]).all()
        assert np.isnan(r["sphere_clearance"][n]).all() and r["min_sphere"][n] == -1 and r["n_below"][n] == -1
        assert not r["grad"][n].any()


def test_a_tiny_but_valid_quaternion_and_the_argument_rules():
    sph = np.array([[0.3, 0.0, 0.0, 0.1]])
    tiny = np.array([[0, 0, 0, 1e-150, 0, 0, 1e-150]])       # s = 2e-300, k = 1e300: finite
    one = np.array([[0, 0, 0, 1.0, 0, 0, 1.0]])              # the same rotation: a quarter turn about z
    a, b = body_query_model(point_field, sph, tiny, 9.0), body_query_model(point_field, sph, one, 9.0)
    assert np.allclose(a["min_pos"], [[0.0, 0.3, 0.0]], atol=1e-15) and np.allclose(a["min_pos"], b["min_pos"], atol=1e-15)
    for bad_sph in (np.zeros((0, 4)), np.zeros((1025, 4)), [[0, 0, 0, -0.1]], [[np.nan, 0, 0, 0.1]], [[0, 0, 0, np.inf]]):
        with pytest.raises(ValueError):
            body_query_model(point_field, bad_sph, one, 1.0)
    for bad_margin in (np.nan, np.inf):
        with pytest.raises(ValueError):
            body_query_model(point_field, sph, one, bad_margin)
    empty = body_query_model(point_field, sph, np.zeros((0, 7)), 1.0)
    assert empty["cost"].shape == (0,) and empty["grad"].shape == (0, 6) and empty["sphere_clearance"].shape == (0, 1)
