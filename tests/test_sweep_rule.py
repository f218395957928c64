"""CPU side of the body sweeps (fiesta_hip_body_sweep, include/fiesta_hip.h): the definition.

fiesta_amd.sweep_poses and fiesta_amd.body_sweep_model are the model the GPU tests compare the kernels with, so they must be the
header's rule.  Here they are checked against a literal triple loop over paths, samples and spheres (Python floats, one operation per
line of the header) on an analytic field, against path_samples where nothing rotates, and for what the rule promises: the waypoint
samples, the indifference to a quaternion's sign, valid sample poses, the spacing of consecutive samples, every special and invalid
path.  Pure Python: nothing built is needed.
"""
import math

import numpy as np
import pytest

from fiesta_amd import body_query_model, body_reach, body_rotation, body_sweep_model, path_samples, sweep_poses
from test_body_rule import bits, point_field

FIELDS = ("min_clearance", "min_sample", "min_sphere", "min_pose", "min_pos", "min_grad", "first_below", "first_below_sphere",
          "first_below_pose", "n_below", "n_samples")
POSE_FIELDS = ("min_pose", "first_below_pose")


def assert_bits(got, want, keys=FIELDS, what=""):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries differ in bits, first {bad[:3].tolist()}: {a[tuple(bad[0])]!r} / {b[tuple(bad[0])]!r}"


def unit(pose):
    """(valid, u) of a waypoint pose, in Python floats"""
    px, py, pz, qw, qx, qy, qz = (float(v) for v in pose)
    s = ((qw * qw + qx * qx) + qy * qy) + qz * qz
    if not all(math.isfinite(v) for v in (px, py, pz, qw, qx, qy, qz)) or not s > 0:
        return False, None
    with np.errstate(over="ignore"):
        k = float(np.float64(2.0) / np.float64(s))
    if not math.isfinite(k):
        return False, None
    n = math.sqrt(s)
    return True, [qw / n, qx / n, qy / n, qz / n]


def loop_poses(poses, offsets, step, reach):
    """the header's rule, path by path and sample by sample: (list of per-path sample lists or None for an invalid path)"""
    out = []
    for p in range(len(offsets) - 1):
        rows = [poses[i] for i in range(offsets[p], offsets[p + 1])]
        units = [unit(r) for r in rows]
        ok = all(v for v, _ in units)
        samples = []
        for j in range(len(rows) - 1):
            if not ok:
                break
            a, b = [float(v) for v in rows[j][:3]], [float(v) for v in rows[j + 1][:3]]
            u0, u1 = units[j][1], units[j + 1][1]
            d = [b[c] - a[c] for c in range(3)]
            L = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            dot = ((u0[0] * u1[0] + u0[1] * u1[1]) + u0[2] * u1[2]) + u0[3] * u1[3]
            v = u1 if dot >= 0 else [-x for x in u1]
            e = [v[c] - u0[c] for c in range(4)]
            ch = math.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3])
            W = (2.25 * reach) * ch
            ratio = (L + W) / step
            if not ratio <= 2.0 ** 24:
                ok = False
                break
            S = max(1, int(math.ceil(ratio)))
            Sd = float(S)
            for k in range(S):
                t = float(k) / Sd
                r = 1.0 - t
                samples.append([a[c] + d[c] * t for c in range(3)] + [r * u0[c] + t * v[c] for c in range(4)])
        if ok and rows:
            samples.append([float(v) for v in rows[-1][:3]] + units[-1][1])
        out.append(samples if ok else None)
    return out


def loop_model(query, spheres, poses, offsets, step, margin):
    """the whole call as a triple loop: paths, samples, spheres"""
    reach = max(math.sqrt((float(c[0]) * float(c[0]) + float(c[1]) * float(c[1])) + float(c[2]) * float(c[2])) for c in spheres)
    N = len(offsets) - 1
    out = {"min_clearance": np.full(N, np.inf), "min_sample": np.full(N, -1, np.int64), "min_sphere": np.full(N, -1, np.int32),
           "min_pose": np.full((N, 7), np.nan), "min_pos": np.full((N, 3), np.nan), "min_grad": np.zeros((N, 3)),
           "first_below": np.full(N, -1, np.int64), "first_below_sphere": np.full(N, -1, np.int32),
           "first_below_pose": np.full((N, 7), np.nan), "n_below": np.zeros(N, np.int64), "n_samples": np.zeros(N, np.int64)}
    for p, samples in enumerate(loop_poses(poses, offsets, step, reach)):
        if samples is None:
            out["min_clearance"][p], out["n_below"][p], out["n_samples"][p] = np.nan, -1, -1
            continue
        out["n_samples"][p] = len(samples)
        best = None
        for i, (px, py, pz, qw, qx, qy, qz) in enumerate(samples):
            s = ((qw * qw + qx * qx) + qy * qy) + qz * qz
            k = 2.0 / s
            xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
            R = [[1.0 - k * (yy + zz), k * (xy - wz), k * (xz + wy)],
                 [k * (xy + wz), 1.0 - k * (xx + zz), k * (yz - wx)],
                 [k * (xz - wy), k * (yz + wx), 1.0 - k * (xx + yy)]]
            below = False
            for j, (cx, cy, cz, rad) in enumerate(spheres):
                cx, cy, cz, rad = float(cx), float(cy), float(cz), float(rad)
                x = [(px, py, pz)[c] + ((R[c][0] * cx + R[c][1] * cy) + R[c][2] * cz) for c in range(3)]
                d, g = query(np.array([x]))
                si = float(d[0]) - rad
                if best is None or si < best:
                    best = si
                    out["min_clearance"][p], out["min_sample"][p], out["min_sphere"][p] = si, i, j
                    out["min_pose"][p], out["min_pos"][p], out["min_grad"][p] = samples[i], x, g[0]
                if si < margin and not below:
                    below = True
                    out["n_below"][p] += 1
                    if out["first_below"][p] < 0:
                        out["first_below"][p], out["first_below_sphere"][p], out["first_below_pose"][p] = i, j, samples[i]
    return out


def random_quats(rng, n, scale=True):
    q = rng.randn(n, 4)
    return q * ((10.0 ** rng.uniform(-1, 1, n) if scale else 1.0) / np.linalg.norm(q, axis=1))[:, None]


def random_batch(rng, n_paths, lo=(0.0, -1.0, -3.0), hi=(6.0, 3.0, 2.0), leg=0.5):
    """paths of 0 .. 6 poses: random walks of ~`leg` metres per segment, every few poses repeated or turned in place"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    rows, off = [], [0]
    for p in range(n_paths):
        nw = int(rng.randint(0, 7))
        pos = lo + rng.rand(3) * (hi - lo)
        for j in range(nw):
            kind = rng.randint(0, 6) if j else 5
            q = random_quats(rng, 1)[0]
            if kind == 0:
                rows.append(list(rows[-1]))          # a repeated pose
            elif kind == 1:
                rows.append(list(pos) + list(q))     # a turn in place
            else:
                pos = pos + rng.randn(3) * leg
                rows.append(list(pos) + list(q))
        off.append(len(rows))
    return np.array(rows, np.float64).reshape(-1, 7), np.array(off, np.int64)


SPH = np.array([[0.4, 0.0, 0.0, 0.1], [-0.4, 0.1, 0.0, 0.12], [0.0, 0.0, 0.3, 0.05], [0.1, -0.2, -0.1, 0.0], [0.0, 0.0, 0.0, 0.2]])


def test_models_equal_the_literal_loop():
    rng = np.random.RandomState(1)
    poses, off = random_batch(rng, 40)
    reach = body_reach(SPH)
    assert reach == max(math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) for c in SPH.tolist())
    for step in (0.05, 0.31):
        rows, n = sweep_poses(poses, off, step, reach)
        want = loop_poses(poses, off, step, reach)
        assert n.tolist() == [len(s) for s in want] and len(rows) == n.sum() and n.min() == 0 and n.max() > 20
        flat = np.array([s for path in want for s in path], np.float64).reshape(-1, 7)
        assert np.array_equal(bits(rows), bits(flat))
        for margin in (2.5, 0.6, -1.0):
            got = body_sweep_model(point_field, SPH, poses, off, step, margin)
            loop = loop_model(point_field, SPH, poses, off, step, margin)
            assert_bits(got, loop, what=f"step {step} margin {margin}")
        some = body_sweep_model(point_field, SPH, poses, off, step, 2.5)
        assert 5 < np.count_nonzero(some["first_below"] >= 0) < np.count_nonzero(n > 0)        # (not an empty comparison)


def test_without_rotation_the_positions_are_path_samples():
    rng = np.random.RandomState(2)
    poses, off = random_batch(rng, 30)
    for q in ([1.0, 0.0, 0.0, 0.0], [0.3, -2.0, 0.7, 0.01], [-1e-3, 2e-3, 0.0, 1e-3]):
        poses[:, 3:] = q
        rows, n = sweep_poses(poses, off, 0.07, 1.7)
        pos, n_path = path_samples(poses[:, :3], off, 0.07)
        assert np.array_equal(n, n_path) and np.array_equal(bits(rows[:, :3]), bits(pos))
        s = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        u = np.array([v / s for v in q])
        # r*u + t*u rounds back to u up to an ulp; at the waypoints it is u exactly
        assert np.max(np.abs(rows[:, 3:] - u)) < 4e-16


def test_waypoint_samples_are_the_waypoints_normalised():
    rng = np.random.RandomState(3)
    poses, off = random_batch(rng, 30)
    reach = 0.8
    rows, n = sweep_poses(poses, off, 0.1, reach)
    want = loop_poses(poses, off, 0.1, reach)
    first = np.cumsum(n) - n
    checked = 0
    for p in range(len(n)):
        nw = off[p + 1] - off[p]
        if nw == 0:
            continue
        # the sample counts of the path's segments, from the literal loop: the waypoints sit at their running sum
        at = 0
        for j in range(nw):
            row = rows[first[p] + at]
            ok, u = unit(poses[off[p] + j])
            assert ok and np.array_equal(bits(row[:3]), bits(poses[off[p] + j, :3])) and np.array_equal(bits(row[3:]), bits(np.array(u)))
            checked += 1
            if j + 1 < nw:     # S of segment j: the samples up to the next one that equals waypoint j + 1 exactly
                seg = loop_poses(poses[off[p] + j:off[p] + j + 2], np.array([0, 2]), 0.1, reach)[0]
                at += len(seg) - 1
        assert at == n[p] - 1 and want[p] is not None
    assert checked > 60


def test_negating_a_quaternion_changes_only_the_quaternion_columns():
    rng = np.random.RandomState(4)
    poses, off = random_batch(rng, 40)
    base = body_sweep_model(point_field, SPH, poses, off, 0.05, 1.5)
    rows0, n0 = sweep_poses(poses, off, 0.05, body_reach(SPH))
    other = [k for k in FIELDS if k not in POSE_FIELDS]
    for i in rng.choice(len(poses), 25, replace=False):
        neg = poses.copy()
        neg[i, 3:] = -neg[i, 3:]
        rows, n = sweep_poses(neg, off, 0.05, body_reach(SPH))
        assert np.array_equal(n, n0) and np.array_equal(bits(rows[:, :3]), bits(rows0[:, :3]))
        assert np.array_equal(bits(np.abs(rows[:, 3:])), bits(np.abs(rows0[:, 3:])))       # q or -q, component for component
        got = body_sweep_model(point_field, SPH, neg, off, 0.05, 1.5)
        assert_bits(got, base, other, f"pose {i} negated")
        for k in POSE_FIELDS:
            assert np.array_equal(bits(got[k][:, :3]), bits(base[k][:, :3]))
            assert np.array_equal(bits(np.abs(got[k][:, 3:])), bits(np.abs(base[k][:, 3:])))


def test_every_sample_pose_is_a_valid_body_pose():
    rng = np.random.RandomState(5)
    poses, off = random_batch(rng, 200)
    # opposite and nearly opposite quaternions, and a right angle between them: dot = -1, ~0
    poses[1, 3:] = -3.0 * poses[0, 3:]
    rows, n = sweep_poses(poses, off, 0.02, 1.0)
    assert n.min() >= 0 and len(rows) > 20000
    _, valid = body_rotation(rows)
    s = np.sum(rows[:, 3:] ** 2, axis=1)
    print(f"{len(rows)} sample poses: |q|^2 in [{s.min():.15f}, {s.max():.15f}]")
    assert valid.all() and s.min() >= 0.5 - 1e-12 and s.max() <= 1.0 + 1e-12


def segment_pairs(rng, n, max_deg):
    """n two-pose paths: random directions and lengths, a rotation of up to max_deg about a random axis"""
    q0 = random_quats(rng, n, scale=False)
    ang = np.radians(rng.uniform(0, max_deg, n))
    ang[: n // 10] = np.radians(max_deg)                 # the bound's own case
    axis = rng.randn(n, 3)
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    dq = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
    w0, v0, w1, v1 = dq[:, 0], dq[:, 1:], q0[:, 0], q0[:, 1:]
    q1 = np.concatenate([(w0 * w1 - np.sum(v0 * v1, 1))[:, None], w0[:, None] * v1 + w1[:, None] * v0 + np.cross(v0, v1)], axis=1)
    a = rng.uniform(-2, 2, (n, 3))
    length = rng.choice([0.0, 0.05, 0.4, 2.0], n) * rng.rand(n)
    dirs = rng.randn(n, 3)
    b = a + dirs / np.linalg.norm(dirs, axis=1)[:, None] * length[:, None]
    scale = 10.0 ** rng.uniform(-1, 1, (2, n, 1))
    poses = np.empty((2 * n, 7))
    poses[0::2] = np.concatenate([a, q0 * scale[0]], axis=1)
    poses[1::2] = np.concatenate([b, q1 * scale[1] * rng.choice([-1.0, 1.0], (n, 1))], axis=1)
    return poses, np.arange(0, 2 * n + 1, 2, dtype=np.int64)


def worst_centre_step(poses, off, step, centres):
    """the largest displacement of any of `centres` (body frame) between consecutive samples of a path, over the batch, in steps"""
    rows, n = sweep_poses(poses, off, step, float(np.max(np.linalg.norm(centres, axis=1))))
    assert n.min() >= 2
    R, valid = body_rotation(rows)
    assert valid.all()
    x = rows[:, None, :3] + np.einsum("nij,kj->nki", R, centres)
    move = np.linalg.norm(np.diff(x, axis=0), axis=2).max(axis=1)
    ends = np.cumsum(n)[:-1] - 1                           # (the pair that straddles two paths is not a step of the sweep)
    move[ends] = 0.0
    return float(move.max() / step)


def test_consecutive_samples_move_no_sphere_centre_farther_than_the_bound():
    """Why W.  u0 and v are unit vectors at the angle phi = theta / 2, theta the segment's rotation, so ch = 2 sin(theta / 4).
    q(t) = (1 - t) u0 + t v turns in their plane at the rate sin(phi) / |q(t)|^2 per unit t, at most sin(phi) / cos^2(phi / 2) =
    2 tan(phi / 2) (mid-arc), so the body turns at most 4 tan(theta / 4) / S between two samples, and a centre at rho <= reach
    moves at most (L + 4 reach tan(theta / 4)) / S.  S >= (L + 4.5 reach sin(theta / 4)) / step, so the move is at most
    step * max(1, 1 / (1.125 cos(theta / 4))): 0.962 -> step itself up to 90 degrees (109 degrees, in fact), 1.257 step at 180."""
    rng = np.random.RandomState(6)
    centres = np.array([[0.6, 0.0, 0.0], [0.0, -0.6, 0.0], [0.35, 0.35, 0.35], [0.0, 0.0, 0.1], [-0.3, 0.2, -0.45]])
    worst = {}
    for max_deg, bound in ((90.0, 1.0 + 1e-9), (180.0, 1.26)):
        poses, off = segment_pairs(rng, 2000, max_deg)
        worst[max_deg] = max(worst_centre_step(poses, off, step, centres) for step in (0.05, 0.011))
        print(f"rotations up to {max_deg:.0f} degrees: the worst centre displacement between consecutive samples is {worst[max_deg]:.4f} step")
        assert worst[max_deg] <= bound, (max_deg, worst[max_deg])
    assert worst[90.0] > 0.9 and worst[180.0] > 1.15         # the bounds are tight: W is not larger than it has to be


def test_pure_rotation_in_place_and_repeated_poses():
    half = math.sqrt(0.5)
    poses = np.array([[1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, half, 0.0, 0.0, half],       # 90 degrees about z, in place
                      [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0],         # a repeated pose
                      [2.0, 0.0, 0.0, 0.0, -7.0, 0.0, 0.0]])                                             # and again, negated and scaled
    off = np.array([0, 2, 4, 5, 5], np.int64)
    reach, step = 0.5, 0.01
    rows, n = sweep_poses(poses, off, step, reach)
    ch = 2.0 * math.sin(math.pi / 8)
    assert n[0] == math.ceil(2.25 * reach * ch / step) + 1 and abs(n[0] - 1 - 87) <= 1
    assert np.all(rows[:n[0], :3] == 1.0)                                    # L = 0: every sample stands in place
    yaw = 2.0 * np.arctan2(rows[:n[0], 6], rows[:n[0], 3])
    assert np.all(np.diff(yaw) > 0) and yaw[0] == 0 and abs(yaw[-1] - math.pi / 2) < 1e-15
    assert n[1] == 2 and np.array_equal(rows[n[0]], rows[n[0] + 1]) and rows[n[0]].tolist() == [2.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert n[2] == 1 and rows[n[0] + 2].tolist() == [2.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0]       # a path of one pose: its own u
    assert n[3] == 0 and len(rows) == n.sum()
    # a repeated pose whose quaternion is negated is still one sample per segment (the shorter arc has length 0)
    both = np.array([poses[2], poses[4]])
    rows2, n2 = sweep_poses(both, np.array([0, 2]), step, reach)
    assert n2[0] == 2 and rows2[0].tolist() == [2.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0] and rows2[1].tolist() == [2.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0]
    out = body_sweep_model(point_field, SPH, poses, off, step, 0.5)
    assert out["n_samples"].tolist() == sweep_poses(poses, off, step, body_reach(SPH))[1].tolist() and out["min_clearance"][3] == np.inf and out["min_sample"][3] == -1
    assert out["n_below"][3] == 0 and not out["min_grad"][3].any() and np.isnan(out["min_pose"][3]).all() and np.isnan(out["min_pos"][3]).all()
    assert out["first_below"][3] == -1 and out["first_below_sphere"][3] == -1 and np.isnan(out["first_below_pose"][3]).all()


BAD_POSES = {"nan position": (1, np.nan), "inf position": (0, np.inf), "inf quaternion": (5, np.inf), "nan quaternion": (3, np.nan),
             "zero quaternion": (None, (0.0, 0.0, 0.0, 0.0)), "k overflows": (None, (1e-160, 0.0, 0.0, 0.0)),
             "s underflows": (None, (1e-200, 1e-200, 1e-200, 1e-200))}


@pytest.mark.parametrize("kind", sorted(BAD_POSES) + ["too many samples", "too many samples by rotation"])
def test_invalid_paths_leave_their_neighbours_alone(kind):
    rng = np.random.RandomState(7)
    poses, off = random_batch(rng, 30)
    long_paths = [p for p in range(30) if off[p + 1] - off[p] >= 3]
    victim = long_paths[len(long_paths) // 2]
    clean = body_sweep_model(point_field, SPH, poses, off, 0.05, 1.5)
    assert clean["n_samples"][victim] > 0
    bad, step, sph = poses.copy(), 0.05, SPH
    row = off[victim] + 1                                     # a waypoint in the middle of the path
    if kind == "too many samples":
        bad[row, 0] += 0.05 * 2.0 ** 24 * 1.01
    elif kind == "too many samples by rotation":              # L = 0 and a half turn of a table with a long reach
        poses[:, 3:] = bad[:, 3:] = q = np.array([0.5, -1.0, 0.25, 2.0])       # (nothing else in the batch turns: W = 0 there)
        bad[row, :3] = bad[row - 1, :3]
        bad[row, 3:] = (-q[1], q[0], q[3], -q[2])             # orthogonal to q: ch = sqrt(2)
        sph = SPH.copy()
        sph[0, 0] = 0.05 * 2.0 ** 24 / (2.25 * math.sqrt(2.0)) * 1.01
        clean = body_sweep_model(point_field, sph, poses, off, 0.05, 1.5)
    else:
        col, v = BAD_POSES[kind]
        if col is None:
            bad[row, 3:] = v
        else:
            bad[row, col] = v
    got = body_sweep_model(point_field, sph, bad, off, step, 1.5)
    assert_bits(got, loop_model(point_field, sph, bad, off, step, 1.5), what=kind)
    rows, n = sweep_poses(bad, off, step, body_reach(sph))
    assert n[victim] == -1 and len(rows) == np.maximum(n, 0).sum()
    assert got["n_samples"][victim] == -1 and np.isnan(got["min_clearance"][victim]) and got["n_below"][victim] == -1
    assert got["min_sample"][victim] == got["min_sphere"][victim] == got["first_below"][victim] == got["first_below_sphere"][victim] == -1
    assert np.isnan(got["min_pose"][victim]).all() and np.isnan(got["min_pos"][victim]).all() and np.isnan(got["first_below_pose"][victim]).all()
    assert not got["min_grad"][victim].any()
    keep = np.arange(30) != victim
    assert_bits({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()}, what=f"{kind}: the other paths")


def test_the_sample_limit_is_two_to_the_24():
    """(L + W) / step one ulp above 2^24 is invalid, by translation and by rotation; the valid side of the limit has 2^24 + 1 samples
    and is left to the device test"""
    q = [1.0, 0.0, 0.0, 0.0]
    over = [[0.0, 0.0, 0.0] + q, [np.nextafter(2.0 ** 24, np.inf), 0.0, 0.0] + q, [0.0, 0.0, 0.0] + q, [1.0, 0.0, 0.0] + q]
    _, n = sweep_poses(np.array(over), np.array([0, 2, 4]), 1.0, 1.0)
    assert n.tolist() == [-1, 2]
    turn = [[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]]        # ch = sqrt(2), L = 0
    w = (2.25 * 1.0) * math.sqrt(2.0)
    _, n = sweep_poses(np.array(turn), np.array([0, 2]), np.nextafter(w / 2.0 ** 24, 0.0), 1.0)
    assert n.tolist() == [-1]
    _, n = sweep_poses(np.array(turn), np.array([0, 2]), w / 2.0 ** 10, 1.0)
    assert n.tolist() == [2 ** 10 + 1]


def test_whole_call_errors_of_the_model():
    poses, off = np.zeros((2, 7)), np.array([0, 2])
    poses[:, 3] = 1.0
    for bad_off in ([1, 2], [0, 1], [0, 3], [0, 2, 1, 2]):
        with pytest.raises(ValueError):
            sweep_poses(poses, np.array(bad_off), 0.1, 1.0)
    for step in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            sweep_poses(poses, off, step, 1.0)
    for sph, margin in ((np.zeros((0, 4)), 0.1), (np.array([[0, 0, 0, -1.0]]), 0.1), (np.array([[np.nan, 0, 0, 1.0]]), 0.1), (SPH, np.nan)):
        with pytest.raises(ValueError):
            body_sweep_model(point_field, sph, poses, off, 0.1, margin)


def test_the_model_is_the_body_query_reduced_per_path():
    rng = np.random.RandomState(8)
    poses, off = random_batch(rng, 60)
    poses[off[7] + 1, 3:] = 0.0 if off[8] - off[7] > 1 else poses[off[7] + 1, 3:]
    margin, step = 1.8, 0.04
    got = body_sweep_model(point_field, SPH, poses, off, step, margin)
    rows, n = sweep_poses(poses, off, step, body_reach(SPH))
    per = body_query_model(point_field, SPH, rows, margin)
    first = np.cumsum(np.maximum(n, 0)) - np.maximum(n, 0)
    seen = 0
    for p in range(60):
        if n[p] <= 0:
            continue
        mc, nb = per["min_clearance"][first[p]:first[p] + n[p]], per["n_below"][first[p]:first[p] + n[p]]
        assert got["min_clearance"][p] == mc.min() and got["min_sample"][p] == int(np.argmin(mc))
        hit = np.nonzero(nb > 0)[0]
        assert got["first_below"][p] == (hit[0] if len(hit) else -1) and got["n_below"][p] == len(hit)
        seen += len(hit) > 0
    assert 5 < seen < np.count_nonzero(n > 0)
