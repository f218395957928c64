"""The definition of fiesta_hip_body_sweep (include/fiesta_hip.h) in numpy: a body of spheres moved along polylines of poses."""
from __future__ import annotations

import numpy as np

from .body_model import body_query_model, body_rotation
from .esdf_map import PATH_MAX_RATIO


def body_reach(spheres):
    """The reach of a sphere table ((K, 4): cx, cy, cz, r): the farthest centre from the body origin, in the header's operation
    order."""
    sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
    cx, cy, cz = sph[:, 0], sph[:, 1], sph[:, 2]
    return float(np.max(np.sqrt((cx * cx + cy * cy) + cz * cz))) if len(sph) else 0.0


def sweep_poses(poses, offsets, step, reach):
    """The sample rule of fiesta_hip_body_sweep in numpy, bit for bit.  Every waypoint quaternion is normalised, u = q / sqrt(|q|^2);
    for each segment (a, u0) -> (b, u1) of a path d = b - a, L = |d|, v = u1 on u0's side, ch = |v - u0|, W = (2.25 * reach) * ch,
    S = max(1, ceil((L + W) / step)), the samples (a + d * t, (1 - t) * u0 + t * v) at t = k / S for k < S; then the last waypoint
    with its own u.  Returns (sample_poses, n_samples): the samples of every valid path, path after path, as an (M, 7) f64 array, and
    per path its count (0: empty, -1: invalid -- an invalid waypoint pose by the body query's rule, or a segment with
    (L + W) / step > 2^24; an invalid path contributes no rows).  Sample i of path p is row sum(max(n_samples[:p], 0)) + i."""
    w = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    step, reach = float(step), float(reach)
    if len(off) < 1 or off[0] != 0 or off[-1] != len(w) or np.any(np.diff(off) < 0):
        raise ValueError("offsets: n_paths + 1 non-decreasing entries from 0 to n_poses")
    if not (np.isfinite(step) and step > 0):
        raise ValueError("step must be finite and > 0")
    n_paths, nw = len(off) - 1, np.diff(off)
    path_of = np.repeat(np.arange(n_paths), nw)                      # the path of every waypoint
    last = np.zeros(len(w), bool)
    last[off[1:][nw > 0] - 1] = True                                 # the last waypoint of its path: no segment starts there
    _, valid = body_rotation(w)
    with np.errstate(all="ignore"):
        q = w[:, 3:]
        s = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        u = q / np.sqrt(s)[:, None]
        u1 = np.zeros_like(u)
        u1[:-1] = u[1:]
        d = np.zeros((len(w), 3))
        d[:-1] = w[1:, :3] - w[:-1, :3]
        L = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        dot = ((u[:, 0] * u1[:, 0] + u[:, 1] * u1[:, 1]) + u[:, 2] * u1[:, 2]) + u[:, 3] * u1[:, 3]
        v = np.where((dot >= 0)[:, None], u1, -u1)
        e = v - u
        ch = np.sqrt(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) + e[:, 3] * e[:, 3])
        W = (2.25 * reach) * ch
        ratio = (L + W) / step
        seg_ok = last | (ratio <= PATH_MAX_RATIO)
        S = np.where(last, 1, np.maximum(1, np.ceil(np.where(seg_ok, ratio, 0.0)))).astype(np.int64)
    bad_wp = ~valid | ~seg_ok
    bad = np.zeros(n_paths, bool)
    np.logical_or.at(bad, path_of, bad_wp)
    S[bad[path_of]] = 0                                              # an invalid path has no samples
    n_samples = np.zeros(n_paths, np.int64)
    np.add.at(n_samples, path_of, S)
    n_samples[bad] = -1
    idx = np.repeat(np.arange(len(w)), S)                            # the waypoint each sample starts from, in sample order
    k = np.arange(len(idx)) - np.repeat(np.cumsum(S) - S, S)
    with np.errstate(all="ignore"):
        t = k.astype(np.float64) / S[idx].astype(np.float64)
        r = 1.0 - t
        pos = w[idx, :3] + d[idx] * t[:, None]
        rot = r[:, None] * u[idx] + t[:, None] * v[idx]
    fin = last[idx][:, None]                                         # the final sample: the last waypoint with its own u
    out = np.concatenate([np.where(fin, w[idx, :3], pos), np.where(fin, u[idx], rot)], axis=1)
    return np.ascontiguousarray(out), n_samples


def body_sweep_model(query, spheres, poses, offsets, step, margin):
    """fiesta_hip_body_sweep over any `query(pos) -> (d, grad)` that answers an (M, 3) batch (a map's GetDistWithGradTrilinear, or any
    callable): the samples of sweep_poses, each evaluated by body_query_model, reduced per path in sample order -- bit for bit what
    the library computes from the same (d, grad).  Returns a dict of the eleven outputs named as the fields of
    fiesta_hip_sweep_result."""
    samples, n_samples = sweep_poses(poses, offsets, step, body_reach(spheres))
    bq = body_query_model(query, spheres, samples, margin)
    margin = float(margin)
    N = len(n_samples)
    out = {"min_clearance": np.full(N, np.inf), "min_sample": np.full(N, -1, np.int64), "min_sphere": np.full(N, -1, np.int32),
           "min_pose": np.full((N, 7), np.nan), "min_pos": np.full((N, 3), np.nan), "min_grad": np.zeros((N, 3)),
           "first_below": np.full(N, -1, np.int64), "first_below_sphere": np.full(N, -1, np.int32),
           "first_below_pose": np.full((N, 7), np.nan), "n_below": np.zeros(N, np.int64), "n_samples": n_samples.copy()}
    out["min_clearance"][n_samples < 0] = np.nan
    out["n_below"][n_samples < 0] = -1
    first = np.cumsum(np.maximum(n_samples, 0)) - np.maximum(n_samples, 0)
    for p in np.nonzero(n_samples > 0)[0]:
        lo, hi = first[p], first[p] + n_samples[p]
        i = lo + int(np.argmin(bq["min_clearance"][lo:hi]))          # the first (lowest) sample of the minimum
        out["min_clearance"][p], out["min_sample"][p], out["min_sphere"][p] = bq["min_clearance"][i], i - lo, bq["min_sphere"][i]
        out["min_pose"][p], out["min_pos"][p], out["min_grad"][p] = samples[i], bq["min_pos"][i], bq["min_grad"][i]
        below = bq["n_below"][lo:hi] > 0
        out["n_below"][p] = np.count_nonzero(below)
        if below.any():
            f = lo + int(np.argmax(below))
            out["first_below"][p], out["first_below_pose"][p] = f - lo, samples[f]
            out["first_below_sphere"][p] = int(np.argmax(bq["sphere_clearance"][f] < margin))
    return out
