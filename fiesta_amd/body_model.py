"""The definition of fiesta_hip_body_query (include/fiesta_hip.h) in numpy: a body of spheres at a batch of poses."""
from __future__ import annotations

import numpy as np

BODY_MAX_SPHERES = 1024   # FIESTA_HIP_BODY_MAX_SPHERES


def body_rotation(poses):
    """The header's pose rule, operation by operation: (R (N, 3, 3), valid (N,)) of an (N, 7) batch px, py, pz, qw, qx, qy, qz.  A pose
    is valid iff its seven numbers are finite, s = |q|^2 > 0 and k = 2 / s is finite; the rows of an invalid pose hold whatever
    the arithmetic gives."""
    P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    qw, qx, qy, qz = P[:, 3], P[:, 4], P[:, 5], P[:, 6]
    with np.errstate(all="ignore"):
        s = ((qw * qw + qx * qx) + qy * qy) + qz * qz
        k = 2.0 / s
        valid = np.all(np.isfinite(P), axis=1) & (s > 0) & np.isfinite(k)
        xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
        R = np.empty((len(P), 3, 3))
        R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1.0 - k * (yy + zz), k * (xy - wz), k * (xz + wy)
        R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = k * (xy + wz), 1.0 - k * (xx + zz), k * (yz - wx)
        R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = k * (xz - wy), k * (yz + wx), 1.0 - k * (xx + yy)
    return R, valid


def body_query_model(query, spheres, poses, margin):
    """fiesta_hip_body_query over any `query(pos) -> (d, grad)` that answers an (M, 3) batch (a map's GetDistWithGradTrilinear, or any
    callable): every per-pose and per-sphere TERM in the header's operation order -- bit for bit what the library computes from the
    same (d, grad) -- and the sums over a pose's spheres in sphere order.  spheres: (K, 4) cx, cy, cz, r; poses: (N, 7).  Returns a
    dict: the eight outputs named as the fields of fiesta_hip_body_result (sphere_clearance (N, K), grad (N, 6)) and, for the
    tolerance of a comparison with another order of summation, cost_n / grad_n (the number of summed terms: K) and cost_abs (N,) /
    grad_abs (N, 6), the sums of the terms' absolute values.  Two orders differ by at most (n + 16) * 2^-52 * abs."""
    sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
    P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    margin = float(margin)
    K, N = len(sph), len(P)
    if not 1 <= K <= BODY_MAX_SPHERES:
        raise ValueError("n_spheres must be 1 .. 1024")
    if not np.all(np.isfinite(sph)) or np.any(sph[:, 3] < 0):
        raise ValueError("a sphere's centre and radius must be finite, its radius >= 0")
    if not np.isfinite(margin):
        raise ValueError("margin must be finite")
    R, valid = body_rotation(P)
    Rv, pv = R[valid], P[valid, :3]
    M = len(Rv)
    cx, cy, cz, rad = sph[None, :, 0], sph[None, :, 1], sph[None, :, 2], sph[None, :, 3]
    a = np.empty((M, K, 3))
    for c in range(3):
        a[:, :, c] = (Rv[:, c, 0, None] * cx + Rv[:, c, 1, None] * cy) + Rv[:, c, 2, None] * cz
    x = pv[:, None, :] + a
    if M:
        d, g = query(np.ascontiguousarray(x.reshape(-1, 3)))
        d, g = np.asarray(d, np.float64).reshape(M, K), np.asarray(g, np.float64).reshape(M, K, 3)
    else:
        d, g = np.zeros((0, K)), np.zeros((0, K, 3))
    s = d - rad
    below = s < margin
    e = np.where(below, margin - s, 0.0)
    phi = e * e
    gam = np.where(below[:, :, None], (-2.0 * e)[:, :, None] * g, 0.0)
    t = np.empty((M, K, 3))
    t[:, :, 0] = a[:, :, 1] * gam[:, :, 2] - a[:, :, 2] * gam[:, :, 1]
    t[:, :, 1] = a[:, :, 2] * gam[:, :, 0] - a[:, :, 0] * gam[:, :, 2]
    t[:, :, 2] = a[:, :, 0] * gam[:, :, 1] - a[:, :, 1] * gam[:, :, 0]
    terms = np.concatenate([phi[:, :, None], gam, t], axis=2)          # (M, K, 7)
    zero = np.zeros((M, 1, 7))                                         # every sum starts from +0 (so a sum of -0 terms is +0)
    sums = np.cumsum(np.concatenate([zero, terms], axis=1), axis=1)[:, -1, :]          # (cumsum adds in sphere order)
    asums = np.cumsum(np.concatenate([zero, np.abs(terms)], axis=1), axis=1)[:, -1, :]
    arg = np.argmin(s, axis=1)                                         # the first (lowest) index of the minimum
    rows = np.arange(M)
    out = {"min_clearance": np.full(N, np.nan), "min_sphere": np.full(N, -1, np.int32), "min_pos": np.full((N, 3), np.nan),
           "min_grad": np.full((N, 3), np.nan), "n_below": np.full(N, -1, np.int32), "cost": np.full(N, np.nan),
           "grad": np.zeros((N, 6)), "sphere_clearance": np.full((N, K), np.nan),
           "cost_n": np.full(N, K, np.int64), "cost_abs": np.zeros(N), "grad_n": np.full(N, K, np.int64), "grad_abs": np.zeros((N, 6))}
    out["min_clearance"][valid] = s[rows, arg]
    out["min_sphere"][valid] = arg
    out["min_pos"][valid] = x[rows, arg]
    out["min_grad"][valid] = g[rows, arg]
    out["n_below"][valid] = np.count_nonzero(below, axis=1)
    out["cost"][valid] = sums[:, 0]
    out["grad"][valid] = sums[:, 1:]
    out["sphere_clearance"][valid] = s
    out["cost_abs"][valid] = asums[:, 0]
    out["grad_abs"][valid] = asums[:, 1:]
    return out
