"""The definition of fiesta_hip_articulated_query (include/fiesta_hip.h) in numpy: spheres on frames, one pose per frame."""
from __future__ import annotations

import numpy as np

from .body_model import BODY_MAX_SPHERES, body_rotation

BODY_MAX_FRAMES = 64   # FIESTA_HIP_BODY_MAX_FRAMES


def group_spheres_by_frame(spheres, sphere_frame):
    """A table whose spheres are not grouped by frame, in the form the call takes: (spheres[order], sphere_frame[order], order) with
    `order` the stable sort by frame, so the spheres of a frame keep their order.  Sphere j of the result is sphere order[j] of the
    input: `min_sphere` of the input is order[result min_sphere], and back[:, order] = result sphere_clearance undoes the columns."""
    sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
    frm = np.ascontiguousarray(sphere_frame, dtype=np.int32).reshape(-1)
    if len(frm) != len(sph):
        raise ValueError("sphere_frame must hold one frame index per sphere")
    order = np.argsort(frm, kind="stable")
    return np.ascontiguousarray(sph[order]), np.ascontiguousarray(frm[order]), order


def articulated_query_model(query, spheres, sphere_frame, n_frames, frame_poses, margin):
    """fiesta_hip_articulated_query over any `query(pos) -> (d, grad)` that answers an (M, 3) batch: every TERM in the header's
    operation order -- body_query_model's, with R and p of the sphere's frame -- and the sums over a frame's (for cost: all) spheres
    in sphere order.  spheres: (K, 4); sphere_frame: (K,) non-decreasing, 0 .. n_frames - 1; frame_poses: (N, F, 7).  Returns a
    dict: the ten outputs named as the fields of fiesta_hip_articulated_result (frame_clearance and frame_cost (N, F), frame_grad
    (N, F, 6), sphere_clearance (N, K)) and, for the tolerance of a comparison with another order of summation, cost_n (N,),
    frame_cost_n (N, F), frame_grad_n (N, F) (the number of summed terms: K, the frame's sphere count) and cost_abs (N,),
    frame_cost_abs (N, F), frame_grad_abs (N, F, 6), the sums of the terms' absolute values.  Two orders differ by at most
    (n + 16) * 2^-52 * abs.  Raises ValueError on the call's whole-call errors."""
    sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
    frm_in = np.asarray(sphere_frame)
    margin = float(margin)
    K, F = len(sph), int(n_frames)
    if not 1 <= K <= BODY_MAX_SPHERES:
        raise ValueError("n_spheres must be 1 .. 1024")
    if not 1 <= F <= BODY_MAX_FRAMES:
        raise ValueError("n_frames must be 1 .. 64")
    if frm_in.size != K or not np.issubdtype(frm_in.dtype, np.integer):
        raise ValueError("sphere_frame must hold one integer frame index per sphere")
    frm = frm_in.reshape(-1).astype(np.int64)
    if not np.all(np.isfinite(sph)) or np.any(sph[:, 3] < 0):
        raise ValueError("a sphere's centre and radius must be finite, its radius >= 0")
    if np.any(frm < 0) or np.any(frm >= F):
        raise ValueError("a frame index is outside 0 .. n_frames - 1")
    if np.any(np.diff(frm) < 0):
        raise ValueError("the spheres are not grouped by frame (sphere_frame decreases)")
    if not np.isfinite(margin):
        raise ValueError("margin must be finite")
    P = np.ascontiguousarray(frame_poses, dtype=np.float64)
    if P.size % (7 * F):
        raise ValueError("frame_poses must be (N, n_frames, 7)")
    P = P.reshape(-1, F, 7)
    N = len(P)
    R, fvalid = body_rotation(P.reshape(-1, 7))
    R, valid = R.reshape(N, F, 3, 3), fvalid.reshape(N, F).all(axis=1)
    Rv, pv = R[valid][:, frm], P[valid][:, frm, :3]          # (M, K, 3, 3), (M, K, 3): every sphere's own frame
    M = len(Rv)
    cx, cy, cz, rad = sph[None, :, 0], sph[None, :, 1], sph[None, :, 2], sph[None, :, 3]
    a = np.empty((M, K, 3))
    for c in range(3):
        a[:, :, c] = (Rv[:, :, c, 0] * cx + Rv[:, :, c, 1] * cy) + Rv[:, :, c, 2] * cz
    x = pv + a
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

    def ordered_sum(block):                                            # every sum starts from +0; cumsum adds in sphere order
        return np.cumsum(np.concatenate([np.zeros((M, 1, block.shape[2])), block], axis=1), axis=1)[:, -1, :]
    counts = np.bincount(frm, minlength=F)
    fsum, fabs, fmin = np.zeros((M, F, 7)), np.zeros((M, F, 7)), np.full((M, F), np.inf)
    for f in range(F):
        own = frm == f
        if own.any():
            fsum[:, f], fabs[:, f], fmin[:, f] = ordered_sum(terms[:, own]), ordered_sum(np.abs(terms[:, own])), s[:, own].min(axis=1)
    arg = np.argmin(s, axis=1)                                         # the first (lowest) index of the minimum
    rows = np.arange(M)
    out = {"min_clearance": np.full(N, np.nan), "min_sphere": np.full(N, -1, np.int32), "min_pos": np.full((N, 3), np.nan),
           "min_grad": np.full((N, 3), np.nan), "n_below": np.full(N, -1, np.int32), "cost": np.full(N, np.nan),
           "frame_clearance": np.full((N, F), np.nan), "frame_cost": np.full((N, F), np.nan), "frame_grad": np.zeros((N, F, 6)),
           "sphere_clearance": np.full((N, K), np.nan),
           "cost_n": np.full(N, K, np.int64), "cost_abs": np.zeros(N),
           "frame_cost_n": np.tile(counts.astype(np.int64), (N, 1)), "frame_cost_abs": np.zeros((N, F)),
           "frame_grad_n": np.tile(counts.astype(np.int64), (N, 1)), "frame_grad_abs": np.zeros((N, F, 6))}
    out["min_clearance"][valid] = s[rows, arg]
    out["min_sphere"][valid] = arg
    out["min_pos"][valid] = x[rows, arg]
    out["min_grad"][valid] = g[rows, arg]
    out["n_below"][valid] = np.count_nonzero(below, axis=1)
    out["cost"][valid] = ordered_sum(phi[:, :, None])[:, 0]
    out["frame_clearance"][valid] = fmin
    out["frame_cost"][valid] = fsum[:, :, 0]
    out["frame_grad"][valid] = fsum[:, :, 1:]
    out["sphere_clearance"][valid] = s
    out["cost_abs"][valid] = ordered_sum(phi[:, :, None])[:, 0]
    out["frame_cost_abs"][valid] = fabs[:, :, 0]
    out["frame_grad_abs"][valid] = fabs[:, :, 1:]
    return out
