"""The definition of fiesta_hip_path_refine (include/fiesta_hip.h) in numpy, and the glue from corridors to its bounds.

path_refine_model      the whole call: vectorised over the waypoints of the batch, a loop over the iterations; every operation in
                       the header's order, so every output except `cost` has the library's bits (the terms of `cost` have them too,
                       only the order of their sum is numpy's)
path_refine_gradient   G and J of one configuration (the rule test differentiates J numerically and compares)
corridor_bounds        per waypoint of a voxel polyline the box it may move in: its corridor box, intersected with the next box
                       where the path changes boxes
corridor_bounds_model  the definition of fiesta_hip_corridor_bounds, the same step on the device: a literal loop, explicit inset,
                       the per-waypoint box index, VOID_BROKEN, truncated corridors and the device variant's offset rules
"""
from __future__ import annotations

import numpy as np

REFINE_MAX_WAYPOINTS = 1024
REFINE_MAX_ITERATIONS = 1024
REFINE_OK = 0
REFINE_INVALID = 1
REFINE_MAX_COORD = 2.0 ** 40
BOUNDS_VOID_BROKEN = 1
_LIM = 2.0 ** 20


def _batch(waypoints, offsets, bounds):
    w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if len(off) < 1 or off[0] != 0 or off[-1] != len(w) or np.any(np.diff(off) < 0):
        raise ValueError("offsets: n_paths + 1 non-decreasing entries from 0 to n_waypoints")
    b = None
    if bounds is not None:
        b = np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1, 6)
        if len(b) != len(w):
            raise ValueError("bounds: one row of lo xyz, hi xyz per waypoint")
    return w, off, b


def _check_params(margin, w_obstacle, w_smooth, alpha, max_step, tolerance, iterations):
    ok = (np.isfinite(margin) and abs(margin) <= _LIM and 0 <= w_obstacle <= _LIM and 0 <= w_smooth <= _LIM and 0 < alpha <= _LIM
          and 0 < max_step <= _LIM and np.isfinite(tolerance) and tolerance >= 0
          and int(iterations) == iterations and 0 <= iterations <= REFINE_MAX_ITERATIONS)
    if not ok:
        raise ValueError("path refine: a parameter is outside its range (include/fiesta_hip.h: fiesta_hip_refine_params)")


def _layout(w, off, b):
    """path_of, interior (per waypoint) and invalid (per path)"""
    n_paths, m = len(off) - 1, np.diff(off)
    path_of = np.repeat(np.arange(n_paths), m)
    k = np.arange(len(w)) - off[:-1][path_of]                       # the waypoint's index in its path
    interior = (k >= 1) & (k <= m[path_of] - 2)
    with np.errstate(invalid="ignore"):
        bad_wp = ~np.all(np.abs(w) <= REFINE_MAX_COORD, axis=1)     # (a NaN fails the comparison)
        if b is not None:
            bad_wp |= interior & ~np.all(b[:, :3] <= b[:, 3:], axis=1)  # lo > hi, or a NaN
    invalid = m > REFINE_MAX_WAYPOINTS
    np.logical_or.at(invalid, path_of, bad_wp)
    return path_of, interior, invalid


def _second_differences(W, idx):
    """a_j of every waypoint (zero outside idx, the interior waypoints of the valid paths)"""
    a = np.zeros_like(W)
    a[idx] = (W[idx - 1] - 2.0 * W[idx]) + W[idx + 1]
    return a


def _sample(query, pos, margin):
    """(d, phi, gamma) at pos, the header's sample"""
    if len(pos) == 0:
        return np.zeros(0), np.zeros(0), np.zeros((0, 3))
    d, g = query(pos)
    d, g = np.asarray(d, np.float64).reshape(-1), np.asarray(g, np.float64).reshape(-1, 3)
    below = d < margin
    e = np.where(below, margin - d, 0.0)
    phi = e * e
    gam = np.where(below[:, None], (-2.0 * e)[:, None] * g, 0.0)
    return d, phi, gam


def _terms(query, W, idx, margin, w_obstacle, w_smooth):
    """e_i of the waypoints idx at the positions W"""
    _, phi, _ = _sample(query, W[idx], margin)
    a = _second_differences(W, idx)[idx]
    return w_obstacle * phi + w_smooth * ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def path_refine_model(query, waypoints, offsets, bounds=None, *, margin, w_obstacle, w_smooth, alpha, max_step, tolerance=0.0,
                      iterations):
    """fiesta_hip_path_refine in numpy.  `query(pos) -> (d, grad)` answers an (N, 3) batch: a map's GetDistWithGradTrilinear, or any
    callable.  Returns a dict of the seven outputs (waypoints (N, 3), cost (n_paths, 2), last_move, iterations, n_below, min_dist,
    status) and, for the tolerance of a comparison with another order of summation, cost_n and cost_abs ((n_paths, 2): the number of
    terms of each J and the sum of their magnitudes).  Two orders of summation differ by at most (n + 16) * 2^-52 * abs."""
    w, off, b = _batch(waypoints, offsets, bounds)
    margin, w_obstacle, w_smooth, alpha, max_step, tolerance = (float(v) for v in (margin, w_obstacle, w_smooth, alpha, max_step, tolerance))
    _check_params(margin, w_obstacle, w_smooth, alpha, max_step, tolerance, iterations)
    n_paths = len(off) - 1
    path_of, interior, invalid = _layout(w, off, b)
    valid_wp = ~invalid[path_of]
    inner = np.nonzero(interior & valid_wp)[0]                      # the waypoints that may move
    out = {"waypoints": w.copy(), "cost": np.zeros((n_paths, 2)), "last_move": np.zeros(n_paths), "iterations": np.zeros(n_paths, np.int32),
           "n_below": np.zeros(n_paths, np.int64), "min_dist": np.full(n_paths, np.inf), "status": np.where(invalid, REFINE_INVALID, REFINE_OK).astype(np.int32),
           "cost_n": np.zeros((n_paths, 2), np.int64), "cost_abs": np.zeros((n_paths, 2))}

    def J(W, col):
        e = _terms(query, W, inner, margin, w_obstacle, w_smooth)
        np.add.at(out["cost"][:, col], path_of[inner], e)
        np.add.at(out["cost_n"][:, col], path_of[inner], 1)
        np.add.at(out["cost_abs"][:, col], path_of[inner], np.abs(e))

    J(w, 0)
    W = w.copy()
    active = np.zeros(n_paths, bool)
    active[path_of[inner]] = True                                   # valid paths with an interior waypoint
    ws2 = 2.0 * w_smooth
    for _ in range(int(iterations)):
        idx = inner[active[path_of[inner]]]
        if len(idx) == 0:
            break
        _, _, gam = _sample(query, W[idx], margin)
        a = _second_differences(W, idx)
        s = (a[idx - 1] - 2.0 * a[idx]) + a[idx + 1]
        G = w_obstacle * gam + ws2 * s
        delta = alpha * G
        delta = np.where(delta > max_step, max_step, delta)
        delta = np.where(delta < -max_step, -max_step, delta)
        x = W[idx] - delta
        if b is not None:
            x = np.where(x < b[idx, :3], b[idx, :3], x)
            x = np.where(x > b[idx, 3:], b[idx, 3:], x)
        move = np.abs(x - W[idx])
        last = np.zeros(n_paths)
        np.maximum.at(last, path_of[idx], move.max(axis=1))
        W = W.copy()
        W[idx] = x
        out["last_move"][active] = last[active]
        out["iterations"][active] += 1
        active &= ~(last <= tolerance)
    J(W, 1)
    every = np.nonzero(valid_wp)[0]                                 # n_below and min_dist: ends included
    d, _, _ = _sample(query, W[every], margin)
    np.add.at(out["n_below"], path_of[every], (d < margin).astype(np.int64))
    np.minimum.at(out["min_dist"], path_of[every], d)
    out["waypoints"] = W
    out["cost"][invalid] = np.nan
    out["last_move"][invalid] = np.nan
    out["min_dist"][invalid] = np.nan
    out["iterations"][invalid] = -1
    out["n_below"][invalid] = -1
    return out


def path_refine_gradient(query, waypoints, offsets, *, margin, w_obstacle, w_smooth):
    """G ((N, 3): the header's G at every interior waypoint, zero rows at the ends and on invalid paths) and J ((n_paths,), NaN for
    an invalid path) of one configuration"""
    w, off, _ = _batch(waypoints, offsets, None)
    margin, w_obstacle, w_smooth = float(margin), float(w_obstacle), float(w_smooth)
    path_of, interior, invalid = _layout(w, off, None)
    idx = np.nonzero(interior & ~invalid[path_of])[0]
    _, _, gam = _sample(query, w[idx], margin)
    a = _second_differences(w, idx)
    G = np.zeros_like(w)
    G[idx] = w_obstacle * gam + (2.0 * w_smooth) * ((a[idx - 1] - 2.0 * a[idx]) + a[idx + 1])
    Jv = np.zeros(len(off) - 1)
    np.add.at(Jv, path_of[idx], _terms(query, w, idx, margin, w_obstacle, w_smooth))
    Jv[invalid] = np.nan
    return G, Jv


def _inside(vox, box):
    return bool(np.all(vox >= box[:3]) and np.all(vox <= box[3:]))


def corridor_bounds(waypoints_vox, offsets, corridor, inset=None):
    """The bounds of fiesta_hip_path_refine for voxel polylines and their corridors (`corridor`: what ESDFMap.PathCorridor returned for
    the same waypoints_vox and offsets, with boxes_pos).  Returns (bounds (N, 6) f64: lo xyz, hi xyz in metres, ok (n_paths,) bool).
    The chain index of waypoint i of a path is c_0 = 0, c_{i+1} = c_i + |w_{i+1} - w_i|_1; its box b(i) is the last box of its path
    with entry <= c_i; its bounds are boxes_pos[b(i)], intersected with boxes_pos[b(i) + 1] if b(i + 1) = b(i) + 1 (not empty:
    consecutive boxes of a corridor share a voxel).  A path whose corridor status is not OK, or with b(i + 1) > b(i) + 1 somewhere,
    gets ok = False, and its rows keep each waypoint's own box (NaN rows where the path has no box at all).  So does a path whose
    FIRST waypoint, which the refinement never moves, lies outside the box its successor changes to (b(1) = 1 and w_0 not in box 1;
    it cannot happen on a 6-connected path, whose new boxes are seeded with the chain voxel before them).
    inset (metres; None: 2^-20 of the voxel size, read off the first box) is taken off every UPPER face: a box's upper face is the
    lower face of the next voxel, and a waypoint clamped exactly onto it would be filed under that voxel by the point queries.
    Why this is safe: waypoints i and i + 1 of an ok path are both bounded to box b(i + 1) -- it is either i's own box or the one
    i's bounds were intersected with, and the two fixed ends lie in it as well -- so after any number of clamped steps the two still
    share a convex box of traversable voxels, and the whole segment between them lies in traversable space, whatever the obstacle
    cost does."""
    v = np.ascontiguousarray(waypoints_vox, dtype=np.int64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    boff = np.ascontiguousarray(corridor["offsets"], dtype=np.int64).reshape(-1)
    entry = np.asarray(corridor["entry"], dtype=np.int64).reshape(-1)
    pos = np.asarray(corridor["boxes_pos"], dtype=np.float64).reshape(-1, 6)
    boxes = np.asarray(corridor["boxes"], dtype=np.int64).reshape(-1, 6)
    status = np.asarray(corridor["status"]).reshape(-1)
    n_paths = len(off) - 1
    if len(boff) != n_paths + 1 or off[0] != 0 or off[-1] != len(v) or np.any(np.diff(off) < 0):
        raise ValueError("corridor_bounds: offsets and corridor do not describe the same batch")
    bounds = np.full((len(v), 6), np.nan)
    ok = np.zeros(n_paths, bool)
    for p in range(n_paths):
        o0, o1, b0, b1 = int(off[p]), int(off[p + 1]), int(boff[p]), int(boff[p + 1])
        ok[p] = status[p] == 0
        if o1 == o0 or b1 == b0:
            continue
        c = np.concatenate([[0], np.cumsum(np.abs(np.diff(v[o0:o1], axis=0)).sum(axis=1))])
        bi = np.searchsorted(entry[b0:b1], c, side="right") - 1   # the last box with entry <= c_i (entry[b0] = 0)
        rows = pos[b0 + bi].copy()
        if ok[p]:
            step = np.diff(bi)
            if np.any(step > 1) or (len(step) and step[0] == 1 and not _inside(v[o0], boxes[b0 + 1])):
                ok[p] = False
            else:
                nxt = np.nonzero(step == 1)[0]
                other = pos[b0 + bi[nxt] + 1]
                rows[nxt, :3] = np.maximum(rows[nxt, :3], other[:, :3])
                rows[nxt, 3:] = np.minimum(rows[nxt, 3:], other[:, 3:])
        bounds[o0:o1] = rows
    if inset is None:
        inset = (pos[0, 3] - pos[0, 0]) / float(boxes[0, 3] - boxes[0, 0] + 1) * 2.0 ** -20 if len(pos) else 0.0
    bounds[:, 3:] -= float(inset)
    return bounds, ok


def _flagged_offsets(off, n_wp):
    """path clearance's device offset rule: a path is valid iff its start is in range and is the running maximum of the in-range
    entries before it, and its end lies in [start, n_waypoints]"""
    o0, o1 = off[:-1], off[1:]
    run = np.maximum.accumulate(np.where((o0 >= 0) & (o0 <= n_wp), o0, np.iinfo(np.int64).min))
    return ~((o0 >= 0) & (o0 == run) & (o1 >= o0) & (o1 <= n_wp))


def corridor_bounds_model(waypoints_vox, offsets, corridor, inset, void_broken=False, n_boxes=None, device_offsets=False):
    """The definition of fiesta_hip_corridor_bounds (include/fiesta_hip.h): a literal loop over paths and waypoints.  `corridor` holds
    the corridor call's offsets, boxes, boxes_pos, entry and status for the batch (waypoints_vox, offsets); n_boxes (None: the rows
    boxes_pos holds) is the number of box rows present.  `inset` is explicit, in metres: the ABI has no default, the class methods'
    default is resolution * 2.0 ** -20 -- corridor_bounds' own inset=None divides the first box's width by its voxel count instead,
    whose bits can differ.  Returns dict(bounds (N, 6) f64, ok (n_paths,) int32, box (N,) int64).
    device_offsets=False is the host variant: offsets that break the CSR rules, or a box range that decreases, is negative or ends
    above n_boxes, raise ValueError (the whole-call error).  True is the _dev variant: such a path gets ok = 0, reads nothing, and
    its rows (as every row no valid path owns) are NaN with box -1.
    Against corridor_bounds with the same inset: bounds and ok are equal bit for bit wherever that function accepts the input, the
    arrays hold no negative zero (np.maximum and a comparison choose differently between +0 and -0) and entry[1] of a path is not
    0 (it tests the path's box 1 where rule 4 says b(0) + 1; the corridor call's entries increase strictly)."""
    v = np.ascontiguousarray(waypoints_vox, dtype=np.int64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    boff = np.ascontiguousarray(corridor["offsets"], dtype=np.int64).reshape(-1)
    entry = np.asarray(corridor["entry"], dtype=np.int64).reshape(-1)
    pos = np.asarray(corridor["boxes_pos"], dtype=np.float64).reshape(-1, 6)
    boxes = np.asarray(corridor["boxes"], dtype=np.int64).reshape(-1, 6)
    status = np.asarray(corridor["status"]).reshape(-1)
    inset = float(inset)
    if not (np.isfinite(inset) and inset >= 0):
        raise ValueError("corridor_bounds: inset must be finite and >= 0")
    n_paths, n_wp = len(off) - 1, len(v)
    n_boxes = len(pos) if n_boxes is None else int(n_boxes)
    if n_paths < 0 or len(boff) != n_paths + 1 or len(status) != n_paths or not 0 <= n_boxes <= min(len(pos), len(boxes), len(entry)):
        raise ValueError("corridor_bounds: offsets and corridor do not describe the same batch")
    flagged = _flagged_offsets(off, n_wp) if device_offsets else np.zeros(n_paths, bool)
    bad_box = (boff[:-1] < 0) | (boff[1:] < boff[:-1]) | (boff[1:] > n_boxes)
    if not device_offsets and n_paths > 0 and (off[0] != 0 or off[-1] != n_wp or np.any(np.diff(off) < 0) or bad_box.any()):
        raise ValueError("corridor_bounds: offsets break the CSR rules, or a box range decreases, is negative or ends above n_boxes")
    bounds = np.full((n_wp, 6), np.nan)
    box = np.full(n_wp, -1, np.int64)
    ok = np.zeros(n_paths, np.int32)
    for p in range(n_paths):
        if flagged[p] or bad_box[p]:
            continue
        o0, o1, b0, b1 = int(off[p]), int(off[p + 1]), int(boff[p]), int(boff[p + 1])
        good = int(status[p]) == 0
        ok[p] = good
        m, nb = o1 - o0, b1 - b0
        if m == 0 or nb == 0:
            continue
        c, b = 0, []
        for i in range(m):
            if i:
                c += int(np.abs(v[o0 + i] - v[o0 + i - 1]).sum())
            k = 0                                            # the last box with entry <= c_i, clamped into the path's range
            while k + 1 < nb and entry[b0 + k + 1] <= c:
                k += 1
            b.append(k)
        for i in range(m - 1):
            if b[i + 1] > b[i] + 1:
                good = False
        if m > 1 and b[1] == b[0] + 1 and not _inside(v[o0], boxes[b0 + b[0] + 1]):
            good = False
        ok[p] = good
        for i in range(m):
            row = pos[b0 + b[i]].copy()
            if good and i + 1 < m and b[i + 1] == b[i] + 1:
                other = pos[b0 + b[i] + 1]
                row[:3] = np.where(row[:3] > other[:3], row[:3], other[:3])
                row[3:] = np.where(row[3:] < other[3:], row[3:], other[3:])
            row[3:] = row[3:] - inset
            if void_broken and not good:
                row[:] = np.nan
            bounds[o0 + i] = row
            box[o0 + i] = b0 + b[i]
    return {"bounds": bounds, "ok": ok, "box": box}
