"""The definition of fiesta_hip_view_coverage (include/fiesta_hip.h) in plain numpy over fiesta_amd.ray_walk and boolean class
arrays: every (usable view, listed member) pair is tested for range and field of view with the header's expressions, the survivors'
rays are walked by ray_walk and their voxels classified as the ray query classifies them.  Slow and obvious on purpose: the device
call (fiesta_amd/csrc/view_kernels.hpp) has to reproduce every output of this function bit for bit."""
from __future__ import annotations

import math

import numpy as np

from .esdf_map import RAY_FREE, RAY_MAX_COORD, RAY_OCCUPIED, RAY_OUTSIDE, RAY_UNKNOWN, ray_walk

VIEW_OMNI = 1                 # FIESTA_HIP_VIEW_OMNI
VIEW_MAX_COUNT = 2 ** 24      # entries, groups, members, views


def view_ring(radii, n_angles, heights):
    """A ring of candidate view offsets for the ring form: for every radius r, height h and angle phi = 2 pi i / n_angles the row
    (r cos phi, r sin phi, h, -cos phi, -sin phi) -- a pose on the circle that looks back at its centre.  (len(radii) * len(heights) *
    n_angles, 5) f64, ordered by radius, then height, then angle."""
    rows = []
    for r in np.atleast_1d(radii):
        for h in np.atleast_1d(heights):
            for i in range(int(n_angles)):
                phi = 2.0 * math.pi * i / int(n_angles)
                c, s = math.cos(phi), math.sin(phi)
                rows.append((float(r) * c, float(r) * s, float(h), -c, -s))
    return np.array(rows, np.float64).reshape(-1, 5)


def view_coverage_model(observed, occupied, origin, resolution, vox, pos=None, dir=None, group=None, centroid=None, ring=None, offsets=None,
                        members=None, n_groups=None, n_groups_effective=None, min_range=0.0, max_range=math.inf, tan_h=math.inf,
                        tan_v=math.inf, block_mask=RAY_OCCUPIED, omni=False, min_clearance=0.0, min_visible=1, dist=None,
                        origin_vox=(0, 0, 0), bounded=True, pos_range=None, walk_cache=None, want_pairs=False):
    """observed / occupied (and dist, the f64 array of GetDistance(Vector3i), needed only with min_clearance > 0): 3-D arrays indexed
    [x, y, z] whose element (0, 0, 0) is map voxel `origin_vox`; bounded / pos_range as in ray_query_model.  vox: (n, 3) target
    voxels.  Views: pos (V, 3), dir (V, 2), group (V,) -- or centroid (G, 3) and ring (M, 5).  offsets / members: the CSR pair, both
    optional; n_groups defaults to len(offsets) - 1 (1 without offsets); n_groups_effective: what a device counter would hold.
    walk_cache: a dict shared among calls (ray -> blocked-relevant walk).  Returns a dict: view_class, n_in_view, n_visible (V,);
    cover_count, first_view (n,); best_view, best_count (n_groups,); n_usable, n_pairs, pairs_in_view, pairs_visible; with want_pairs
    also `pairs`: per pair (view, entry, in_range, in_view, visible), entry -1 for a member index out of range."""
    obs = np.asarray(observed, dtype=bool)
    occ = np.asarray(occupied, dtype=bool)
    res = float(resolution)
    org = np.asarray(origin, dtype=np.float64).reshape(3)
    ov = np.asarray(origin_vox, dtype=np.int64).reshape(3)
    tv = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    n = len(tv)
    block_mask, min_visible = int(block_mask), int(min_visible)
    if not 0 <= block_mask <= 7 or min_visible < 1:
        raise ValueError("block_mask must be a subset of OCCUPIED | UNKNOWN | OUTSIDE, min_visible >= 1")
    if not (min_range >= 0 and max_range >= 0 and min_range <= max_range and tan_h >= 0 and tan_v >= 0):
        raise ValueError("0 <= min_range <= max_range and tangents >= 0 are required")
    if (pos is None) == (centroid is None):
        raise ValueError("exactly one view form must be given")
    if offsets is not None:
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        G = len(offsets) - 1 if n_groups is None else int(n_groups)
    else:
        G = 1
    if members is not None:
        members = np.asarray(members, dtype=np.int64).reshape(-1)
    n_members = n if members is None else len(members)
    if pos is None:
        cen = np.asarray(centroid, dtype=np.float64).reshape(-1, 3)[:G]
        rg = np.asarray(ring, dtype=np.float64).reshape(-1, 5)
        M = len(rg)
        pos = (cen[:, None, :] + rg[None, :, :3]).reshape(-1, 3)            # one add
        dir = np.broadcast_to(rg[None, :, 3:5], (G, M, 2)).reshape(-1, 2)
        group = np.repeat(np.arange(G, dtype=np.int64), M)
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    V = len(pos)
    if dir is None and not omni:
        raise ValueError("dir is required without omni")
    dir = None if dir is None else np.ascontiguousarray(dir, dtype=np.float64).reshape(V, 2)
    group = np.zeros(V, np.int64) if group is None else np.asarray(group, dtype=np.int64).reshape(V)
    if max(n, G, n_members, V) > VIEW_MAX_COUNT:
        raise ValueError("a count above 2^24")
    Ge = G if n_groups_effective is None else max(0, min(G, int(n_groups_effective)))
    p_all = (tv.astype(np.float64) + 0.5) * res + org                       # the targets' centres
    lo_r, hi_r = (org, org + (ov + np.array(obs.shape)) * res) if pos_range is None else [np.asarray(q, np.float64).reshape(3) for q in pos_range]

    def classes(W):
        """the ray query's class of every walk voxel of W (m, 3), and the map voxel of its centre"""
        W = np.asarray(W, np.int64).reshape(-1, 3)
        pc = (W.astype(np.float64) + 0.5) * res
        v = np.clip(np.floor((pc - org) / res), -(2.0 ** 31 - 1), 2.0 ** 31 - 1).astype(np.int64)
        idx = v - ov
        inside = np.all((idx >= 0) & (idx < np.array(obs.shape)), axis=1)
        ic = np.where(inside[:, None], idx, 0)
        o = obs[ic[:, 0], ic[:, 1], ic[:, 2]] & inside
        cls = np.where(o, np.where(occ[ic[:, 0], ic[:, 1], ic[:, 2]], RAY_OCCUPIED, RAY_FREE), RAY_UNKNOWN)
        if bounded:
            in_map = ~(np.any(pc < lo_r, axis=1) | np.any(pc > hi_r, axis=1))
            cls = np.where(in_map & inside, cls, RAY_OUTSIDE)
        return cls, v, ic

    def segment(g):
        if offsets is None:
            return 0, n_members
        lo, hi = (int(min(max(offsets[g + k], 0), n_members)) for k in (0, 1))
        return lo, max(hi, lo)

    out = {"view_class": np.zeros(V, np.uint8), "n_in_view": np.full(V, -1, np.int32), "n_visible": np.full(V, -1, np.int32),
           "cover_count": np.zeros(n, np.int32), "first_view": np.full(n, -1, np.int32), "best_view": np.full(G, -1, np.int64),
           "best_count": np.zeros(G, np.int32)}
    n_usable = n_pairs = tot_in = tot_vis = 0
    pairs = []
    cache = walk_cache if walk_cache is not None else {}
    min2, max2 = float(min_range) * float(min_range), float(max_range) * float(max_range)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for v in range(V):
            a = pos[v] / res
            if not (np.isfinite(pos[v]).all() and (np.abs(a) < RAY_MAX_COORD).all()):
                continue
            cls, mv, ic = classes(np.floor(a).astype(np.int64))
            out["view_class"][v] = cls[0]
            g = int(group[v])
            if cls[0] != RAY_FREE or not 0 <= g < Ge:
                continue
            if min_clearance > 0 and not np.asarray(dist, np.float64)[ic[0, 0], ic[0, 1], ic[0, 2]] >= min_clearance:
                continue
            n_usable += 1
            lo, hi = segment(g)
            ent = np.arange(lo, hi, dtype=np.int64) if members is None else members[lo:hi]
            n_pairs += len(ent)
            listed = (ent >= 0) & (ent < n)
            e = np.where(listed, ent, 0)
            q = p_all[e] - pos[v] if n else np.zeros((len(e), 3))
            q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
            d2 = q0 * q0 + q1 * q1 + q2 * q2
            in_range = listed & (min2 <= d2) & (d2 <= max2)
            if omni:
                in_view = np.abs(q2) <= tan_v * np.sqrt(q0 * q0 + q1 * q1)
            else:
                dx, dy = dir[v]
                fwd, lat = q0 * dx + q1 * dy, q1 * dx - q0 * dy
                in_view = (fwd > 0) & (np.abs(lat) <= tan_h * fwd) & (np.abs(q2) <= tan_v * fwd)
            in_view &= in_range
            visible = np.zeros(len(e), bool)
            at = np.flatnonzero(in_view)
            targets, which = np.unique(e[at], return_inverse=True)                  # (a target listed many times is walked once)
            seen_t = np.zeros(len(targets), bool)
            for k, t in enumerate(targets):
                b = p_all[t] / res
                key = (a.tobytes(), b.tobytes())
                if key not in cache:
                    w = ray_walk(a, b)
                    cache[key] = None if w is None else classes(w[:-1])[0]          # the last voxel is the target's own: never tested
                c = cache[key]
                seen_t[k] = c is not None and not np.any(c & block_mask)
            visible[at] = seen_t[which.reshape(-1)]
            out["n_in_view"][v], out["n_visible"][v] = int(in_view.sum()), int(visible.sum())
            tot_in += int(in_view.sum())
            tot_vis += int(visible.sum())
            seen = e[visible]
            np.add.at(out["cover_count"], seen, 1)
            fresh = seen[out["first_view"][seen] < 0]
            out["first_view"][fresh] = v                                            # (views in increasing order: the lowest index)
            if visible.sum() >= min_visible and visible.sum() > out["best_count"][g]:   # (strictly more: the lowest index wins a tie)
                out["best_view"][g], out["best_count"][g] = v, int(visible.sum())
            if want_pairs:
                pairs.append(np.stack([np.full(len(e), v, np.int64), np.where(listed, ent, -1), in_range, in_view, visible], 1))
    out.update(n_usable=n_usable, n_pairs=n_pairs, pairs_in_view=tot_in, pairs_visible=tot_vis)
    if want_pairs:
        out["pairs"] = np.concatenate(pairs) if pairs else np.zeros((0, 5), np.int64)
    return out
