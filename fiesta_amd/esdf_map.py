"""Host-side mirror of the reference's operator API for the ESDF hot path.

``ESDFMap`` keeps the public method names, argument meaning and error conventions of
``class fiesta::ESDFMap`` (reference include/ESDFMap.h:111-166, src/ESDFMap.cpp) and forwards every
call through the C ABI of ``libfiesta_hip.so`` (include/fiesta_hip.h) to the HIP kernels.  Methods
accept either one voxel/position (scalar result, like the C++ class) or an (n,3) batch (array result);
the batch form is the fast path.  The reference is compiled C++; the C++ facade with the identical
class signature is include/fiesta/ESDFMap.h -- this module exists so that the parity tests and the
bench read like the reference's own driver (test/test_ESDF_Map.cpp:42-104).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import ArticulatedResult, BodyResult, SweepResult, ClusterInfo, ClusterResult, SplitInfo, SplitResult, ViewInfo, ViewResult, ViewSensor, ViewSet, Config, FiestaHipError, PathCostResult, PathResult, RaycastParams, RayResult, ReachInfo, ReachMatrixInfo, ReachMatrixResult, ReachPathsResult, LegPathsInfo, LegPathsResult, ReachResult, CorridorResult, FreeBoxesResult, RefineParams, RefineResult, TimingParams, TimingResult, BoundsResult, Stats, TourInfo, TourResult, check
from .refine_model import BOUNDS_VOID_BROKEN

UNDEFINED = -10000   # undefined_  (src/ESDFMap.cpp:182)
INFINITY = 10000     # infinity_   (src/ESDFMap.cpp:181)
D2_INF = 0x7FFFFFFF
# what `update_engine=None` means (the library itself reads no environment: the test suites switch this attribute to run
# every scenario on both UpdateESDF engines)
DEFAULT_UPDATE_ENGINE = 0


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _d3(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(3))


ENGINES = {"auto": 0, "rounds": 1, "bulk": 2, "levels": 3, "envelope": 4, "cells": 5, "masked": 6}

# fiesta_hip_path_result, in struct order: (name, dtype, per-path shape)
PATH_FIELDS = (("min_dist", np.float64, ()), ("min_index", np.int64, ()), ("min_pos", np.float64, (3,)),
               ("min_grad", np.float64, (3,)), ("first_below", np.int64, ()), ("first_below_pos", np.float64, (3,)),
               ("n_samples", np.int64, ()))
# the per-cluster arrays of fiesta_hip_cluster_result, in struct order (label before, offsets and members after them)
CLUSTER_FIELDS = (("size", np.int32, ()), ("root", np.int64, ()), ("box_lo", np.int32, (3,)), ("box_hi", np.int32, (3,)),
                  ("centroid", np.float64, (3,)), ("mask_or", np.uint8, ()), ("key_min", np.int32, ()), ("key_argmin", np.int64, ()))
# the per-part arrays of fiesta_hip_split_result, in struct order (offsets, members and label after them)
SPLIT_FIELDS = (("parent", np.int32, ()), ("depth", np.uint8, ())) + CLUSTER_FIELDS
SPLIT_INFO_KEYS = ("n_parts", "n_members", "n_split_clusters", "n_oversize", "largest", "deepest", "status")   # fiesta_hip_split_info, as the dicts name it
# the arrays of fiesta_hip_view_result, in struct order: (name, dtype, which count sizes it)
VIEW_FIELDS = (("view_class", np.uint8, "views"), ("n_in_view", np.int32, "views"), ("n_visible", np.int32, "views"),
               ("cover_count", np.int32, "entries"), ("first_view", np.int32, "entries"), ("best_view", np.int64, "groups"),
               ("best_count", np.int32, "groups"))
VIEW_INFO_KEYS = ("n_usable", "n_pairs", "pairs_in_view", "pairs_visible")   # fiesta_hip_view_info, as the dicts name it
PATH_MAX_RATIO = 2.0 ** 24  # a segment with L / step above this makes its path invalid


def path_samples(waypoints, offsets, step):
    """The sample rule of fiesta_hip_path_clearance (include/fiesta_hip.h) in numpy, bit for bit: for each segment a -> b of a
    path d = b - a, L = sqrt(d0*d0 + d1*d1 + d2*d2), S = max(1, ceil(L / step)), samples a + d * (k / S) for k < S; then the
    last waypoint itself.  Returns (positions, n_samples): the samples of every valid path, path after path, as an (N, 3) f64
    array, and per path its count (0: empty, -1: invalid -- a non-finite waypoint or a segment with L / step > 2^24; an invalid
    path contributes no positions).  Sample i of path p is positions[sum(max(n_samples[:p], 0)) + i]."""
    w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    step = float(step)
    if len(off) < 1 or off[0] != 0 or off[-1] != len(w) or np.any(np.diff(off) < 0):
        raise ValueError("offsets: n_paths + 1 non-decreasing entries from 0 to n_waypoints")
    if not (np.isfinite(step) and step > 0):
        raise ValueError("step must be finite and > 0")
    n_paths, nw = len(off) - 1, np.diff(off)
    path_of = np.repeat(np.arange(n_paths), nw)                      # the path of every waypoint
    last = np.zeros(len(w), bool)
    last[off[1:][nw > 0] - 1] = True                                 # the last waypoint of its path: no segment starts there
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.zeros_like(w)
        d[:-1] = w[1:] - w[:-1]
        L = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        q = L / step
        seg_ok = last | (q <= PATH_MAX_RATIO)
        S = np.where(last, 1, np.maximum(1, np.ceil(np.where(seg_ok, q, 0.0)))).astype(np.int64)
    bad_wp = ~np.all(np.isfinite(w), axis=1) | ~seg_ok
    bad = np.zeros(n_paths, bool)
    np.logical_or.at(bad, path_of, bad_wp)
    S[bad[path_of]] = 0                                              # an invalid path has no samples
    n_samples = np.zeros(n_paths, np.int64)
    np.add.at(n_samples, path_of, S)
    n_samples[bad] = -1
    idx = np.repeat(np.arange(len(w)), S)                            # the waypoint each sample starts from, in sample order
    k = np.arange(len(idx)) - np.repeat(np.cumsum(S) - S, S)
    with np.errstate(invalid="ignore", over="ignore"):
        t = k.astype(np.float64) / S[idx].astype(np.float64)
        pos = w[idx] + d[idx] * t[:, None]
    pos = np.where(last[idx][:, None], w[idx], pos)                  # the final sample: the last waypoint itself
    return np.ascontiguousarray(pos), n_samples


# fiesta_hip_path_cost_result, in struct order: (name, dtype, one row per "path" or per "waypoint", row shape)
PATH_COST_FIELDS = (("cost", np.float64, "path", ()), ("grad", np.float64, "waypoint", (3,)), ("length", np.float64, "path", ()),
                    ("n_below", np.int64, "path", ()), ("n_samples", np.int64, "path", ()))


# fiesta_hip_body_result, in struct order: (name, dtype, row shape; "K": one entry per sphere): one row per pose
BODY_FIELDS = (("min_clearance", np.float64, ()), ("min_sphere", np.int32, ()), ("min_pos", np.float64, (3,)), ("min_grad", np.float64, (3,)),
               ("n_below", np.int32, ()), ("cost", np.float64, ()), ("grad", np.float64, (6,)), ("sphere_clearance", np.float64, ("K",)))
# fiesta_hip_articulated_result, in struct order: (name, dtype, row shape; "K": one entry per sphere, "F": per frame): one row per configuration
ARTICULATED_FIELDS = (("min_clearance", np.float64, ()), ("min_sphere", np.int32, ()), ("min_pos", np.float64, (3,)),
                      ("min_grad", np.float64, (3,)), ("n_below", np.int32, ()), ("cost", np.float64, ()),
                      ("frame_clearance", np.float64, ("F",)), ("frame_cost", np.float64, ("F",)), ("frame_grad", np.float64, ("F", 6)),
                      ("sphere_clearance", np.float64, ("K",)))

# fiesta_hip_sweep_result, in struct order: (name, dtype, row shape): one row per path
SWEEP_FIELDS = (("min_clearance", np.float64, ()), ("min_sample", np.int64, ()), ("min_sphere", np.int32, ()), ("min_pose", np.float64, (7,)),
                ("min_pos", np.float64, (3,)), ("min_grad", np.float64, (3,)), ("first_below", np.int64, ()),
                ("first_below_sphere", np.int32, ()), ("first_below_pose", np.float64, (7,)), ("n_below", np.int64, ()),
                ("n_samples", np.int64, ()))


# fiesta_hip_refine_result, in struct order: (name, dtype, one row per "path" or per "waypoint", row shape)
REFINE_FIELDS = (("waypoints", np.float64, "waypoint", (3,)), ("cost", np.float64, "path", (2,)), ("last_move", np.float64, "path", ()),
                 ("iterations", np.int32, "path", ()), ("n_below", np.int64, "path", ()), ("min_dist", np.float64, "path", ()),
                 ("status", np.int32, "path", ()))

# fiesta_hip_path_timing_result, in struct order: (name, dtype, one row per "path" or per "waypoint", row shape)
TIMING_FIELDS = (("duration", np.float64, "path", ()), ("length", np.float64, "path", ()), ("n_samples", np.int64, "path", ()),
                 ("n_below", np.int64, "path", ()), ("min_speed", np.float64, "path", ()), ("min_index", np.int64, "path", ()),
                 ("status", np.int32, "path", ()), ("time", np.float64, "waypoint", ()), ("speed", np.float64, "waypoint", ()))
TIMING_PARAMS = ("step", "margin", "v_max", "v_min", "a_max", "corner_dev", "v_start", "v_end")   # fiesta_hip_timing_params, in struct order


def path_cost_model(query, waypoints, offsets, step, margin):
    """The definition of fiesta_hip_path_cost (include/fiesta_hip.h) in numpy over path_samples: every per-sample and per-segment
    TERM in the header's operation order (bit for bit what the library computes from the same (d, grad)), the sums over a segment's
    interior samples in numpy's order.  `query(pos) -> (d, grad)` answers an (N, 3) batch: a map's GetDistWithGradTrilinear, or any
    callable.  Returns a dict: the five outputs (cost, grad, length, n_below, n_samples) and, for the tolerance of a comparison with
    another order of summation, per float output component the number of summed terms and the sum of their absolute values on the
    output's own scale: cost_n / cost_abs and length_n / length_abs per path, grad_n per waypoint, grad_abs per waypoint and
    component.  Two orders of summation differ by at most (n + 16) * 2^-52 * abs."""
    w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    step, margin = float(step), float(margin)
    if not np.isfinite(margin):
        raise ValueError("margin must be finite")
    pos, ns = path_samples(w, off, step)
    if len(pos):
        d, g = query(pos)
        d, g = np.asarray(d, np.float64).reshape(-1), np.asarray(g, np.float64).reshape(-1, 3)
    else:
        d, g = np.zeros(0), np.zeros((0, 3))
    n_paths = len(ns)
    below = d < margin
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(below, margin - d, 0.0)
        phi_all = e * e
        gam_all = np.where(below[:, None], (-2.0 * e)[:, None] * g, 0.0)
    out = {"cost": np.zeros(n_paths), "grad": np.zeros((len(w), 3)), "length": np.zeros(n_paths),
           "n_below": np.zeros(n_paths, np.int64), "n_samples": ns.copy(),
           "cost_n": np.zeros(n_paths, np.int64), "cost_abs": np.zeros(n_paths), "length_n": np.zeros(n_paths, np.int64),
           "length_abs": np.zeros(n_paths), "grad_n": np.zeros(len(w), np.int64), "grad_abs": np.zeros((len(w), 3))}
    at = 0
    for p in range(n_paths):
        n = int(ns[p])
        if n < 0:
            out["cost"][p] = out["length"][p] = np.nan
            out["n_below"][p] = -1
            continue
        if n == 0:
            continue
        o0, o1 = int(off[p]), int(off[p + 1])
        phi, gam = phi_all[at:at + n], gam_all[at:at + n]
        out["n_below"][p] = int(np.count_nonzero(below[at:at + n]))
        at += n
        if o1 - o0 < 2:
            continue
        a = w[o0:o1]
        dd = a[1:] - a[:-1]
        L = np.sqrt(dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2])
        S = np.maximum(1, np.ceil(L / step)).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(S)])           # sample 0 of every segment, then the final sample: the waypoints
        assert first[-1] + 1 == n
        sidx = np.repeat(np.arange(len(S)), S)
        k = np.arange(n - 1) - first[sidx]
        Sd = S.astype(np.float64)
        t = k.astype(np.float64) / Sd[sidx]
        r = 1.0 - t
        inner = (k > 0)[:, None]
        terms = np.where(inner, np.concatenate([phi[:-1, None], r[:, None] * gam[:-1], t[:, None] * gam[:-1]], 1), 0.0)
        sums = np.add.reduceat(terms, first[:-1], axis=0)       # P, A[3], B[3] per segment
        asums = np.add.reduceat(np.abs(terms), first[:-1], axis=0)
        ra_phi, rb_phi, ra_gam, rb_gam = phi[first[:-1]], phi[first[1:]], gam[first[:-1]], gam[first[1:]]
        ok = L > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            h = L / Sd
            Q = (ra_phi * 0.5 + sums[:, 0]) + rb_phi * 0.5
            qs = Q / Sd
            u = dd / L[:, None]
            hq = np.where(ok, h * Q, 0.0)
            N = np.where(ok[:, None], h[:, None] * (ra_gam * 0.5 + sums[:, 1:4]) - qs[:, None] * u, 0.0)
            E = np.where(ok[:, None], h[:, None] * (sums[:, 4:7] + rb_gam * 0.5) + qs[:, None] * u, 0.0)
            absN = np.where(ok[:, None], h[:, None] * (np.abs(ra_gam) * 0.5 + asums[:, 1:4]) + np.abs(qs[:, None] * u), 0.0)
            absE = np.where(ok[:, None], h[:, None] * (asums[:, 4:7] + np.abs(rb_gam) * 0.5) + np.abs(qs[:, None] * u), 0.0)
            absQ = np.where(ok, h * (np.abs(ra_phi) * 0.5 + asums[:, 0] + np.abs(rb_phi) * 0.5), 0.0)
        zero = np.zeros((1, 3))
        out["cost"][p] = np.cumsum(hq)[-1]                      # (cumsum adds in segment order)
        out["length"][p] = np.cumsum(L)[-1]
        out["grad"][o0:o1] = np.concatenate([N, zero]) + np.concatenate([zero, E])
        out["cost_n"][p], out["cost_abs"][p] = int((S + 1).sum()), absQ.sum()
        out["length_n"][p], out["length_abs"][p] = len(L), L.sum()
        out["grad_abs"][o0:o1] = np.concatenate([absN, zero]) + np.concatenate([zero, absE])
        out["grad_n"][o0:o1] = np.concatenate([S + 2, [0]]) + np.concatenate([[0], S + 2])
    return out


def frontier_model(observed, occupied, dist=None, lo=None, hi=None, min_clearance=0.0, origin_vox=(0, 0, 0), bounded=True):
    """The definition of fiesta_hip_get_frontier_voxels (include/fiesta_hip.h) in numpy, over 3-D boolean arrays indexed [x, y, z]
    whose element (0, 0, 0) is map voxel `origin_vox`: the observed, unoccupied voxels with a never-observed 6-neighbour, inside the
    inclusive map-voxel box [lo, hi] (None: everything), and -- only if min_clearance > 0 -- with dist >= min_clearance (`dist`: the
    f64 array of GetDistance(Vector3i)).  A neighbour outside the array is not unknown when `bounded` (a dense map's outer face is no
    frontier) and unknown otherwise (a hash-block map scattered into a padded array).  Returns (vox (n, 3) int32 in map voxel
    coordinates, mask (n,) uint8: bit 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z), sorted lexicographically by (x, y, z)."""
    obs = np.asarray(observed, dtype=bool)
    free = obs & ~np.asarray(occupied, dtype=bool)
    unknown = np.pad(~obs, 1, constant_values=not bounded)   # unknown[i + 1, j + 1, k + 1] belongs to voxel (i, j, k)
    nx, ny, nz = obs.shape
    mask = np.zeros(obs.shape, np.uint8)
    for bit, (dx, dy, dz) in enumerate(((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))):
        nb = unknown[1 + dx:1 + dx + nx, 1 + dy:1 + dy + ny, 1 + dz:1 + dz + nz]
        mask |= (nb & free).astype(np.uint8) << bit
    keep = mask != 0
    org = np.asarray(origin_vox, dtype=np.int64).reshape(3)
    if lo is not None or hi is not None:
        if lo is None or hi is None:
            raise ValueError("lo and hi must both be given or both be None")
        lo = np.asarray(lo, dtype=np.int64).reshape(3) - org
        hi = np.asarray(hi, dtype=np.int64).reshape(3) - org
        ix, iy, iz = np.ogrid[:nx, :ny, :nz]
        keep &= (ix >= lo[0]) & (ix <= hi[0]) & (iy >= lo[1]) & (iy <= hi[1]) & (iz >= lo[2]) & (iz <= hi[2])
    if min_clearance > 0:
        keep &= np.asarray(dist, dtype=np.float64) >= min_clearance
    idx = np.argwhere(keep)                                   # (row-major: sorted by x, then y, then z)
    return (idx + org).astype(np.int32).reshape(-1, 3), mask[keep].astype(np.uint8)


# fiesta_hip_ray_query (include/fiesta_hip.h): the classes, the result struct in its order (name, dtype, per-ray shape), the limits
RAY_FREE, RAY_OCCUPIED, RAY_UNKNOWN, RAY_OUTSIDE = 0, 1, 2, 4
RAY_FIELDS = (("n_visited", np.int32, ()), ("hit_index", np.int32, ()), ("hit_class", np.uint8, ()), ("hit_vox", np.int32, (3,)),
              ("hit_dist", np.float64, ()), ("counts", np.int32, (4,)))
RAY_MAX_COORD = 2.0 ** 30     # |start / resolution| and |end / resolution| stay below it
RAY_MAX_MANHATTAN = 4095      # voxel steps between the two ends
RAY_MAX_STEPS = 8192          # the traversal's own loop bound
RAY_NO_VOXEL = -2 ** 31


def _ray_first_crossing(s, ds):
    """intbound (reference src/raycast.cpp:14-23) with mod (:10-12); a zero ds divides a positive number by +0"""
    if ds < 0:
        s, ds = -s, -ds
    w = math.fmod(math.fmod(s, 1.0) + 1.0, 1.0)
    return (1 - w) / ds if ds != 0 else math.inf


def ray_walk(a, b):
    """The walk W of fiesta_hip_ray_query (include/fiesta_hip.h) for a ray from a to b, both in VOXEL units (position / resolution),
    in plain Python floats (f64, every operation rounded once): the definition.  The reference's Raycast (src/raycast.cpp:56-158)
    without clipping box and without its 1500-voxel exception, at most 8192 iterations, then the last voxel replaced by floor(b);
    [floor(b)] if both ends lie in one voxel.  Returns an (m, 3) int64 array from start to end, or None for an invalid ray (a
    non-finite component, one at or beyond 2^30, more than 4095 voxel steps between the ends)."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    if not all(math.isfinite(v) and abs(v) < RAY_MAX_COORD for v in a + b):
        return None
    c, e = [math.floor(v) for v in a], [math.floor(v) for v in b]
    if sum(abs(e[i] - c[i]) for i in range(3)) > RAY_MAX_MANHATTAN:
        return None
    r0, r1, r2 = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    reach2 = r0 * r0 + r1 * r1 + r2 * r2
    step, tmax, tstep = [0] * 3, [0.0] * 3, [0.0] * 3
    for i in range(3):
        delta = float(e[i] - c[i])      # the integer voxel delta, not the true direction (:89-91)
        step[i] = (delta > 0) - (delta < 0)
        tmax[i] = _ray_first_crossing(a[i], delta)
        tstep[i] = step[i] / delta if delta != 0 else math.nan
    out = []
    if step != [0, 0, 0]:
        for _ in range(RAY_MAX_STEPS):
            out.append(tuple(c))
            q0, q1, q2 = c[0] - a[0], c[1] - a[1], c[2] - a[2]
            if q0 * q0 + q1 * q1 + q2 * q2 > reach2 or c == e:
                break
            if tmax[0] < tmax[1]:       # strict '<' tie rules (:139-157)
                ax = 0 if tmax[0] < tmax[2] else 2
            else:
                ax = 1 if tmax[1] < tmax[2] else 2
            c[ax] += step[ax]
            tmax[ax] += tstep[ax]
    if out:
        out[-1] = tuple(e)
    else:
        out = [tuple(e)]
    return np.array(out, np.int64).reshape(-1, 3)


def ray_walks(start, end, resolution):
    """ray_walk of every ray of an (n, 3) batch in metres: a = start / resolution, b = end / resolution.  A list (None: invalid)."""
    s = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(s).all(1) & np.isfinite(t).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = s / float(resolution), t / float(resolution)
    return [ray_walk(a[i], b[i]) if ok[i] else None for i in range(len(s))]


def ray_query_model(observed, occupied, origin, resolution, start, end, stop_mask, origin_vox=(0, 0, 0), bounded=True, pos_range=None,
                    walks=None):
    """The definition of fiesta_hip_ray_query (include/fiesta_hip.h) in numpy over ray_walk: `observed` / `occupied` are 3-D boolean
    arrays indexed [x, y, z] whose element (0, 0, 0) is map voxel `origin_vox` (a dense map: download_field's d2 >= 0 and occ; a
    hash-block map: download_hash scattered into an array), `origin` / `resolution` the map's.  bounded: a voxel outside the array,
    or whose centre lies outside pos_range = (lo, hi) in metres (PosInMap; a dense map's (origin, origin + map_size), which is also
    the default with map_size = (origin_vox + shape) * resolution), is OUTSIDE; not bounded: it is UNKNOWN and there is no OUTSIDE.  `walks`: the
    result of ray_walks for these rays, to share it among calls.  Returns a dict of the six outputs, bit for bit the library's."""
    obs = np.asarray(observed, dtype=bool)
    occ = np.asarray(occupied, dtype=bool)
    res = float(resolution)
    org = np.asarray(origin, dtype=np.float64).reshape(3)
    ov = np.asarray(origin_vox, dtype=np.int64).reshape(3)
    s = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 3)
    stop_mask = int(stop_mask)
    if len(s) != len(t) or not 0 <= stop_mask <= 7:
        raise ValueError("start and end need the same length, stop_mask a subset of OCCUPIED | UNKNOWN | OUTSIDE")
    n = len(s)
    if walks is None:
        walks = ray_walks(s, t, res)
    out = {"n_visited": np.full(n, -1, np.int32), "hit_index": np.full(n, -1, np.int32), "hit_class": np.zeros(n, np.uint8),
           "hit_vox": np.full((n, 3), RAY_NO_VOXEL, np.int32), "hit_dist": np.full(n, np.nan), "counts": np.zeros((n, 4), np.int32)}
    valid = np.array([w is not None for w in walks], bool)
    if not valid.any():
        return out
    rays = np.flatnonzero(valid)
    lens = np.array([len(walks[i]) for i in rays], np.int64)
    first = np.concatenate([[0], np.cumsum(lens)])               # walk of rays[j]: rows first[j] .. first[j + 1] - 1
    W = np.concatenate([walks[i] for i in rays])
    p = (W.astype(np.float64) + 0.5) * res                       # the centres
    v = np.clip(np.floor((p - org) / res), -(2.0 ** 31 - 1), 2.0 ** 31 - 1).astype(np.int64)   # Pos2Vox, saturated
    idx = v - ov
    inside = np.all((idx >= 0) & (idx < np.array(obs.shape)), axis=1)
    ic = np.where(inside[:, None], idx, 0)
    o = obs[ic[:, 0], ic[:, 1], ic[:, 2]] & inside
    cls = np.where(o, np.where(occ[ic[:, 0], ic[:, 1], ic[:, 2]], RAY_OCCUPIED, RAY_FREE), RAY_UNKNOWN)
    if bounded:
        lo, hi = (org, org + (ov + np.array(obs.shape)) * res) if pos_range is None else [np.asarray(q, np.float64).reshape(3) for q in pos_range]
        in_map = ~(np.any(p < lo, axis=1) | np.any(p > hi, axis=1))
        cls = np.where(in_map & inside, cls, RAY_OUTSIDE)
    N = len(W)
    at = np.where((cls & stop_mask) != 0, np.arange(N), N)
    hit = np.minimum.reduceat(at, first[:-1])                    # row of the first blocking voxel of each walk; >= its end: none
    has = hit < first[1:]
    stop = np.where(has, hit, first[1:])                         # the rows before it are counted
    out["hit_index"][rays] = np.where(has, hit - first[:-1], -1)
    out["n_visited"][rays] = np.where(has, hit - first[:-1] + 1, lens)
    h = hit[has]
    out["hit_class"][rays[has]] = cls[h]
    out["hit_vox"][rays[has]] = v[h]
    q = p[h] - s[rays[has]]
    out["hit_dist"][rays[has]] = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])
    for k, c in enumerate((RAY_FREE, RAY_OCCUPIED, RAY_UNKNOWN, RAY_OUTSIDE)):
        cs = np.concatenate([[0], np.cumsum(cls == c)])
        out["counts"][rays, k] = cs[stop] - cs[first[:-1]]
    return out


class ESDFMap:
    """Drop-in for ``fiesta::ESDFMap``; array mode by default, hash-block mode with ``mode="hash"``."""

    def __init__(self, origin, resolution, map_size=None, reserve_size=0, mode="array", device=0,
                 update_engine=None, shard_lo=None, global_grid=None):
        self._lib = _lib.load()
        cfg = Config()
        cfg.mode = 0 if mode == "array" else 1
        cfg.device = int(device)
        cfg.origin[:] = list(_d3(origin))
        cfg.resolution = float(resolution)
        cfg.map_size[:] = list(_d3(map_size if map_size is not None else (0, 0, 0)))
        cfg.reserve_size = int(reserve_size)
        if update_engine is None or update_engine == 0 or update_engine == "auto":
            update_engine = DEFAULT_UPDATE_ENGINE
        cfg.update_engine = ENGINES.get(update_engine, update_engine)
        if shard_lo is not None:
            cfg.shard_lo[:] = [int(v) for v in shard_lo]
            cfg.global_grid[:] = [int(v) for v in global_grid]
        self.mode = mode
        self.device = int(device)
        self._frontier_buffers, self._frontier_capacity = None, 1 << 16   # FrontierClusters' device buffers
        self._view_cluster_capacity = 1024                                # FrontierViews: clusters that get views
        self._view_ring = None                                            # FrontierViews: (the ring's bytes, its device copy)
        self.resolution = float(resolution)
        self.origin = _d3(origin)
        # PosInMap's range of an array-mode map as the library adds it up (ray_query_model's pos_range); a shard: the global map's
        self.pos_range = (self.origin, self.origin + (np.array(global_grid, np.float64) * float(resolution) if shard_lo is not None
                                                      else _d3(cfg.map_size[:])))
        self._h = C.c_void_p()
        check(self._lib.fiesta_hip_create(C.byref(cfg), C.byref(self._h)))
        gs = np.zeros(3, np.int32)
        check(self._lib.fiesta_hip_grid_size(self._h, _p(gs)))
        self.grid_size = tuple(int(v) for v in gs)
        self.last_insert = self.last_delete = 0
        self.served = {"levels": 0, "rounds": 0, "bulk": 0}   # UpdateESDF calls with work, by the engine that served them

    # -- life cycle ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.fiesta_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def grid_total_size_(self) -> int:  # public data member of the array build (include/ESDFMap.h:115)
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_grid_total_size(self._h, C.byref(n)))
        return n.value

    # -- parameters / window ------------------------------------------------------------------------
    def SetParameters(self, p_hit, p_miss, p_min, p_max, p_occ):
        check(self._lib.fiesta_hip_set_prob_params(self._h, p_hit, p_miss, p_min, p_max, p_occ))

    def SetUpdateRange(self, min_pos, max_pos, new_vec=True):
        check(self._lib.fiesta_hip_set_update_range(self._h, _p(_d3(min_pos)), _p(_d3(max_pos)), int(bool(new_vec))))

    def SetOriginalRange(self):
        check(self._lib.fiesta_hip_set_original_range(self._h))

    def set_update_engine(self, update_engine):
        """"auto" / "rounds" / "bulk" / "levels" / "envelope" / "cells" / "masked" (0 ... 6) from the next UpdateESDF on."""
        check(self._lib.fiesta_hip_set_update_engine(self._h, ENGINES.get(update_engine, update_engine)))

    # -- occupancy ingest ----------------------------------------------------------------------------
    def SetOccupancy(self, where, occ, want_ret=True):
        """SetOccupancy(Vector3i|Vector3d, int).  Integer input -> voxel overload, float -> position."""
        a = np.asarray(where)
        scalar = a.ndim == 1
        if np.issubdtype(a.dtype, np.integer):
            v = np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 3)
            fn = self._lib.fiesta_hip_set_occupancy_vox
        else:
            v = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
            fn = self._lib.fiesta_hip_set_occupancy_pos
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(occ, dtype=np.int32), (len(v),)))
        ret = np.empty(len(v), np.int32) if want_ret else None
        check(fn(self._h, _p(v), _p(o), len(v), _p(ret)))
        if ret is None:
            return None
        return int(ret[0]) if scalar else ret

    def SetOccupancyDevice(self, vox_dev_ptr: int, occ_dev_ptr: int, n: int):
        """Batch already resident in HBM (n x 3 int32 voxels, n int32 flags)."""
        check(self._lib.fiesta_hip_set_occupancy_vox_dev(self._h, C.c_void_p(vox_dev_ptr), C.c_void_p(occ_dev_ptr), n))

    def SetOccupancyBox(self, lo, hi, occ):
        """SetOccupancy(Vector3i, occ) for every voxel of the inclusive voxel box [lo, hi], on the device."""
        a = np.ascontiguousarray(lo, dtype=np.int32).reshape(3)
        b = np.ascontiguousarray(hi, dtype=np.int32).reshape(3)
        check(self._lib.fiesta_hip_set_occupancy_box(self._h, _p(a), _p(b), int(occ)))

    def CheckUpdate(self) -> bool:
        out = C.c_int32(0)
        check(self._lib.fiesta_hip_check_update(self._h, C.byref(out)))
        return bool(out.value)

    def UpdateOccupancy(self, global_map=True) -> bool:
        ni, nd, any_ = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(self._lib.fiesta_hip_update_occupancy(self._h, int(bool(global_map)), C.byref(ni), C.byref(nd),
                                                    C.byref(any_)))
        self.last_insert, self.last_delete = ni.value, nd.value
        return bool(any_.value)

    def UpdateESDF(self) -> dict:
        st = Stats()
        check(self._lib.fiesta_hip_update_esdf(self._h, C.byref(st)))
        d = st.as_dict()
        if d["inserted"] or d["deleted"] or d["rounds"] or d["bulk"]:   # (an update that had something to do)
            self.served["bulk" if d["bulk"] else "levels" if d["levels"] else "rounds"] += 1
        return d

    def level_trace(self):
        """The last level-engine update, level by level: [(frontier entries, microseconds inside the kernel), ...] for its
        first 48 levels, and the number of levels it ran (fiesta_hip_level_trace)."""
        out = (C.c_uint32 * 48)()
        n = C.c_int32(0)
        check(self._lib.fiesta_hip_level_trace(self._h, out, C.byref(n)))
        return [(int(w) >> 16, (int(w) & 0xFFFF) / 100.0) for w in list(out)[: min(n.value, 48)]], n.value

    def level_tuning(self, grid_groups=-1, spin_limit=-1):
        """Diagnostics of the level engine's wide levels (fiesta_hip_level_tuning): work-groups that take part (0: off), polls
        a barrier among them waits before the update is given up (0: at once)."""
        check(self._lib.fiesta_hip_level_tuning(self._h, int(grid_groups), int(spin_limit)))

    @property
    def only_levels(self) -> bool:
        """Every UpdateESDF of this map so far that had work ran the level engine from start to end (fiesta_hip_stats.levels):
        what the parity tests key their contract on (tests/scenarios.py: assert_envelope)."""
        return self.served["rounds"] == 0 and self.served["bulk"] == 0

    # -- ray casting -----------------------------------------------------------------------------------
    def RaycastFrame(self, points, transform, origin, min_ray_length, max_ray_length, l_cornor, r_cornor,
                     dedup=1, inverse=0):
        """One frame of Fiesta::RaycastProcess (include/Fiesta.h:194-278) on sensor-frame points.  inverse=1: this map
        is the SIGNED_NEEDED companion (inv_esdf_map_, :216-218, :249-251) -- end points free, crossed voxels occupied."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(transform, dtype=np.float64).reshape(16)
        prm = RaycastParams(min_ray_length, max_ray_length, (C.c_double * 3)(*l_cornor),
                            (C.c_double * 3)(*r_cornor), int(dedup), int(inverse))
        check(self._lib.fiesta_hip_raycast_frame(self._h, _p(pts), len(pts), _p(T), _p(_d3(origin)), C.byref(prm)))

    def RaycastDepth(self, depth_mm, fx, fy, cx, cy, transform, origin, min_ray_length, max_ray_length,
                     l_cornor, r_cornor, dedup=1, inverse=0):
        """uint16 millimetre depth image -> points (include/Fiesta.h:341-351) -> ray cast, all on device."""
        d = np.ascontiguousarray(depth_mm, dtype=np.uint16)
        T = np.ascontiguousarray(transform, dtype=np.float64).reshape(16)
        prm = RaycastParams(min_ray_length, max_ray_length, (C.c_double * 3)(*l_cornor),
                            (C.c_double * 3)(*r_cornor), int(dedup), int(inverse))
        check(self._lib.fiesta_hip_raycast_depth(self._h, _p(d), d.shape[0], d.shape[1], fx, fy, cx, cy, _p(T),
                                                 _p(_d3(origin)), C.byref(prm)))

    @staticmethod
    def _depth_filter(rel_transform, tolerance, max_dist, min_dist, margin, reset):
        from ._lib import DepthFilter
        f = DepthFilter(tolerance, max_dist, min_dist, int(margin), int(bool(reset)))
        f.rel_transform[:] = list(np.asarray(rel_transform, np.float64).reshape(16))
        return f

    def RaycastDepthFiltered(self, depth_mm, fx, fy, cx, cy, transform, origin, min_ray_length, max_ray_length, l_cornor,
                             r_cornor, rel_transform, tolerance=0.1, max_dist=10.0, min_dist=0.1, margin=0, reset=False,
                             dedup=1):
        """RaycastDepth with DepthConversion's temporal consistency filter (include/Fiesta.h:352-379); rel_transform =
        inv(last_transform) @ transform. The previous image lives on the device; the first image of a run casts nothing."""
        d = np.ascontiguousarray(depth_mm, dtype=np.uint16)
        T = np.ascontiguousarray(transform, dtype=np.float64).reshape(16)
        prm = RaycastParams(min_ray_length, max_ray_length, (C.c_double * 3)(*l_cornor),
                            (C.c_double * 3)(*r_cornor), int(dedup), 0)
        f = self._depth_filter(rel_transform, tolerance, max_dist, min_dist, margin, reset)
        check(self._lib.fiesta_hip_raycast_depth_filtered(self._h, _p(d), d.shape[0], d.shape[1], fx, fy, cx, cy, _p(T),
                                                          _p(_d3(origin)), C.byref(prm), C.byref(f)))

    def DepthConversion(self, depth_mm, fx, fy, cx, cy, rel_transform=None, tolerance=0.1, max_dist=10.0, min_dist=0.1,
                        margin=0, reset=False):
        """Fiesta::DepthConversion: (rows*cols x 3 float32 points with NaN where the filter rejected, surviving count)."""
        d = np.ascontiguousarray(depth_mm, dtype=np.uint16)
        out = np.empty((d.shape[0] * d.shape[1], 3), np.float32)
        n = C.c_int64(0)
        f = None if rel_transform is None else self._depth_filter(rel_transform, tolerance, max_dist, min_dist, margin, reset)
        check(self._lib.fiesta_hip_depth_conversion(self._h, _p(d), d.shape[0], d.shape[1], fx, fy, cx, cy,
                                                    C.byref(f) if f is not None else None, _p(out), C.byref(n)))
        return out, n.value

    # -- queries ------------------------------------------------------------------------------------------
    def _query(self, where, fn_vox, fn_pos, out_dtype):
        a = np.asarray(where)
        scalar = a.ndim == 1
        if np.issubdtype(a.dtype, np.integer):
            v = np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 3)
            fn = fn_vox
        else:
            v = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
            fn = fn_pos
        out = np.empty(len(v), out_dtype)
        check(fn(self._h, _p(v), len(v), _p(out)))
        return out[0].item() if scalar else out

    def GetDistance(self, where):
        return self._query(where, self._lib.fiesta_hip_get_distance_vox, self._lib.fiesta_hip_get_distance_pos,
                           np.float64)

    def GetOccupancy(self, where):
        return self._query(where, self._lib.fiesta_hip_get_occupancy_vox, self._lib.fiesta_hip_get_occupancy_pos,
                           np.int32)

    def GetDistWithGradTrilinear(self, pos):
        a = np.asarray(pos, dtype=np.float64)
        scalar = a.ndim == 1
        v = np.ascontiguousarray(a).reshape(-1, 3)
        dist = np.empty(len(v), np.float64)
        grad = np.zeros((len(v), 3), np.float64)
        check(self._lib.fiesta_hip_get_dist_grad(self._h, _p(v), len(v), _p(dist), _p(grad)))
        return (float(dist[0]), grad[0]) if scalar else (dist, grad)

    def GetDistWithGradTrilinearDevice(self, pos_dev_ptr: int, n: int, dist_dev_ptr: int, grad_dev_ptr: int = 0):
        """device-resident batch (n x 3 f64 positions, n f64 distances, n x 3 f64 gradients or 0): the planner-side fast path"""
        check(self._lib.fiesta_hip_get_dist_grad_dev(self._h, C.c_void_p(pos_dev_ptr), n, C.c_void_p(dist_dev_ptr),
                                                     C.c_void_p(grad_dev_ptr) if grad_dev_ptr else None))

    def PathClearance(self, waypoints, offsets, step, margin=0.0) -> dict:
        """fiesta_hip_path_clearance: per path (CSR `offsets` over `waypoints`) the minimum of GetDistWithGradTrilinear over its
        samples (path_samples), its first index, position and gradient, and the first sample below `margin` -- a dict of numpy
        arrays named as the fields of fiesta_hip_path_result"""
        w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1:
            raise ValueError("offsets needs n_paths + 1 entries")
        n = len(off) - 1
        out = {name: np.empty((n,) + shape, dtype) for name, dtype, shape in PATH_FIELDS}
        res = PathResult(*[out[name].ctypes.data for name, _, _ in PATH_FIELDS])
        check(self._lib.fiesta_hip_path_clearance(self._h, _p(w), len(w), _p(off), n, float(step), float(margin), C.byref(res)))
        return out

    def PathClearanceDevice(self, waypoints_dev_ptr: int, n_waypoints: int, offsets_dev_ptr: int, n_paths: int, step, margin=0.0,
                            out=None):
        """fiesta_hip_path_clearance_dev: inputs and outputs resident on the device (n_waypoints x 3 f64, n_paths + 1 int64;
        `out` maps field names of fiesta_hip_path_result to device pointers, missing fields are not written); only enqueued"""
        out = out or {}
        res = PathResult(*[int(out.get(name, 0)) or None for name, _, _ in PATH_FIELDS])
        check(self._lib.fiesta_hip_path_clearance_dev(self._h, C.c_void_p(waypoints_dev_ptr), int(n_waypoints),
                                                      C.c_void_p(offsets_dev_ptr), int(n_paths), float(step), float(margin),
                                                      C.byref(res)))

    def PathCost(self, waypoints, offsets, step, margin) -> dict:
        """fiesta_hip_path_cost: per path (CSR `offsets` over `waypoints`) the penalty (margin - d)^2 of GetDistWithGradTrilinear
        below `margin`, integrated along the polyline by the trapezoid rule over path_samples, and its derivative with respect to
        every waypoint -- a dict of numpy arrays named as the fields of fiesta_hip_path_cost_result (grad: one row per waypoint)"""
        w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1:
            raise ValueError("offsets needs n_paths + 1 entries")
        n = len(off) - 1
        out = {name: np.empty((n if per == "path" else len(w),) + shape, dtype) for name, dtype, per, shape in PATH_COST_FIELDS}
        res = PathCostResult(*[out[name].ctypes.data for name, _, _, _ in PATH_COST_FIELDS])
        check(self._lib.fiesta_hip_path_cost(self._h, _p(w), len(w), _p(off), n, float(step), float(margin), C.byref(res)))
        return out

    def PathCostDevice(self, waypoints_dev_ptr: int, n_waypoints: int, offsets_dev_ptr: int, n_paths: int, step, margin, out=None):
        """fiesta_hip_path_cost_dev: inputs and outputs resident on the device (`out` maps field names of
        fiesta_hip_path_cost_result to device pointers, missing fields are not written); only enqueued on the map's stream"""
        out = out or {}
        res = PathCostResult(*[int(out.get(name, 0)) or None for name, _, _, _ in PATH_COST_FIELDS])
        check(self._lib.fiesta_hip_path_cost_dev(self._h, C.c_void_p(waypoints_dev_ptr), int(n_waypoints), C.c_void_p(offsets_dev_ptr),
                                                 int(n_paths), float(step), float(margin), C.byref(res)))

    def BodyQuery(self, spheres, poses, margin) -> dict:
        """fiesta_hip_body_query: a body of spheres ((K, 4): body-frame centre and radius) at a batch of poses ((N, 7): px, py, pz, qw,
        qx, qy, qz; the quaternion need not be normalised).  Per pose the minimum of d - r over the spheres (d: GetDistWithGradTrilinear
        at the sphere's world centre), the sphere that attains it, its position and gradient, the number of spheres below `margin`,
        the penalty sum (margin - (d - r))^2 and its derivative with respect to the position and to a small world-frame rotation,
        and every sphere's clearance -- a dict of numpy arrays named as the fields of fiesta_hip_body_result;
        fiesta_amd.body_query_model is the definition"""
        sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        n, k = len(P), len(sph)
        out = {name: np.empty((n,) + tuple(k if d == "K" else d for d in shape), dtype) for name, dtype, shape in BODY_FIELDS}
        res = BodyResult(*[out[name].ctypes.data for name, _, _ in BODY_FIELDS])
        check(self._lib.fiesta_hip_body_query(self._h, _p(sph), k, _p(P), n, float(margin), C.byref(res)))
        return out

    def BodyQueryDevice(self, spheres, poses_dev_ptr: int, n_poses: int, margin, out=None):
        """fiesta_hip_body_query_dev: `spheres` is a host array as in BodyQuery, the poses (n_poses x 7 f64) and the outputs are
        resident on the device (`out` maps field names of fiesta_hip_body_result to device pointers, missing fields are not
        written); only enqueued on the map's stream"""
        sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
        out = out or {}
        res = BodyResult(*[int(out.get(name, 0)) or None for name, _, _ in BODY_FIELDS])
        check(self._lib.fiesta_hip_body_query_dev(self._h, _p(sph), len(sph), C.c_void_p(poses_dev_ptr), int(n_poses), float(margin),
                                                  C.byref(res)))

    def ArticulatedQuery(self, spheres, sphere_frame, frame_poses, margin) -> dict:
        """fiesta_hip_articulated_query: spheres on frames ((K, 4): centre in the frame of its own link and radius; sphere_frame (K,):
        the sphere's frame, non-decreasing) at a batch of configurations, one pose per frame (frame_poses (N, F, 7): px, py, pz, qw,
        qx, qy, qz; F is read from its shape).  Per configuration BodyQuery's minimum, sphere, position, gradient, count and cost over
        all spheres; per configuration and frame the minimum clearance, the cost and its derivative with respect to that frame's
        position and to a small world-frame rotation about its origin; and every sphere's clearance -- a dict of numpy arrays named
        as the fields of fiesta_hip_articulated_result; fiesta_amd.articulated_query_model is the definition"""
        sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
        frm = np.ascontiguousarray(sphere_frame, dtype=np.int32).reshape(-1)
        P = np.ascontiguousarray(frame_poses, dtype=np.float64)
        if P.ndim != 3 or P.shape[2] != 7 or len(frm) != len(sph):
            raise ValueError("ArticulatedQuery: frame_poses must be (N, F, 7) and sphere_frame hold one index per sphere")
        n, f, k = P.shape[0], P.shape[1], len(sph)
        dims = {"K": k, "F": f}
        out = {name: np.empty((n,) + tuple(dims.get(d, d) for d in shape), dtype) for name, dtype, shape in ARTICULATED_FIELDS}
        res = ArticulatedResult(*[out[name].ctypes.data for name, _, _ in ARTICULATED_FIELDS])
        check(self._lib.fiesta_hip_articulated_query(self._h, _p(sph), _p(frm), k, f, _p(P), n, float(margin), C.byref(res)))
        return out

    def ArticulatedQueryDevice(self, spheres, sphere_frame, n_frames: int, frame_poses_dev_ptr: int, n_configs: int, margin, out=None):
        """fiesta_hip_articulated_query_dev: `spheres` and `sphere_frame` are host arrays as in ArticulatedQuery, the frame poses
        (n_configs x n_frames x 7 f64) and the outputs are resident on the device (`out` maps field names of
        fiesta_hip_articulated_result to device pointers, missing fields are not written); only enqueued on the map's stream"""
        sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
        frm = np.ascontiguousarray(sphere_frame, dtype=np.int32).reshape(-1)
        if len(frm) != len(sph):
            raise ValueError("ArticulatedQueryDevice: sphere_frame must hold one index per sphere")
        out = out or {}
        res = ArticulatedResult(*[int(out.get(name, 0)) or None for name, _, _ in ARTICULATED_FIELDS])
        check(self._lib.fiesta_hip_articulated_query_dev(self._h, _p(sph), _p(frm), len(sph), int(n_frames), C.c_void_p(frame_poses_dev_ptr),
                                                         int(n_configs), float(margin), C.byref(res)))

    def BodySweep(self, spheres, poses, offsets, step, margin) -> dict:
        """fiesta_hip_body_sweep: a body of spheres ((K, 4): body-frame centre and radius) moved along polylines of waypoint poses
        ((N, 7): px, py, pz, qw, qx, qy, qz; CSR `offsets` over the pose rows).  The poses between two waypoints are sampled by the
        header's rule (at most `step` metres of travel of any sphere centre per sample for turns up to 90 degrees), each is evaluated
        as BodyQuery evaluates a pose; per path the minimum clearance with its sample, sphere, pose, position and gradient, the
        first sample with a sphere below `margin`, the count of such samples and the sample count -- a dict of numpy arrays named as
        the fields of fiesta_hip_sweep_result; fiesta_amd.body_sweep_model is the definition"""
        sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        n = len(off) - 1
        out = {name: np.empty((max(n, 0),) + shape, dtype) for name, dtype, shape in SWEEP_FIELDS}
        res = SweepResult(*[out[name].ctypes.data for name, _, _ in SWEEP_FIELDS])
        check(self._lib.fiesta_hip_body_sweep(self._h, _p(sph), len(sph), _p(P), len(P), _p(off), n, float(step), float(margin), C.byref(res)))
        return out

    def BodySweepDevice(self, spheres, poses_dev_ptr: int, n_poses: int, offsets_dev_ptr: int, n_paths: int, step, margin, out=None):
        """fiesta_hip_body_sweep_dev: `spheres` is a host array as in BodySweep, the waypoint poses (n_poses x 7 f64), the offsets
        (n_paths + 1 int64) and the outputs are resident on the device (`out` maps field names of fiesta_hip_sweep_result to device
        pointers, missing fields are not written); only enqueued on the map's stream"""
        sph = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
        out = out or {}
        res = SweepResult(*[int(out.get(name, 0)) or None for name, _, _ in SWEEP_FIELDS])
        check(self._lib.fiesta_hip_body_sweep_dev(self._h, _p(sph), len(sph), C.c_void_p(poses_dev_ptr), int(n_poses),
                                                  C.c_void_p(offsets_dev_ptr), int(n_paths), float(step), float(margin), C.byref(res)))

    def PathRefine(self, waypoints, offsets, bounds=None, *, margin, w_obstacle, w_smooth, alpha, max_step, tolerance=0.0,
                   iterations) -> dict:
        """fiesta_hip_path_refine: every path of the batch (CSR `offsets` over `waypoints`) takes `iterations` projected-gradient
        steps of size `alpha` (at most `max_step` per component) on w_obstacle * sum (margin - d)^2 + w_smooth * sum |second
        difference|^2 over its interior waypoints, each clamped to its row of `bounds` ((N, 6): lo xyz, hi xyz; None: free;
        fiesta_amd.corridor_bounds makes them from a corridor); the ends never move; a path stops once an iteration moved it by at
        most `tolerance`.  Returns a dict of numpy arrays named as the fields of fiesta_hip_refine_result (waypoints: one row per
        waypoint; cost: J before, J after); fiesta_amd.path_refine_model is the definition"""
        w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1:
            raise ValueError("offsets needs n_paths + 1 entries")
        b = None
        if bounds is not None:
            b = np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1, 6)
            if len(b) != len(w):
                raise ValueError("bounds needs one row of lo xyz, hi xyz per waypoint")
        n = len(off) - 1
        out = {name: np.empty((n if per == "path" else len(w),) + shape, dtype) for name, dtype, per, shape in REFINE_FIELDS}
        par = RefineParams(float(margin), float(w_obstacle), float(w_smooth), float(alpha), float(max_step), float(tolerance), int(iterations), 0)
        res = RefineResult(*[out[name].ctypes.data for name, _, _, _ in REFINE_FIELDS])
        check(self._lib.fiesta_hip_path_refine(self._h, _p(w), len(w), _p(off), n, _p(b), C.byref(par), C.byref(res)))
        return out

    def PathRefineDevice(self, waypoints_dev_ptr: int, n_waypoints: int, offsets_dev_ptr: int, n_paths: int, bounds_dev_ptr: int = 0, *,
                         margin, w_obstacle, w_smooth, alpha, max_step, tolerance=0.0, iterations, out=None):
        """fiesta_hip_path_refine_dev: inputs and outputs resident on the device (bounds 0: every waypoint free; `out` maps field
        names of fiesta_hip_refine_result to device pointers, missing fields are not written; out["waypoints"] may be the input
        pointer: in place); only enqueued on the map's stream"""
        out = out or {}
        par = RefineParams(float(margin), float(w_obstacle), float(w_smooth), float(alpha), float(max_step), float(tolerance), int(iterations), 0)
        res = RefineResult(*[int(out.get(name, 0)) or None for name, _, _, _ in REFINE_FIELDS])
        check(self._lib.fiesta_hip_path_refine_dev(self._h, C.c_void_p(waypoints_dev_ptr), int(n_waypoints), C.c_void_p(offsets_dev_ptr),
                                                   int(n_paths), C.c_void_p(bounds_dev_ptr or None), C.byref(par), C.byref(res)))

    def PathTiming(self, waypoints, offsets, *, step, margin, v_max, v_min, a_max, corner_dev, v_start=0.0, v_end=0.0) -> dict:
        """fiesta_hip_path_timing: per path (CSR `offsets` over `waypoints`) the travel time of the fastest speed profile that
        stays below the clearance limit 2 a_max (d - margin) of every sample (path_samples; v_min below the margin), the
        junction-deviation limit at every bend (corner_dev metres; inf: none), v_start / v_end at the ends and the acceleration
        bound a_max.  Returns a dict of numpy arrays named as the fields of fiesta_hip_path_timing_result (time, speed: one row per
        waypoint); fiesta_amd.path_timing_model is the definition"""
        w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1:
            raise ValueError("offsets needs n_paths + 1 entries")
        n = len(off) - 1
        out = {name: np.empty((n if per == "path" else len(w),) + shape, dtype) for name, dtype, per, shape in TIMING_FIELDS}
        par = TimingParams(float(step), float(margin), float(v_max), float(v_min), float(a_max), float(corner_dev), float(v_start), float(v_end))
        res = TimingResult(*[out[name].ctypes.data for name, _, _, _ in TIMING_FIELDS])
        check(self._lib.fiesta_hip_path_timing(self._h, _p(w), len(w), _p(off), n, C.byref(par), C.byref(res)))
        return out

    def PathTimingDevice(self, waypoints_dev_ptr: int, n_waypoints: int, offsets_dev_ptr: int, n_paths: int, *, step, margin, v_max, v_min,
                         a_max, corner_dev, v_start=0.0, v_end=0.0, out=None):
        """fiesta_hip_path_timing_dev: inputs and outputs resident on the device (`out` maps field names of
        fiesta_hip_path_timing_result to device pointers, missing fields are not written); only enqueued on the map's stream"""
        out = out or {}
        par = TimingParams(float(step), float(margin), float(v_max), float(v_min), float(a_max), float(corner_dev), float(v_start), float(v_end))
        res = TimingResult(*[int(out.get(name, 0)) or None for name, _, _, _ in TIMING_FIELDS])
        check(self._lib.fiesta_hip_path_timing_dev(self._h, C.c_void_p(waypoints_dev_ptr), int(n_waypoints), C.c_void_p(offsets_dev_ptr),
                                                   int(n_paths), C.byref(par), C.byref(res)))

    @property
    def host_cache_fetches(self) -> int:
        """bricks of the field fetched for scalar host queries so far (fiesta_hip_host_cache_fetches)"""
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_host_cache_fetches(self._h, C.byref(n)))
        return int(n.value)

    # -- whole field -----------------------------------------------------------------------------------------
    def download_field(self, want=("d2", "coc", "occ", "logodds")):
        n = self.grid_total_size_
        d2 = np.empty(n, np.int32) if "d2" in want else None
        coc = np.empty((n, 3), np.int32) if "coc" in want else None
        occ = np.empty(n, np.uint8) if "occ" in want else None
        lo = np.empty(n, np.float64) if "logodds" in want else None
        check(self._lib.fiesta_hip_download_field(self._h, _p(d2), _p(coc), _p(occ), _p(lo)))
        return {"d2": d2, "coc": coc, "occ": occ, "logodds": lo}

    def GetOccupiedVoxels(self) -> np.ndarray:
        """Voxel coordinates of all occupied voxels (the content of ESDFMap::GetPointCloud, src/ESDFMap.cpp:544-582)."""
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_get_occupied_voxels(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), np.int32)
        if n.value:
            check(self._lib.fiesta_hip_get_occupied_voxels(self._h, _p(out), n.value, C.byref(n)))
        return out

    def GetFrontierVoxels(self, lo=None, hi=None, min_clearance=0.0, want_mask=True):
        """fiesta_hip_get_frontier_voxels: the observed-free voxels with a never-observed 6-neighbour inside the inclusive map-voxel
        box [lo, hi] (both None: the whole map), optionally only those with GetDistance >= min_clearance -- (vox (n, 3) int32,
        mask (n,) uint8: the unknown-neighbour bits, or None without want_mask), unordered; frontier_model is the definition"""
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_get_frontier_voxels(self._h, _p(blo), _p(bhi), float(min_clearance), None, None, 0, C.byref(n)))
        vox = np.empty((n.value, 3), np.int32)
        mask = np.empty(n.value, np.uint8) if want_mask else None
        if n.value:
            check(self._lib.fiesta_hip_get_frontier_voxels(self._h, _p(blo), _p(bhi), float(min_clearance), _p(vox), _p(mask), n.value,
                                                           C.byref(n)))
        return vox, mask

    def GetFrontierVoxelsDevice(self, lo, hi, min_clearance, vox_dev_ptr: int, mask_dev_ptr: int, capacity: int, n_out_dev_ptr: int):
        """fiesta_hip_get_frontier_voxels_dev: the outputs and the 64-bit counter resident on the device (0: that array is not
        written), lo / hi host triples or None; only enqueued on the map's stream, the call zeroes the counter itself"""
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        check(self._lib.fiesta_hip_get_frontier_voxels_dev(self._h, _p(blo), _p(bhi), float(min_clearance), C.c_void_p(vox_dev_ptr or None),
                                                           C.c_void_p(mask_dev_ptr or None), int(capacity),
                                                           C.c_void_p(n_out_dev_ptr or None)))

    SKELETON_FIELDS = (("vox", np.int32, (3,)), ("mask", np.uint8, ()), ("d2", np.int32, ()), ("sep2", np.int32, ()))

    def GetSkeletonVoxels(self, lo=None, hi=None, min_sep2=9, min_clearance=0.0, want=("vox", "mask", "d2", "sep2")) -> dict:
        """fiesta_hip_get_skeleton_voxels: the free voxels on the distance field's ridge -- a 6-neighbour names a closest obstacle at
        least sqrt(min_sep2) voxels from the voxel's own and the bisector of the two passes between them -- inside the inclusive
        map-voxel box [lo, hi] (both None: the whole map), optionally only those with GetDistance >= min_clearance.  A dict of the
        arrays named in `want` (vox (n, 3) int32, mask (n,) uint8: the ridge-neighbour bits, d2 (n,) int32, sep2 (n,) int32: the
        largest separation over the mask's bits) and "n", unordered; skeleton_model is the definition"""
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        unknown = set(want) - {f[0] for f in self.SKELETON_FIELDS}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        n = C.c_int64(0)
        res = _lib.SkeletonResult(None, None, None, None)
        check(self._lib.fiesta_hip_get_skeleton_voxels(self._h, _p(blo), _p(bhi), int(min_sep2), float(min_clearance), 0, C.byref(res),
                                                       C.byref(n)))
        out = {name: np.empty((n.value,) + shape, dt) for name, dt, shape in self.SKELETON_FIELDS if name in want}
        if n.value and out:
            res = _lib.SkeletonResult(*[out[name].ctypes.data if name in out else None for name, _, _ in self.SKELETON_FIELDS])
            total = C.c_int64(0)
            check(self._lib.fiesta_hip_get_skeleton_voxels(self._h, _p(blo), _p(bhi), int(min_sep2), float(min_clearance), n.value,
                                                           C.byref(res), C.byref(total)))
        out["n"] = int(n.value)
        return out

    def GetSkeletonVoxelsDevice(self, lo, hi, min_sep2, min_clearance, capacity: int, n_out_dev_ptr: int, vox_dev_ptr: int = 0,
                                mask_dev_ptr: int = 0, d2_dev_ptr: int = 0, sep2_dev_ptr: int = 0):
        """fiesta_hip_get_skeleton_voxels_dev: the outputs and the 64-bit counter resident on the device (0: that array is not
        written), lo / hi host triples or None; only enqueued on the map's stream, the call zeroes the counter itself"""
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        res = _lib.SkeletonResult(vox_dev_ptr or None, mask_dev_ptr or None, d2_dev_ptr or None, sep2_dev_ptr or None)
        check(self._lib.fiesta_hip_get_skeleton_voxels_dev(self._h, _p(blo), _p(bhi), int(min_sep2), float(min_clearance), int(capacity),
                                                           C.byref(res), C.c_void_p(n_out_dev_ptr or None)))

    def RayQuery(self, start, end, stop_mask=7) -> dict:
        """fiesta_hip_ray_query: per segment start -> end (metres, (n, 3) or one triple) the first voxel of its walk whose class is in
        `stop_mask` (RAY_OCCUPIED | RAY_UNKNOWN | RAY_OUTSIDE), its index, class, map voxel and distance, the number of voxels visited
        and the counts of free / occupied / unknown / outside voxels before it -- a dict of numpy arrays named as the fields of
        fiesta_hip_ray_result; ray_query_model is the definition.  One launch per call: batch the rays."""
        s = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 3)
        if len(s) != len(t):
            raise ValueError("start and end need the same number of rows")
        n = len(s)
        out = {name: np.empty((n,) + shape, dtype) for name, dtype, shape in RAY_FIELDS}
        res = RayResult(*[out[name].ctypes.data for name, _, _ in RAY_FIELDS])
        check(self._lib.fiesta_hip_ray_query(self._h, _p(s), _p(t), n, int(stop_mask), C.byref(res)))
        return out

    def RayQueryDevice(self, start_dev_ptr: int, end_dev_ptr: int, n: int, stop_mask=7, out=None):
        """fiesta_hip_ray_query_dev: inputs and outputs resident on the device (n x 3 f64 each; `out` maps field names of
        fiesta_hip_ray_result to device pointers, missing fields are not written); only enqueued on the map's stream"""
        out = out or {}
        res = RayResult(*[int(out.get(name, 0)) or None for name, _, _ in RAY_FIELDS])
        check(self._lib.fiesta_hip_ray_query_dev(self._h, C.c_void_p(start_dev_ptr), C.c_void_p(end_dev_ptr), int(n), int(stop_mask),
                                                 C.byref(res)))

    @staticmethod
    def _reach_info(info) -> dict:
        d = {k: getattr(info, k) for k, _ in ReachInfo._fields_}
        d["box_lo"], d["box_hi"] = list(info.box_lo), list(info.box_hi)
        return d

    def ReachField(self, seeds, lo=None, hi=None, targets=None, min_clearance=0.0, connectivity=26, flags=0, want_cost=True) -> dict:
        """fiesta_hip_reach_field: the cost-to-go field of the inclusive map-voxel box [lo, hi] (both None: a dense map's whole array)
        flooded from `seeds` ((n, 3) map voxels) through the traversable voxels -- observed free, with GetDistance >= min_clearance if
        that is > 0, and with flags = REACH_THROUGH_UNKNOWN the never-observed ones too -- by moves of weight 3 / 4 / 5 (connectivity 6:
        only 3).  Returns the fields of fiesta_hip_reach_info plus cost ((ex, ey, ez) int32 over the clipped box: -1 not traversable,
        2^31 - 1 not reached; None without want_cost) and, with `targets`, target_cost ((n,) int32; -1 outside the box);
        fiesta_amd.reach_model is the definition"""
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        s = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
        t = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32).reshape(-1, 3)
        nt = 0 if t is None else len(t)
        tc = None if t is None else np.empty(nt, np.int32)
        info = ReachInfo()
        args = (_p(blo), _p(bhi), _p(s) if len(s) else None, len(s), _p(t) if nt else None, nt, float(min_clearance), int(connectivity),
                int(flags))
        cost = None
        if want_cost:
            cost = np.empty(self._reach_extents(blo, bhi), np.int32)   # (the clipped box decides the size of the field)
        res = ReachResult(cost.ctypes.data if cost is not None and cost.size else None, tc.ctypes.data if nt else None)
        check(self._lib.fiesta_hip_reach_field(self._h, *args, C.byref(res), C.byref(info)))
        out = self._reach_info(info)
        out["cost"] = cost
        if t is not None:
            out["target_cost"] = tc
        return out

    def _reach_extents(self, blo, bhi):
        """extents of the box a reach call clips [blo, bhi] to (host arithmetic, the library's rule)"""
        if self.mode != "array":
            if blo is None:
                raise ValueError("a hash-block map has no outside: the box is mandatory")
            a, b = np.clip(blo.astype(np.int64), -2 ** 30, 2 ** 30), np.clip(bhi.astype(np.int64), -2 ** 30, 2 ** 30)
        else:
            org = self._array_origin()
            dims = np.array(self.grid_size, np.int64)
            a = np.zeros(3, np.int64) if blo is None else np.maximum(blo.astype(np.int64) - org, 0)
            b = dims - 1 if bhi is None else np.minimum(bhi.astype(np.int64) - org, dims - 1)
        if np.any(a > b):
            return (0, 0, 0)
        return tuple(int(v) for v in b - a + 1)

    def _array_origin(self):
        """map voxel of element (0, 0, 0) of an array-mode map's array (non-zero on a shard)"""
        info = _lib.ShardInfo()
        check(self._lib.fiesta_hip_shard_info_get(self._h, C.byref(info)))
        return np.array(list(info.local_origin), np.int64)

    def ReachFieldDevice(self, seeds_dev_ptr: int, n_seeds: int, lo=None, hi=None, targets_dev_ptr: int = 0, n_targets: int = 0,
                         min_clearance=0.0, connectivity=26, flags=0, cost_dev_ptr: int = 0, target_cost_dev_ptr: int = 0) -> dict:
        """fiesta_hip_reach_field_dev: seeds, targets, cost and target_cost resident on the device (0: not given / not written; the
        cost field needs ex * ey * ez int32 of the clipped box); returns the fields of fiesta_hip_reach_info.  Synchronises with the
        map's stream, unlike the other device calls"""
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        info = ReachInfo()
        res = ReachResult(int(cost_dev_ptr) or None, int(target_cost_dev_ptr) or None)
        check(self._lib.fiesta_hip_reach_field_dev(self._h, _p(blo), _p(bhi), C.c_void_p(seeds_dev_ptr or None), int(n_seeds),
                                                   C.c_void_p(targets_dev_ptr or None), int(n_targets), float(min_clearance),
                                                   int(connectivity), int(flags), C.byref(res), C.byref(info)))
        return self._reach_info(info)

    @staticmethod
    def _reach_matrix_info(info) -> dict:
        d = {k: getattr(info, k) for k, _ in ReachMatrixInfo._fields_}
        d["box_lo"], d["box_hi"] = list(info.box_lo), list(info.box_hi)
        return d

    def ReachMatrix(self, sources, targets=None, lo=None, hi=None, min_clearance=0.0, connectivity=26, flags=0, max_fields=0) -> dict:
        """fiesta_hip_reach_matrix: the travel cost from every source ((n, 3) map voxels, each a flood of its own) to every column --
        `targets` ((m, 3) map voxels), or the sources themselves (None: the square form) -- through the traversable voxels of the box
        [lo, hi], with ReachField's box, clearance, flags and connectivity; the floods share one traversability bitmap and run side by
        side, at most max_fields at a time (0: as many as 2^28 cost entries allow).  Returns the fields of fiesta_hip_reach_matrix_info
        plus cost ((n, n_cols) int32: row s is ReachField([source s], targets=columns)["target_cost"], or all -1 for a source that is
        not REACH_SITE_OK), source_status ((n,) int32) and source_reached ((n,) int64); fiesta_amd.reach_matrix_model is the definition"""
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        s = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1, 3)
        t = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32).reshape(-1, 3)
        n, nt = len(s), 0 if t is None else len(t)
        cost = np.empty((n, n if t is None else nt), np.int32)
        status, reached = np.empty(n, np.int32), np.empty(n, np.int64)
        info = ReachMatrixInfo()
        res = ReachMatrixResult(cost.ctypes.data if cost.size else None, status.ctypes.data if n else None, reached.ctypes.data if n else None)
        # (an empty `targets` is a matrix without columns, not the square form: the pointer stays non-null)
        tp = None if t is None else _p(t if nt else np.zeros(3, np.int32))
        check(self._lib.fiesta_hip_reach_matrix(self._h, _p(blo), _p(bhi), _p(s) if n else None, n, tp, nt, float(min_clearance), int(connectivity),
                                                int(flags), int(max_fields), C.byref(res), C.byref(info)))
        out = self._reach_matrix_info(info)
        out.update(cost=cost, source_status=status, source_reached=reached)
        return out

    def ReachMatrixDevice(self, sources_dev_ptr: int, n_sources: int, targets_dev_ptr: int = 0, n_targets: int = 0, lo=None, hi=None,
                          min_clearance=0.0, connectivity=26, flags=0, max_fields=0, cost_dev_ptr: int = 0, source_status_dev_ptr: int = 0,
                          source_reached_dev_ptr: int = 0) -> dict:
        """fiesta_hip_reach_matrix_dev: sources, targets (0 with n_targets = 0: the square form), cost (n_sources x n_cols int32),
        source_status (int32) and source_reached (int64) resident on the device (0: not given / not written); returns the fields of
        fiesta_hip_reach_matrix_info.  Synchronises with the map's stream, like ReachFieldDevice"""
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        info = ReachMatrixInfo()
        res = ReachMatrixResult(int(cost_dev_ptr) or None, int(source_status_dev_ptr) or None, int(source_reached_dev_ptr) or None)
        check(self._lib.fiesta_hip_reach_matrix_dev(self._h, _p(blo), _p(bhi), C.c_void_p(sources_dev_ptr or None), int(n_sources),
                                                    C.c_void_p(targets_dev_ptr or None), int(n_targets), float(min_clearance),
                                                    int(connectivity), int(flags), int(max_fields), C.byref(res), C.byref(info)))
        return self._reach_matrix_info(info)

    def SiteTour(self, cost, start=0, closed=False, restarts=64, seed=0, max_moves=0) -> dict:
        """fiesta_hip_site_tour: the order in which to visit every site the start can reach through the symmetric cost matrix `cost`
        ((n, ld) int32 with ld >= n: ReachMatrix's square form; -1 and 2^31 - 1 are no connections), as an open path from `start` or
        a closed tour back to it, minimising the summed leg cost: `restarts` local searches (2-opt and Or-opt, best improvement) run
        side by side, restart 0 from the nearest-neighbour tour and the others from shuffles seeded by `seed`, each applying at most
        max_moves moves (0: 8 per visited site).  Returns order, site_status, leg_cost ((n,) int32), restart_length ((restarts,)
        int64) and the fields of fiesta_hip_tour_info; fiesta_amd.tour_model is the definition"""
        c = np.ascontiguousarray(cost, dtype=np.int32)
        if c.ndim != 2:
            raise ValueError("cost must be a matrix")
        n, ld = c.shape
        out = {"order": np.empty(n, np.int32), "site_status": np.empty(n, np.int32), "leg_cost": np.empty(n, np.int32),
               "restart_length": np.empty(max(int(restarts), 0), np.int64)}
        res = TourResult(*[a.ctypes.data if a.size else None for a in out.values()])
        info = TourInfo()
        check(self._lib.fiesta_hip_site_tour(self._h, _p(c) if c.size else None, n, ld, int(start), 1 if closed else 0, int(restarts),
                                             int(seed) & (2 ** 64 - 1), int(max_moves), C.byref(res), C.byref(info)))
        out.update({k: getattr(info, k) for k, _ in TourInfo._fields_})
        return out

    def SiteTourDevice(self, cost_dev_ptr: int, n: int, ld: int, start=0, closed=False, restarts=64, seed=0, max_moves=0, order_dev_ptr: int = 0,
                       site_status_dev_ptr: int = 0, leg_cost_dev_ptr: int = 0, restart_length_dev_ptr: int = 0) -> dict:
        """fiesta_hip_site_tour_dev: the matrix (n x n int32, leading dimension ld: where ReachMatrixDevice left it), order,
        site_status, leg_cost (n int32 each) and restart_length (restarts int64) resident on the device (0: not written); returns
        the fields of fiesta_hip_tour_info.  Synchronises with the map's stream"""
        res = TourResult(int(order_dev_ptr) or None, int(site_status_dev_ptr) or None, int(leg_cost_dev_ptr) or None,
                         int(restart_length_dev_ptr) or None)
        info = TourInfo()
        check(self._lib.fiesta_hip_site_tour_dev(self._h, C.c_void_p(cost_dev_ptr or None), int(n), int(ld), int(start), 1 if closed else 0,
                                                 int(restarts), int(seed) & (2 ** 64 - 1), int(max_moves), C.byref(res), C.byref(info)))
        return {k: getattr(info, k) for k, _ in TourInfo._fields_}

    def ReachPaths(self, targets, cost=None, box=None, connectivity=26, shortcut=False, max_span=4096, want_pos=True) -> dict:
        """fiesta_hip_reach_paths: per target ((n, 3) map voxels) the path down a cost-to-go field from the seed it was reached from to
        the target.  The field: the one the map retained from its last ReachField call (cost and box None), or `cost` ((ex, ey, ez)
        int32) with box = (box_lo, box_hi), the inclusive map-voxel box ReachField reported, and the connectivity it was flooded with.
        shortcut: pull the staircase tight by line of sight through the field's traversable voxels, at most max_span moves per
        segment.  Returns offsets ((n + 1,) int64 CSR), waypoints_vox ((N, 3) int32), waypoints_pos ((N, 3) f64 metres, the input of
        PathClearance / PathCost; None without want_pos), status ((n,) int32, REACH_PATH_*) and n_moves ((n,) int32);
        fiesta_amd.reach_paths_model is the definition"""
        if (cost is None) != (box is None):
            raise ValueError("cost and box must both be given or both be None")
        t = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1, 3)
        n = len(t)
        c = blo = bhi = None
        if cost is not None:
            blo = np.ascontiguousarray(box[0], np.int32).reshape(3)
            bhi = np.ascontiguousarray(box[1], np.int32).reshape(3)
            c = np.ascontiguousarray(cost, dtype=np.int32)
            if c.size != int(np.prod(np.maximum(bhi.astype(np.int64) - blo + 1, 0))):
                raise ValueError("cost does not have the box's number of voxels")
        flags = 1 if shortcut else 0
        out = {"offsets": np.zeros(n + 1, np.int64), "status": np.empty(n, np.int32), "n_moves": np.empty(n, np.int32)}
        res = ReachPathsResult(out["offsets"].ctypes.data, None, None, out["status"].ctypes.data, out["n_moves"].ctypes.data)
        tp = _p(t) if n else None
        check(self._lib.fiesta_hip_reach_paths(self._h, _p(c), _p(blo), _p(bhi), tp, n, int(connectivity), flags, int(max_span), 0, C.byref(res)))
        total = int(out["offsets"][n])
        out["waypoints_vox"] = np.empty((total, 3), np.int32)
        out["waypoints_pos"] = np.empty((total, 3), np.float64) if want_pos else None
        if total:
            # (an explicit field was uploaded by the sizing call: the map retains it)
            res = ReachPathsResult(out["offsets"].ctypes.data, out["waypoints_vox"].ctypes.data,
                                   out["waypoints_pos"].ctypes.data if want_pos else None, None, None)
            check(self._lib.fiesta_hip_reach_paths(self._h, None, None, None, tp, n, int(connectivity), flags, int(max_span), total, C.byref(res)))
        return out

    def ReachPathsDevice(self, targets_dev_ptr: int, n_targets: int, offsets_dev_ptr: int, cost_dev_ptr: int = 0, box=None, connectivity=26,
                         shortcut=False, max_span=4096, capacity: int = 0, waypoints_vox_dev_ptr: int = 0, waypoints_pos_dev_ptr: int = 0,
                         status_dev_ptr: int = 0, n_moves_dev_ptr: int = 0):
        """fiesta_hip_reach_paths_dev: targets, the cost field (0: the retained one; else with box = (box_lo, box_hi), host triples) and
        the outputs resident on the device (offsets: n_targets + 1 int64, required; 0: that array is not written); only enqueued on
        the map's stream.  offsets holds the true totals whatever `capacity` is: enqueue with capacity 0 to size the buffers"""
        blo = None if box is None else np.ascontiguousarray(box[0], np.int32).reshape(3)
        bhi = None if box is None else np.ascontiguousarray(box[1], np.int32).reshape(3)
        res = ReachPathsResult(int(offsets_dev_ptr) or None, int(waypoints_vox_dev_ptr) or None, int(waypoints_pos_dev_ptr) or None,
                               int(status_dev_ptr) or None, int(n_moves_dev_ptr) or None)
        check(self._lib.fiesta_hip_reach_paths_dev(self._h, C.c_void_p(cost_dev_ptr or None), _p(blo), _p(bhi), C.c_void_p(targets_dev_ptr or None),
                                                   int(n_targets), int(connectivity), 1 if shortcut else 0, int(max_span), int(capacity),
                                                   C.byref(res)))

    @staticmethod
    def _leg_info(info) -> dict:
        return {"box_lo": list(info.box_lo), "box_hi": list(info.box_hi), "connectivity": int(info.connectivity), "n_sources": int(info.n_sources)}

    def LegPaths(self, from_, to=None, to_vox=None, shortcut=False, max_span=4096, want_pos=True) -> dict:
        """fiesta_hip_leg_paths: per leg the path from site from_[k] -- an index into the sources of the map's last ReachMatrix call,
        whose floods the map retains while they fitted one batch (its "batches" == 1) -- to site to[k], or to map voxel to_vox[k]
        (exactly one of the two), with nothing flooded again.  A tour's legs: from_ = order[:m - 1], to = order[1:m] of SiteTour.
        shortcut / max_span as in ReachPaths; the connectivity is the retained batch's.  Returns offsets ((n + 1,) int64 CSR),
        waypoints_vox ((N, 3) int32, each leg from its source to its target), waypoints_pos ((N, 3) f64 metres; None without
        want_pos), status ((n,) int32: REACH_PATH_*, LEG_NO_SOURCE, LEG_BAD_INDEX), n_moves, cost ((n,) int32: the matrix entry of
        the leg) and what is retained: box_lo, box_hi, connectivity, n_sources; fiesta_amd.leg_paths_model is the definition"""
        if (to is None) == (to_vox is None):
            raise ValueError("exactly one of to and to_vox must be given")
        f = np.ascontiguousarray(from_, dtype=np.int32).reshape(-1)
        n = len(f)
        t = None if to is None else np.ascontiguousarray(to, dtype=np.int32).reshape(-1)
        tv = None if to_vox is None else np.ascontiguousarray(to_vox, dtype=np.int32).reshape(-1, 3)
        if len(t if tv is None else tv) != n:
            raise ValueError("from_ and to / to_vox differ in length")
        # (an empty batch keeps the pointers non-null: which of to / to_vox is meant does not matter then)
        args = (_p(f) if n else None, _p(t) if n and t is not None else None, _p(tv) if n and tv is not None else None, n, 1 if shortcut else 0,
                int(max_span))
        out = {"offsets": np.zeros(n + 1, np.int64), "status": np.empty(n, np.int32), "n_moves": np.empty(n, np.int32), "cost": np.empty(n, np.int32)}
        ptr = lambda k: out[k].ctypes.data if n else None  # noqa: E731
        info = LegPathsInfo()
        res = LegPathsResult(out["offsets"].ctypes.data, None, None, ptr("status"), ptr("n_moves"), ptr("cost"))
        check(self._lib.fiesta_hip_leg_paths(self._h, *args, 0, C.byref(res), C.byref(info)))
        total = int(out["offsets"][n])
        out["waypoints_vox"] = np.empty((total, 3), np.int32)
        out["waypoints_pos"] = np.empty((total, 3), np.float64) if want_pos else None
        if total:
            res = LegPathsResult(out["offsets"].ctypes.data, out["waypoints_vox"].ctypes.data, out["waypoints_pos"].ctypes.data if want_pos else None,
                                 None, None, None)
            check(self._lib.fiesta_hip_leg_paths(self._h, *args, total, C.byref(res), None))
        out.update(self._leg_info(info))
        return out

    def LegPathsDevice(self, from_dev_ptr: int, n_legs: int, offsets_dev_ptr: int, to_dev_ptr: int = 0, to_vox_dev_ptr: int = 0, shortcut=False,
                       max_span=4096, capacity: int = 0, waypoints_vox_dev_ptr: int = 0, waypoints_pos_dev_ptr: int = 0, status_dev_ptr: int = 0,
                       n_moves_dev_ptr: int = 0, cost_dev_ptr: int = 0) -> dict:
        """fiesta_hip_leg_paths_dev: from, to (n_legs int32 each; they may be views into the order array where SiteTourDevice left
        it) or to_vox (n_legs x 3 int32) and the outputs resident on the device (offsets: n_legs + 1 int64, required; 0: that array
        is not written); only enqueued on the map's stream.  offsets holds the true totals whatever `capacity` is: enqueue with
        capacity 0 to size the buffers.  Returns what the map retains: box_lo, box_hi, connectivity, n_sources"""
        res = LegPathsResult(*[int(v) or None for v in (offsets_dev_ptr, waypoints_vox_dev_ptr, waypoints_pos_dev_ptr, status_dev_ptr,
                                                        n_moves_dev_ptr, cost_dev_ptr)])
        info = LegPathsInfo()
        check(self._lib.fiesta_hip_leg_paths_dev(self._h, C.c_void_p(from_dev_ptr or None), C.c_void_p(to_dev_ptr or None),
                                                 C.c_void_p(to_vox_dev_ptr or None), int(n_legs), 1 if shortcut else 0, int(max_span), int(capacity),
                                                 C.byref(res), C.byref(info)))
        return self._leg_info(info)

    def TourRoute(self, sites, start=0, closed=False, lo=None, hi=None, min_clearance=0.0, connectivity=26, flags=0, restarts=64, seed=0,
                  max_moves=0, shortcut=False, max_span=4096, want_pos=True) -> dict:
        """ReachMatrix -> SiteTour -> LegPaths: the order in which to visit `sites` ((n, 3) map voxels) from sites[start] and the way
        along every leg, the box flooded once per site and never again.  The matrix arguments are ReachMatrix's (all sites must fit
        one batch: else ValueError), the tour's SiteTour's, the paths' LegPaths'.  Leg k runs from order[k] to order[k + 1]; a
        closed tour gets the wrap-around leg order[m - 1] -> order[0] as its last.  Returns SiteTour's dict plus matrix (the cost
        matrix), source_status and legs: LegPaths' dict with its `from` and `to`"""
        mx = self.ReachMatrix(sites, lo=lo, hi=hi, min_clearance=min_clearance, connectivity=connectivity, flags=flags)
        if mx["batches"] != 1:
            raise ValueError("the sites' floods do not fit one batch (or the box is empty): no legs can be extracted")
        out = self.SiteTour(mx["cost"], start=start, closed=closed, restarts=restarts, seed=seed, max_moves=max_moves)
        m = int(out["n_visited"])
        order = out["order"][:m]
        fr, to = order[:-1], order[1:]
        if closed and m >= 2:
            fr, to = order, np.concatenate([order[1:], order[:1]])
        legs = self.LegPaths(fr, to=to, shortcut=shortcut, max_span=max_span, want_pos=want_pos)
        legs["from"], legs["to"] = np.array(fr, np.int32), np.array(to, np.int32)
        out.update(matrix=mx["cost"], source_status=mx["source_status"], legs=legs)
        return out

    @staticmethod
    def _window(lo, hi):
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        blo = None if lo is None else np.ascontiguousarray(lo, np.int32).reshape(3)
        bhi = None if hi is None else np.ascontiguousarray(hi, np.int32).reshape(3)
        return blo, bhi

    def FreeBoxes(self, seeds, lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0) -> dict:
        """fiesta_hip_free_boxes: around every seed ((n, 3) map voxels) the axis-aligned box of traversable voxels -- ReachField's
        traversability, with CORRIDOR_THROUGH_UNKNOWN in `flags` the never-observed voxels too -- grown face by face (-x, +x, -y, +y,
        -z, +z in turn, at most max_grow <= 256 steps each) inside the inclusive map-voxel window [lo, hi] (both None: a dense map's
        whole array, everything on a hash-block map).  Returns box ((n, 6) int32: lo xyz, hi xyz), box_pos ((n, 6) f64 metres: the
        box's two corners), stop ((n, 6) uint8, CORRIDOR_STOP_*), volume ((n,) int64) and status ((n,) int32, FREE_BOX_*);
        fiesta_amd.free_box_model is the definition"""
        blo, bhi = self._window(lo, hi)
        s = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
        n = len(s)
        out = {"box": np.empty((n, 6), np.int32), "box_pos": np.empty((n, 6), np.float64), "stop": np.empty((n, 6), np.uint8),
               "volume": np.empty(n, np.int64), "status": np.empty(n, np.int32)}
        res = FreeBoxesResult(*[a.ctypes.data if n else None for a in out.values()])
        check(self._lib.fiesta_hip_free_boxes(self._h, _p(blo), _p(bhi), _p(s) if n else None, n, float(min_clearance), int(max_grow), int(flags),
                                              C.byref(res)))
        return out

    def FreeBoxesDevice(self, seeds_dev_ptr: int, n: int, lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0, box_dev_ptr: int = 0,
                        box_pos_dev_ptr: int = 0, stop_dev_ptr: int = 0, volume_dev_ptr: int = 0, status_dev_ptr: int = 0):
        """fiesta_hip_free_boxes_dev: seeds and the outputs resident on the device (0: that array is not written); only enqueued on
        the map's stream"""
        blo, bhi = self._window(lo, hi)
        res = FreeBoxesResult(int(box_dev_ptr) or None, int(box_pos_dev_ptr) or None, int(stop_dev_ptr) or None, int(volume_dev_ptr) or None,
                              int(status_dev_ptr) or None)
        check(self._lib.fiesta_hip_free_boxes_dev(self._h, _p(blo), _p(bhi), C.c_void_p(seeds_dev_ptr or None), int(n), float(min_clearance),
                                                  int(max_grow), int(flags), C.byref(res)))

    def PathCorridor(self, waypoints_vox, offsets, lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0, want_pos=True) -> dict:
        """fiesta_hip_path_corridor: for every polyline of the CSR batch (`waypoints_vox` (n, 3) map voxels and `offsets`, as ReachPaths
        returns them) the safe flight corridor -- overlapping boxes inflated as by FreeBoxes along the path's voxel chain, a new box
        wherever the chain leaves the last one.  Returns offsets ((n_paths + 1,) int64 CSR over the boxes), boxes ((N, 6) int32),
        boxes_pos ((N, 6) f64 metres; None without want_pos), stop ((N, 6) uint8), entry ((N,) int32), status ((n_paths,) int32,
        CORRIDOR_*), n_chain, blocked_segment ((n_paths,) int32) and blocked_vox ((n_paths, 3) int32);
        fiesta_amd.corridor_model is the definition"""
        blo, bhi = self._window(lo, hi)
        w = np.ascontiguousarray(waypoints_vox, dtype=np.int32).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 1:
            raise ValueError("offsets must hold n_paths + 1 entries")
        n = len(off) - 1
        out = {"offsets": np.zeros(n + 1, np.int64), "status": np.empty(n, np.int32), "n_chain": np.empty(n, np.int32),
               "blocked_segment": np.empty(n, np.int32), "blocked_vox": np.empty((n, 3), np.int32)}
        args = (_p(blo), _p(bhi), _p(w) if len(w) else None, len(w), _p(off), n, float(min_clearance), int(max_grow), int(flags))
        ptr = lambda k: out[k].ctypes.data if out[k] is not None and out[k].size else None  # noqa: E731
        res = CorridorResult(out["offsets"].ctypes.data, None, None, None, None, ptr("status"), ptr("n_chain"), ptr("blocked_segment"), ptr("blocked_vox"))
        check(self._lib.fiesta_hip_path_corridor(self._h, *args, 0, C.byref(res)))
        total = int(out["offsets"][n])
        out.update(boxes=np.empty((total, 6), np.int32), boxes_pos=np.empty((total, 6), np.float64) if want_pos else None,
                   stop=np.empty((total, 6), np.uint8), entry=np.empty(total, np.int32))
        if total:
            res = CorridorResult(out["offsets"].ctypes.data, ptr("boxes"), ptr("boxes_pos"), ptr("stop"), ptr("entry"), None, None, None, None)
            check(self._lib.fiesta_hip_path_corridor(self._h, *args, total, C.byref(res)))
        return out

    def PathCorridorDevice(self, waypoints_vox_dev_ptr: int, n_waypoints: int, path_offsets_dev_ptr: int, n_paths: int, offsets_dev_ptr: int,
                           lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0, capacity: int = 0, boxes_dev_ptr: int = 0,
                           boxes_pos_dev_ptr: int = 0, stop_dev_ptr: int = 0, entry_dev_ptr: int = 0, status_dev_ptr: int = 0,
                           n_chain_dev_ptr: int = 0, blocked_segment_dev_ptr: int = 0, blocked_vox_dev_ptr: int = 0):
        """fiesta_hip_path_corridor_dev: the waypoints, their CSR offsets (where ReachPathsDevice left them) and the outputs resident
        on the device (offsets: n_paths + 1 int64, required; 0: that array is not written); only enqueued on the map's stream.
        offsets holds the true totals whatever `capacity` is: enqueue with capacity 0 to size the buffers"""
        blo, bhi = self._window(lo, hi)
        res = CorridorResult(*[int(v) or None for v in (offsets_dev_ptr, boxes_dev_ptr, boxes_pos_dev_ptr, stop_dev_ptr, entry_dev_ptr, status_dev_ptr,
                                                        n_chain_dev_ptr, blocked_segment_dev_ptr, blocked_vox_dev_ptr)])
        check(self._lib.fiesta_hip_path_corridor_dev(self._h, _p(blo), _p(bhi), C.c_void_p(waypoints_vox_dev_ptr or None), int(n_waypoints),
                                                     C.c_void_p(path_offsets_dev_ptr or None), int(n_paths), float(min_clearance), int(max_grow),
                                                     int(flags), int(capacity), C.byref(res)))

    def CorridorBounds(self, waypoints_vox, offsets, corridor, inset=None, void_broken=False) -> dict:
        """fiesta_hip_corridor_bounds: the `bounds` of PathRefine for the voxel polylines of a CSR batch and their corridor
        (`corridor`: what PathCorridor returned for the same waypoints_vox and offsets, with boxes_pos) -- each waypoint's corridor
        box, intersected with the next one where the path changes boxes, `inset` metres taken off every upper face.  inset=None is
        resolution * 2.0 ** -20 (fiesta_amd.corridor_bounds' own default reads the voxel size off the first box; its bits can differ:
        pass the same number to both to compare them).  With void_broken the rows of every path that is not ok are NaN, which
        PathRefine reports INVALID and leaves alone.  Returns bounds ((N, 6) f64: lo xyz, hi xyz), ok ((n_paths,) int32) and box ((N,)
        int64: the global index of the waypoint's box, -1: none); fiesta_amd.corridor_bounds_model is the definition"""
        w = np.ascontiguousarray(waypoints_vox, dtype=np.int32).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        boff = np.ascontiguousarray(corridor["offsets"], dtype=np.int64).reshape(-1)
        boxes = np.ascontiguousarray(corridor["boxes"], dtype=np.int32).reshape(-1, 6)
        pos = np.ascontiguousarray(corridor["boxes_pos"], dtype=np.float64).reshape(-1, 6)
        entry = np.ascontiguousarray(corridor["entry"], dtype=np.int32).reshape(-1)
        status = np.ascontiguousarray(corridor["status"], dtype=np.int32).reshape(-1)
        n = len(off) - 1
        if n < 0 or len(boff) != n + 1 or len(status) != n or not len(boxes) == len(pos) == len(entry):
            raise ValueError("offsets and corridor do not describe the same batch")
        inset = self.resolution * 2.0 ** -20 if inset is None else float(inset)
        out = {"bounds": np.empty((len(w), 6), np.float64), "ok": np.empty(n, np.int32), "box": np.empty(len(w), np.int64)}
        res = BoundsResult(*[a.ctypes.data if a.size else None for a in out.values()])
        ptr = lambda a: _p(a) if a.size else None  # noqa: E731
        check(self._lib.fiesta_hip_corridor_bounds(self._h, ptr(w), len(w), _p(off), n, _p(boff), ptr(boxes), ptr(pos), ptr(entry), ptr(status),
                                                   len(pos), inset, BOUNDS_VOID_BROKEN if void_broken else 0, C.byref(res)))
        return out

    def CorridorBoundsDevice(self, waypoints_vox_dev_ptr: int, n_waypoints: int, path_offsets_dev_ptr: int, n_paths: int, box_offsets_dev_ptr: int,
                             boxes_dev_ptr: int, boxes_pos_dev_ptr: int, entry_dev_ptr: int, status_dev_ptr: int, n_boxes: int, inset=None,
                             void_broken=False, bounds_dev_ptr: int = 0, ok_dev_ptr: int = 0, box_dev_ptr: int = 0):
        """fiesta_hip_corridor_bounds_dev: the waypoints, their CSR offsets and the corridor's arrays where ReachPathsDevice and
        PathCorridorDevice left them, n_boxes = min(the corridor's total, its capacity), and the outputs resident on the device (0:
        that array is not written); inset=None is resolution * 2.0 ** -20.  Only enqueued on the map's stream: bounds_dev_ptr can be
        handed to PathRefineDevice at once"""
        inset = self.resolution * 2.0 ** -20 if inset is None else float(inset)
        res = BoundsResult(int(bounds_dev_ptr) or None, int(ok_dev_ptr) or None, int(box_dev_ptr) or None)
        vp = lambda v: C.c_void_p(int(v) or None)  # noqa: E731
        check(self._lib.fiesta_hip_corridor_bounds_dev(self._h, vp(waypoints_vox_dev_ptr), int(n_waypoints), vp(path_offsets_dev_ptr), int(n_paths),
                                                       vp(box_offsets_dev_ptr), vp(boxes_dev_ptr), vp(boxes_pos_dev_ptr), vp(entry_dev_ptr),
                                                       vp(status_dev_ptr), int(n_boxes), inset, BOUNDS_VOID_BROKEN if void_broken else 0,
                                                       C.byref(res)))

    @staticmethod
    def _cluster_info(info) -> dict:
        return {k: int(getattr(info, k)) for k, _ in ClusterInfo._fields_}

    def ClusterVoxels(self, vox, mask=None, key=None, connectivity=26, min_size=1) -> dict:
        """fiesta_hip_cluster_voxels: the connected clusters (connectivity 6, 18 or 26) of the voxel list `vox` ((n, 3) map voxels, any
        order, e.g. GetFrontierVoxels' output), those below `min_size` distinct voxels dropped, the rest numbered by their lowest entry
        index.  mask ((n,) uint8) and key ((n,) int32, e.g. ReachField's target_cost) are optional per-entry data.  Returns label
        ((n,) int32, -1: no cluster), per cluster size, root, box_lo, box_hi, centroid (metres), mask_or, key_min and key_argmin, the
        CSR pair offsets / members (entry indices of each cluster's distinct voxels, unordered inside a cluster), and the totals of
        fiesta_hip_cluster_info; fiesta_amd.cluster_model is the definition"""
        v = np.ascontiguousarray(vox, dtype=np.int32).reshape(-1, 3)
        n = len(v)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        ky = None if key is None else np.ascontiguousarray(key, dtype=np.int32).reshape(-1)
        if (mk is not None and len(mk) != n) or (ky is not None and len(ky) != n):
            raise ValueError("mask and key need one value per entry")
        info = ClusterInfo()
        label = np.empty(n, np.int32)
        members = np.empty(n, np.int64)
        cap = min(n, 1 << 16)   # (clusters are few: one call serves unless there are more than this, then a second one with the total)
        while True:
            out = {name: np.empty((cap,) + shape, dtype) for name, dtype, shape in CLUSTER_FIELDS}
            out["offsets"] = np.zeros(cap + 1, np.int64)
            res = ClusterResult(label.ctypes.data, *[out[name].ctypes.data for name, _, _ in CLUSTER_FIELDS], out["offsets"].ctypes.data,
                                members.ctypes.data)
            check(self._lib.fiesta_hip_cluster_voxels(self._h, _p(v) if n else None, _p(mk), _p(ky), n, int(connectivity), int(min_size), cap, n,
                                                      C.byref(res), C.byref(info)))
            if info.n_clusters <= cap:
                break
            cap = int(info.n_clusters)
        k = int(info.n_clusters)
        out = {name: a[:k + 1] if name == "offsets" else a[:k] for name, a in out.items()}
        out["label"], out["members"] = label, members[:int(info.n_members)]
        out.update(self._cluster_info(info))
        return out

    def ClusterVoxelsDevice(self, vox_dev_ptr: int, n: int, info_dev_ptr: int, mask_dev_ptr: int = 0, key_dev_ptr: int = 0, n_dev_ptr: int = 0,
                            connectivity=26, min_size=1, cluster_capacity: int = 0, member_capacity: int = 0, out=None):
        """fiesta_hip_cluster_voxels_dev: every array resident on the device (`out` maps field names of fiesta_hip_cluster_result to
        device pointers, missing fields are not written; info_dev_ptr: a device fiesta_hip_cluster_info, six int64).  n_dev_ptr: a
        device 64-bit counter, the entry count is min(n, counter) -- GetFrontierVoxelsDevice's.  Only enqueued on the map's stream"""
        out = out or {}
        res = ClusterResult(*[int(out.get(name, 0)) or None for name, _ in ClusterResult._fields_])
        check(self._lib.fiesta_hip_cluster_voxels_dev(self._h, C.c_void_p(vox_dev_ptr or None), C.c_void_p(mask_dev_ptr or None),
                                                      C.c_void_p(key_dev_ptr or None), int(n), C.c_void_p(n_dev_ptr or None), int(connectivity),
                                                      int(min_size), int(cluster_capacity), int(member_capacity), C.byref(res),
                                                      C.c_void_p(info_dev_ptr or None)))

    def SplitClusters(self, vox, offsets, members, mask=None, key=None, max_size=0, max_extent=0, max_depth=63) -> dict:
        """fiesta_hip_split_clusters: bisect every oversize part of the clusters (offsets, members: ClusterVoxels' CSR pair over `vox`)
        at the middle of its box's longest axis until no part holds more than `max_size` members or spans more than `max_extent`
        voxels (0: criterion off), at most `max_depth` levels deep.  Returns per part parent (its cluster), depth, size, root, box_lo,
        box_hi, centroid (metres), mask_or, key_min, key_argmin; the CSR pair offsets / members of the parts; label ((n,) int32, -1:
        listed by no part); and n_parts, n_members, n_split_clusters, n_oversize, largest, deepest (fiesta_hip_split_info.depth) and
        status.  Parts need not be connected.  fiesta_amd.split_model is the definition"""
        v = np.ascontiguousarray(vox, dtype=np.int32).reshape(-1, 3)
        n = len(v)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        mem = np.ascontiguousarray(members, dtype=np.int64).reshape(-1)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        ky = None if key is None else np.ascontiguousarray(key, dtype=np.int32).reshape(-1)
        if (mk is not None and len(mk) != n) or (ky is not None and len(ky) != n):
            raise ValueError("mask and key need one value per entry")
        K, M = max(len(off) - 1, 0), len(mem)
        info = SplitInfo()
        label = np.empty(n, np.int32)
        out_members = np.empty(M, np.int64)
        cap = min(M, max(K, 1 << 12))   # (one call serves unless there are more parts than this, then a second one with the total)
        while True:
            out = {name: np.empty((cap,) + shape, dtype) for name, dtype, shape in SPLIT_FIELDS}
            out["offsets"] = np.zeros(cap + 1, np.int64)
            res = SplitResult(*[out[name].ctypes.data for name, _, _ in SPLIT_FIELDS], out["offsets"].ctypes.data, out_members.ctypes.data,
                              label.ctypes.data)
            check(self._lib.fiesta_hip_split_clusters(self._h, _p(v) if n else None, _p(mk), _p(ky), n, _p(off) if K else None, _p(mem) if M else None,
                                                      K, M, int(max_size), int(max_extent), int(max_depth), cap, C.byref(res), C.byref(info)))
            if info.n_parts <= cap:
                break
            cap = int(info.n_parts)
        k = int(info.n_parts)
        out = {name: a[:k + 1] if name == "offsets" else a[:k] for name, a in out.items()}
        out["label"], out["members"] = label, out_members[:int(info.n_members)]
        out.update(self._split_info(info))
        return out

    @staticmethod
    def _split_info(info) -> dict:
        return dict(zip(SPLIT_INFO_KEYS, (int(getattr(info, k)) for k, _ in SplitInfo._fields_)))

    def SplitClustersDevice(self, vox_dev_ptr: int, n: int, offsets_dev_ptr: int, members_dev_ptr: int, n_clusters: int, n_members: int,
                            info_dev_ptr: int, mask_dev_ptr: int = 0, key_dev_ptr: int = 0, n_clusters_dev_ptr: int = 0, max_size=0, max_extent=0,
                            max_depth=63, part_capacity: int = 0, out=None):
        """fiesta_hip_split_clusters_dev: every array resident on the device (`out` maps field names of fiesta_hip_split_result to
        device pointers, missing fields are not written; info_dev_ptr: a device fiesta_hip_split_info, seven int64).
        n_clusters_dev_ptr: a device int64, the cluster count is min(n_clusters, that) -- ClusterVoxelsDevice's info.  The outputs
        must not overlap the inputs.  Only enqueued on the map's stream"""
        out = out or {}
        res = SplitResult(*[int(out.get(name, 0)) or None for name, _ in SplitResult._fields_])
        vp = lambda v: C.c_void_p(int(v) or None)  # noqa: E731
        check(self._lib.fiesta_hip_split_clusters_dev(self._h, vp(vox_dev_ptr), vp(mask_dev_ptr), vp(key_dev_ptr), int(n), vp(offsets_dev_ptr),
                                                      vp(members_dev_ptr), int(n_clusters), vp(n_clusters_dev_ptr), int(n_members), int(max_size),
                                                      int(max_extent), int(max_depth), int(part_capacity), C.byref(res), vp(info_dev_ptr)))

    def _frontier_alloc(self) -> dict:
        """the device buffers FrontierClusters and FrontierViews share (torch tensors of self._frontier_capacity entries), made on demand"""
        import torch
        b = self._frontier_buffers
        if b is None:
            dev = torch.device("cuda", self.device)
            cap = self._frontier_capacity
            b = {"vox": torch.empty((cap, 3), dtype=torch.int32, device=dev), "mask": torch.empty(cap, dtype=torch.uint8, device=dev),
                 "label": torch.empty(cap, dtype=torch.int32, device=dev), "members": torch.empty(cap, dtype=torch.int64, device=dev),
                 "offsets": torch.empty(cap + 1, dtype=torch.int64, device=dev),
                 "head": torch.zeros(8, dtype=torch.int64, device=dev)}   # [0]: the frontier counter, [1 .. 6]: the cluster info
            for name, dtype, shape in CLUSTER_FIELDS:
                b[name] = torch.empty((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
            torch.cuda.synchronize(dev)   # (the map's stream does not wait for torch's)
            self._frontier_buffers = b
        return b

    def _split_alloc(self, b) -> dict:
        """the device buffers of the parts in FrontierClusters / FrontierViews (made with the first call that splits)"""
        import torch
        sp = b.get("split")
        if sp is None:
            dev = torch.device("cuda", self.device)
            cap = b["label"].shape[0]
            sp = {"label": torch.empty(cap, dtype=torch.int32, device=dev), "members": torch.empty(cap, dtype=torch.int64, device=dev),
                  "offsets": torch.empty(cap + 1, dtype=torch.int64, device=dev), "info": torch.zeros(len(SplitInfo._fields_), dtype=torch.int64, device=dev)}
            for name, dtype, shape in SPLIT_FIELDS:
                sp[name] = torch.empty((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
            torch.cuda.synchronize(dev)   # (the map's stream does not wait for torch's)
            b["split"] = sp
        return sp

    def _split_enqueue(self, b, sp, cluster_capacity, part_capacity, max_size, max_extent, max_depth):
        """SplitClustersDevice on the cluster call's buffers `b` into the part buffers `sp`: the cluster count comes from the device"""
        cap = b["label"].shape[0]
        self.SplitClustersDevice(b["vox"].data_ptr(), cap, b["offsets"].data_ptr(), b["members"].data_ptr(), cluster_capacity, cap,
                                 sp["info"].data_ptr(), mask_dev_ptr=b["mask"].data_ptr(), n_clusters_dev_ptr=b["head"].data_ptr() + 8,
                                 max_size=max_size, max_extent=max_extent, max_depth=max_depth, part_capacity=part_capacity,
                                 out={name: sp[name].data_ptr() for name, _ in SplitResult._fields_})

    @staticmethod
    def _split_results(out, sp, n):
        """replace the per-cluster entries of `out` by the parts'; returns the number of parts"""
        info = dict(zip(SPLIT_INFO_KEYS, (int(x) for x in sp["info"].cpu().numpy())))
        if info["status"] != 0:
            raise ValueError("the clusters handed to the split were broken (fiesta_hip_split_info.status INVALID)")
        k = info["n_parts"]
        for name, _, _ in SPLIT_FIELDS:
            out[name] = sp[name][:k].cpu().numpy()
        out["offsets"] = sp["offsets"][:k + 1].cpu().numpy()
        out["members"] = sp["members"][:info["n_members"]].cpu().numpy()
        out["label"] = sp["label"][:n].cpu().numpy()
        out.update(info)
        return k

    def FrontierClusters(self, lo=None, hi=None, min_clearance=0.0, connectivity=26, min_size=1, max_size=0, max_extent=0, max_depth=63) -> dict:
        """GetFrontierVoxels and ClusterVoxels as one chain on the device: the frontier sweep writes into device buffers this object
        keeps (torch tensors, grown on demand), its device counter feeds the clustering, and the host waits ONCE, at the end, before
        it copies the results back: vox, mask, and everything ClusterVoxels returns for that list.  Only when the buffers turn out too
        small for the frontier (the first call, a frontier that grew by more than a quarter) is the chain run a second time.
        With max_size or max_extent above 0 SplitClusters runs between the two, in the same buffers and with the same single wait:
        the results then describe the PARTS (plus parent, depth and SplitClusters' totals), n_clusters stays the unsplit count."""
        import torch
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        dev = torch.device("cuda", self.device)
        split = max_size > 0 or max_extent > 0
        while True:
            b = self._frontier_alloc()
            cap = b["label"].shape[0]
            head = b["head"].data_ptr()
            sp = self._split_alloc(b) if split else None
            self.GetFrontierVoxelsDevice(lo, hi, min_clearance, b["vox"].data_ptr(), b["mask"].data_ptr(), cap, head)
            outs = {name: b[name].data_ptr() for name, _ in ClusterResult._fields_}
            self.ClusterVoxelsDevice(b["vox"].data_ptr(), cap, head + 8, mask_dev_ptr=b["mask"].data_ptr(), n_dev_ptr=head,
                                     connectivity=connectivity, min_size=min_size, cluster_capacity=cap, member_capacity=cap, out=outs)
            if split:
                self._split_enqueue(b, sp, cap, cap, max_size, max_extent, max_depth)
            self.synchronize()
            h = b["head"].cpu().numpy()
            n = int(h[0])
            if n <= cap:
                break
            self._frontier_buffers, self._frontier_capacity = None, min(max(n + n // 4, 1024), 1 << 24)
            if n > 1 << 24:
                raise ValueError("the frontier holds more than 2^24 voxels: cluster it box by box")
        info = {name: int(h[1 + i]) for i, (name, _) in enumerate(ClusterInfo._fields_)}
        k = info["n_clusters"]
        out = {name: b[name][:k].cpu().numpy() for name, _, _ in CLUSTER_FIELDS}
        out["offsets"] = b["offsets"][:k + 1].cpu().numpy()
        out["members"] = b["members"][:info["n_members"]].cpu().numpy()
        out["vox"], out["mask"], out["label"] = b["vox"][:n].cpu().numpy(), b["mask"][:n].cpu().numpy(), b["label"][:n].cpu().numpy()
        out.update(info)
        if split:
            self._split_results(out, sp, n)
        return out

    @staticmethod
    def _view_sensor(min_range, max_range, tan_h, tan_v, block_mask, omni, min_clearance, min_visible):
        return ViewSensor(float(min_range), float(max_range), float(tan_h), float(tan_v), float(min_clearance), int(block_mask),
                          1 if omni else 0, int(min_visible), 0)

    def ViewCoverage(self, vox, pos=None, dir=None, group=None, centroid=None, ring=None, offsets=None, members=None, min_range=0.0,
                     max_range=np.inf, tan_h=np.inf, tan_v=np.inf, block_mask=1, omni=False, min_clearance=0.0, min_visible=1) -> dict:
        """fiesta_hip_view_coverage: candidate views against the target voxels `vox` ((n, 3) map voxels) of their group.  Views: pos
        (V, 3) metres, dir (V, 2) the horizontal unit forward vector, group (V,) -- or centroid (n_groups, 3) and ring (M, 5; see
        fiesta_amd.view_ring): ring j around centroid k is view k * M + j of group k.  offsets / members: the CSR pair of ClusterVoxels
        (both optional: one group of all entries; offsets alone: segments of vox itself).  Sensor: range in metres, the tangents of
        the half angles, block_mask (RAY_OCCUPIED | RAY_UNKNOWN | RAY_OUTSIDE: what ends a ray), omni (no forward direction),
        min_clearance (a view must stand this far from obstacles), min_visible (below it a view is nobody's best).  Returns per view
        view_class, n_in_view, n_visible (-1: unusable view); per entry cover_count, first_view; per group best_view, best_count; and
        n_usable, n_pairs, pairs_in_view, pairs_visible; fiesta_amd.view_coverage_model is the definition"""
        v = np.ascontiguousarray(vox, dtype=np.int32).reshape(-1, 3)
        n = len(v)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        mem = None if members is None else np.ascontiguousarray(members, dtype=np.int64).reshape(-1)
        G = 1 if off is None else len(off) - 1
        if G < 0:
            raise ValueError("offsets needs n_groups + 1 entries")
        vs = ViewSet()
        keep = []
        if pos is not None:
            ps = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
            V = len(ps)
            dr = None if dir is None else np.ascontiguousarray(dir, dtype=np.float64).reshape(-1, 2)
            gr = None if group is None else np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
            if (dr is not None and len(dr) != V) or (gr is not None and len(gr) != V):
                raise ValueError("dir and group need one row per view")
            # (a zero-length array still has to read as "given": the library tells the two forms apart by the pointers)
            one = np.zeros(3)
            vs.pos, vs.n_views = (ps if V else one).ctypes.data, V
            vs.dir = None if dr is None else (dr if V else one).ctypes.data
            vs.group = None if gr is None or not V else gr.ctypes.data
            keep += [ps, dr, gr, one]
        if centroid is not None:
            cn = np.ascontiguousarray(centroid, dtype=np.float64).reshape(-1, 3)
            rg = np.ascontiguousarray(ring if ring is not None else np.zeros((0, 5)), dtype=np.float64).reshape(-1, 5)
            if len(cn) != G:
                raise ValueError("centroid needs one row per group")
            one = np.zeros(5)
            vs.centroid, vs.ring, vs.n_ring = (cn if G else one).ctypes.data, (rg if len(rg) else one).ctypes.data if ring is not None else None, len(rg)
            V = G * len(rg)
            keep += [cn, rg, one]
        if pos is None and centroid is None:
            V = 0
        sizes = {"views": V, "entries": n, "groups": G}
        out = {name: np.empty(sizes[size], dtype) for name, dtype, size in VIEW_FIELDS}
        res = ViewResult(*[out[name].ctypes.data for name, _, _ in VIEW_FIELDS])
        sn = self._view_sensor(min_range, max_range, tan_h, tan_v, block_mask, omni, min_clearance, min_visible)
        info = ViewInfo()
        check(self._lib.fiesta_hip_view_coverage(self._h, _p(v) if n else None, n, _p(off), None if mem is None else _p(mem if len(mem) else np.zeros(1, np.int64)), G,
                                                 0 if mem is None else len(mem), C.byref(vs), C.byref(sn), C.byref(res), C.byref(info)))
        out.update(zip(VIEW_INFO_KEYS, (int(info.n_usable), int(info.n_pairs), int(info.n_in_view), int(info.n_visible))))
        return out

    def ViewCoverageDevice(self, vox_dev_ptr: int, n: int, info_dev_ptr: int, pos_dev_ptr: int = 0, dir_dev_ptr: int = 0, group_dev_ptr: int = 0,
                           n_views: int = 0, centroid_dev_ptr: int = 0, ring_dev_ptr: int = 0, n_ring: int = 0, offsets_dev_ptr: int = 0,
                           members_dev_ptr: int = 0, n_groups: int = 1, n_groups_dev_ptr: int = 0, n_members: int = 0, min_range=0.0,
                           max_range=np.inf, tan_h=np.inf, tan_v=np.inf, block_mask=1, omni=False, min_clearance=0.0, min_visible=1, out=None):
        """fiesta_hip_view_coverage_dev: every array resident on the device (`out` maps field names of fiesta_hip_view_result to device
        pointers, missing fields are not written; info_dev_ptr: a device fiesta_hip_view_info, four int64).  n_groups_dev_ptr: a
        device int64, the effective group count is min(n_groups, that) -- ClusterVoxelsDevice's info.  Only enqueued on the map's stream"""
        out = out or {}
        vs = ViewSet(pos_dev_ptr or None, dir_dev_ptr or None, group_dev_ptr or None, int(n_views), centroid_dev_ptr or None, ring_dev_ptr or None,
                     int(n_ring))
        res = ViewResult(*[int(out.get(name, 0)) or None for name, _ in ViewResult._fields_])
        sn = self._view_sensor(min_range, max_range, tan_h, tan_v, block_mask, omni, min_clearance, min_visible)
        check(self._lib.fiesta_hip_view_coverage_dev(self._h, C.c_void_p(vox_dev_ptr or None), int(n), C.c_void_p(offsets_dev_ptr or None),
                                                     C.c_void_p(members_dev_ptr or None), int(n_groups), C.c_void_p(n_groups_dev_ptr or None),
                                                     int(n_members), C.byref(vs), C.byref(sn), C.byref(res), C.c_void_p(info_dev_ptr or None)))

    def FrontierViews(self, lo=None, hi=None, min_clearance=0.0, connectivity=26, min_size=1, ring=None, min_range=0.0, max_range=np.inf,
                      tan_h=np.inf, tan_v=np.inf, block_mask=1, omni=False, view_clearance=0.0, min_visible=1, max_size=0, max_extent=0,
                      max_depth=63) -> dict:
        """With max_size or max_extent above 0 SplitClusters runs between clustering and coverage, as in FrontierClusters: the rings
        then stand around the PARTS' centroids and every per-cluster result describes a part.
        GetFrontierVoxels, ClusterVoxels and ViewCoverage (ring form: `ring` around every cluster's centroid, against the cluster's
        own members) as one chain on the device, in FrontierClusters' buffers: the frontier counter feeds the clustering, the cluster
        count and the CSR pair feed the coverage, and the host waits ONCE, at the end -- after a wait for torch's stream when a new ring
        was uploaded or buffers were made (the first call with a ring), and unless the buffers turn out too small for the
        frontier or the clusters (the first call, a frontier that grew by more than a quarter): then the chain runs a second time.
        Returns everything FrontierClusters returns and, for the views k * len(ring) + j, view_class, n_in_view, n_visible, view_pos, view_dir; per frontier voxel cover_count,
        first_view; per cluster best_view, best_count, best_pos, best_dir (NaN where best_view is -1); and ViewCoverage's totals"""
        import torch
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        rg = np.ascontiguousarray(ring, dtype=np.float64).reshape(-1, 5)
        M = len(rg)
        dev = torch.device("cuda", self.device)
        fresh = self._view_ring is None or self._view_ring[0] != rg.tobytes()    # (the uploaded ring is kept: a planner reuses it)
        if fresh:
            self._view_ring = (rg.tobytes(), torch.from_numpy(rg).to(dev) if M else torch.zeros((1, 5), dtype=torch.float64, device=dev))
        ring_dev = self._view_ring[1]
        split = max_size > 0 or max_extent > 0
        while True:
            b = self._frontier_alloc()
            cap = b["label"].shape[0]
            if split and "split" not in b:
                fresh = True
            sp = self._split_alloc(b) if split else None
            # the clusters get a capacity of their own (they are few): it sizes the views, kcap * len(ring) of them
            kcap = min(cap, self._view_cluster_capacity)
            if kcap * max(M, 1) > 1 << 24:
                raise ValueError("more than 2^24 views: use a smaller ring, a larger min_size or a smaller box")
            vb = b.get("views")
            if vb is None or vb["n_visible"].shape[0] < kcap * max(M, 1):
                nv = kcap * max(M, 1)
                vb = {"view_class": torch.empty(nv, dtype=torch.uint8, device=dev), "n_in_view": torch.empty(nv, dtype=torch.int32, device=dev),
                      "n_visible": torch.empty(nv, dtype=torch.int32, device=dev), "cover_count": torch.empty(cap, dtype=torch.int32, device=dev),
                      "first_view": torch.empty(cap, dtype=torch.int32, device=dev), "best_view": torch.empty(cap, dtype=torch.int64, device=dev),
                      "best_count": torch.empty(cap, dtype=torch.int32, device=dev), "info": torch.zeros(4, dtype=torch.int64, device=dev)}
                b["views"] = vb
                fresh = True
            if fresh:
                torch.cuda.synchronize(dev)   # (the map's stream does not wait for torch's: the ring upload, fresh buffers)
                fresh = False
            head = b["head"].data_ptr()
            self.GetFrontierVoxelsDevice(lo, hi, min_clearance, b["vox"].data_ptr(), b["mask"].data_ptr(), cap, head)
            outs = {name: b[name].data_ptr() for name, _ in ClusterResult._fields_}
            self.ClusterVoxelsDevice(b["vox"].data_ptr(), cap, head + 8, mask_dev_ptr=b["mask"].data_ptr(), n_dev_ptr=head,
                                     connectivity=connectivity, min_size=min_size, cluster_capacity=kcap, member_capacity=cap, out=outs)
            g = b
            if split:   # (the groups are the parts: their count -- info.n_parts -- and arrays come from the split's buffers)
                self._split_enqueue(b, sp, kcap, kcap, max_size, max_extent, max_depth)
                g = sp
            # (kcap groups; the device count -- info.n_clusters at head + 8, or info.n_parts -- cuts them down to the groups there are)
            self.ViewCoverageDevice(b["vox"].data_ptr(), cap, vb["info"].data_ptr(), centroid_dev_ptr=g["centroid"].data_ptr(),
                                    ring_dev_ptr=ring_dev.data_ptr(), n_ring=M, offsets_dev_ptr=g["offsets"].data_ptr(),
                                    members_dev_ptr=g["members"].data_ptr(), n_groups=kcap,
                                    n_groups_dev_ptr=sp["info"].data_ptr() if split else head + 8, n_members=cap,
                                    min_range=min_range, max_range=max_range, tan_h=tan_h, tan_v=tan_v, block_mask=block_mask, omni=omni,
                                    min_clearance=view_clearance, min_visible=min_visible,
                                    out={name: vb[name].data_ptr() for name, _ in ViewResult._fields_})
            self.synchronize()
            h = b["head"].cpu().numpy()
            n = int(h[0])
            if n > 1 << 24:
                raise ValueError("the frontier holds more than 2^24 voxels: cluster it box by box")
            if n > cap:
                self._frontier_buffers, self._frontier_capacity = None, min(max(n + n // 4, 1024), 1 << 24)
                continue
            groups = max(int(h[1]), int(sp["info"][0].item())) if split else int(h[1])
            if groups > kcap:
                self._view_cluster_capacity = groups + groups // 4
                continue
            break
        info = {name: int(h[1 + i]) for i, (name, _) in enumerate(ClusterInfo._fields_)}
        k = info["n_clusters"]
        out = {name: b[name][:k].cpu().numpy() for name, _, _ in CLUSTER_FIELDS}
        out["offsets"] = b["offsets"][:k + 1].cpu().numpy()
        out["members"] = b["members"][:info["n_members"]].cpu().numpy()
        out["vox"], out["mask"], out["label"] = b["vox"][:n].cpu().numpy(), b["mask"][:n].cpu().numpy(), b["label"][:n].cpu().numpy()
        out.update(info)
        if split:
            k = self._split_results(out, sp, n)
        for name in ("view_class", "n_in_view", "n_visible"):
            out[name] = vb[name][:k * M].cpu().numpy()
        for name in ("cover_count", "first_view"):
            out[name] = vb[name][:n].cpu().numpy()
        for name in ("best_view", "best_count"):
            out[name] = vb[name][:k].cpu().numpy()
        out.update(zip(VIEW_INFO_KEYS, (int(x) for x in vb["info"].cpu().numpy())))
        out["view_pos"] = (out["centroid"][:, None, :] + rg[None, :, :3]).reshape(-1, 3)
        out["view_dir"] = np.broadcast_to(rg[None, :, 3:5], (k, M, 2)).reshape(-1, 2).copy()
        has = out["best_view"] >= 0
        at = np.where(has, out["best_view"], 0)
        out["best_pos"] = np.where(has[:, None], out["view_pos"][at] if k * M else np.zeros((k, 3)), np.nan)
        out["best_dir"] = np.where(has[:, None], out["view_dir"][at] if k * M else np.zeros((k, 2)), np.nan)
        return out

    def count_no_obstacle(self) -> int:
        """Observed voxels whose distance reads +10000 (on grids beyond 1024 per axis this includes everything farther than
        512 voxels from every obstacle: the reach of a stored id, include/fiesta_hip.h)."""
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_count_no_obstacle(self._h, C.byref(n)))
        return n.value

    def GetSlice(self, z_vox: int) -> np.ndarray:
        """Distances of the plane z = z_vox as an (nx, ny) array (ESDFMap::GetSliceMarker, src/ESDFMap.cpp:639-699)."""
        out = np.empty(self.grid_size[:2], np.float64)
        check(self._lib.fiesta_hip_get_slice(self._h, int(z_vox), _p(out)))
        return out

    def save(self, path: str):
        """Raw checkpoint of the whole map state (include/fiesta_hip.h: fiesta_hip_save)."""
        check(self._lib.fiesta_hip_save(self._h, os.fsencode(path)))

    def load(self, path: str):
        check(self._lib.fiesta_hip_load(self._h, os.fsencode(path)))

    def GetPointCloud(self, vis_lower_bound: int, vis_upper_bound: int) -> np.ndarray:
        """ESDFMap::GetPointCloud (src/ESDFMap.cpp:544-582) as an (n, 3) float32 array of voxel centres (unordered)."""
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_get_point_cloud(self._h, vis_lower_bound, vis_upper_bound, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), np.float32)
        if n.value:
            check(self._lib.fiesta_hip_get_point_cloud(self._h, vis_lower_bound, vis_upper_bound, _p(out), n.value, C.byref(n)))
        return out

    def GetSliceMarker(self, slice_z: int, max_dist: float):
        """ESDFMap::GetSliceMarker (src/ESDFMap.cpp:639-699): (points (n,3) float64, colours (n,4) float32), unordered."""
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_get_slice_marker(self._h, slice_z, max_dist, None, None, 0, C.byref(n)))
        xyz = np.empty((n.value, 3), np.float64)
        rgba = np.empty((n.value, 4), np.float32)
        if n.value:
            check(self._lib.fiesta_hip_get_slice_marker(self._h, slice_z, max_dist, _p(xyz), _p(rgba), n.value, C.byref(n)))
        return xyz, rgba

    def download_counts(self):
        """Pending (num_hit_, num_miss_) per voxel; num_miss_ counts all observations (src/ESDFMap.cpp:424)."""
        n = self.grid_total_size_
        hit = np.empty(n, np.int32)
        miss = np.empty(n, np.int32)
        check(self._lib.fiesta_hip_download_counts(self._h, _p(hit), _p(miss)))
        return hit, miss

    def download_hash(self):
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_download_hash(self._h, C.byref(n), None, None, None, None))
        vox = np.empty((n.value, 3), np.int32)
        d2 = np.empty(n.value, np.int32)
        coc = np.empty((n.value, 3), np.int32)
        occ = np.empty(n.value, np.uint8)
        check(self._lib.fiesta_hip_download_hash(self._h, C.byref(n), _p(vox), _p(d2), _p(coc), _p(occ)))
        return {"vox": vox, "d2": d2, "coc": coc, "occ": occ}

    def hash_window(self):
        """Hash-block mode: (origin, moves) of the moving window -- map voxel of its lowest corner (it spans 1024 voxels per
        axis) and how often it has moved (include/fiesta_hip.h, "the moving window")."""
        org = np.zeros(3, np.int32)
        moves = C.c_int64(0)
        check(self._lib.fiesta_hip_hash_window(self._h, _p(org), C.byref(moves)))
        return org, moves.value

    def hash_recentre(self, centre_vox):
        c = np.ascontiguousarray(centre_vox, np.int32).reshape(3)
        check(self._lib.fiesta_hip_hash_recentre(self._h, _p(c)))

    def distance_from_d2(self, d2):
        """distance_buffer_ as the reference stores it: -10000 / +10000 sentinels, else sqrt(d2)*res."""
        d2 = np.asarray(d2)
        out = np.sqrt(np.maximum(d2, 0).astype(np.float64)) * self.resolution
        out[d2 < 0] = UNDEFINED
        out[d2 == D2_INF] = INFINITY
        return out

    def snapshot_save(self, slot=0):
        check(self._lib.fiesta_hip_snapshot_save(self._h, slot))

    def snapshot_restore(self, slot=0):
        check(self._lib.fiesta_hip_snapshot_restore(self._h, slot))

    def snapshot_count_updated(self, slot=0) -> int:
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_snapshot_count_updated(self._h, slot, C.byref(n)))
        return n.value

    def synchronize(self):
        check(self._lib.fiesta_hip_synchronize(self._h))

    # -- shard interface (driven by fiesta_amd.sharded.ShardedESDFMap) ---------------------------
    def shard_info(self) -> dict:
        info = _lib.ShardInfo()
        check(self._lib.fiesta_hip_shard_info_get(self._h, C.byref(info)))
        return {k: tuple(getattr(info, k)) for k, _ in _lib.ShardInfo._fields_}

    def halo_pack(self, lo, hi) -> np.ndarray:
        lo = np.ascontiguousarray(lo, dtype=np.int32)
        hi = np.ascontiguousarray(hi, dtype=np.int32)
        out = np.empty(tuple(int(b - a + 1) for a, b in zip(lo, hi)), np.uint32)
        check(self._lib.fiesta_hip_halo_pack(self._h, _p(lo), _p(hi), _p(out)))
        return out

    def halo_apply(self, lo, hi, words) -> int:
        lo = np.ascontiguousarray(lo, dtype=np.int32)
        hi = np.ascontiguousarray(hi, dtype=np.int32)
        w = np.ascontiguousarray(words, dtype=np.uint32)
        assert w.size == int(np.prod(hi - lo + 1)), "halo buffer does not match the box"
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_halo_apply(self._h, _p(lo), _p(hi), _p(w), C.byref(n)))
        return n.value

    def halo_pack_dev(self, lo, hi, out_ptr: int):
        lo = np.ascontiguousarray(lo, dtype=np.int32)
        hi = np.ascontiguousarray(hi, dtype=np.int32)
        check(self._lib.fiesta_hip_halo_pack_dev(self._h, _p(lo), _p(hi), C.c_void_p(out_ptr)))

    def halo_apply_dev(self, lo, hi, in_ptr: int) -> int:
        lo = np.ascontiguousarray(lo, dtype=np.int32)
        hi = np.ascontiguousarray(hi, dtype=np.int32)
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_halo_apply_dev(self._h, _p(lo), _p(hi), C.c_void_p(in_ptr), C.byref(n)))
        return n.value

    def export_transitions(self) -> np.ndarray:
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_export_transitions(self._h, None, 0, C.byref(n)))
        out = np.empty(2 * n.value, np.uint32)   # two words per entry: x | y << 16, z | occupied << 31
        if n.value:
            check(self._lib.fiesta_hip_export_transitions(self._h, _p(out), n.value, C.byref(n)))
        return out

    def apply_transitions(self, entries):
        e = np.ascontiguousarray(entries, dtype=np.uint32).reshape(-1)
        check(self._lib.fiesta_hip_apply_transitions(self._h, _p(e), len(e) // 2))

    def export_transitions_dev(self, out_ptr: int, capacity: int) -> int:
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_export_transitions_dev(self._h, C.c_void_p(out_ptr) if out_ptr else None, capacity,
                                                          C.byref(n)))
        return n.value

    def apply_transitions_dev(self, ptr: int, n: int):
        check(self._lib.fiesta_hip_apply_transitions_dev(self._h, C.c_void_p(ptr), n))

    def esdf_seed(self) -> dict:
        st = Stats()
        check(self._lib.fiesta_hip_esdf_seed(self._h, C.byref(st)))
        return st.as_dict()

    def relax_pending(self):
        st = Stats()
        n = C.c_int64(0)
        check(self._lib.fiesta_hip_relax_pending(self._h, C.byref(st), C.byref(n)))
        return n.value, st.as_dict()


def signed_distance(esdf_map: "ESDFMap", inverse_map: "ESDFMap", pos_or_vox) -> np.ndarray:
    """Signed distance of a SIGNED_NEEDED pair (include/Fiesta.h:39-41; the reference leaves the combination as a TODO,
    :515-518): the map's distance to the nearest occupied voxel minus the inverse map's distance to the nearest voxel
    observed free -- positive in free space, negative inside obstacles.  NaN where either map holds no distance."""
    d, di = esdf_map.GetDistance(pos_or_vox), inverse_map.GetDistance(pos_or_vox)
    ok = (np.abs(d) < INFINITY) & (np.abs(di) < INFINITY)
    return np.where(ok, d - di, np.nan)
