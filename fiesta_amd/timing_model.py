"""The definition of fiesta_hip_path_timing (include/fiesta_hip.h) in numpy.

path_timing_model   the whole call over path_samples: a loop over the paths, every per-sample and per-interval TERM vectorised in the
                    header's operation order (bit for bit what the library computes from the same sample values), the two prefix
                    minima by np.minimum.accumulate (min is exact: no order), the sums of dt by np.cumsum (sample order).
No fused multiply-add anywhere: numpy rounds every operation once, as the library does (-ffp-contract=off).
"""
from __future__ import annotations

import numpy as np

TIMING_MAX_WAYPOINTS = 1024
TIMING_MAX_SAMPLES = 4096
TIMING_OK = 0
TIMING_INVALID = 1
TIMING_TOO_LONG = 2
_MAX_RATIO = 2.0 ** 24  # path_samples' limit on L / step


def _check_params(step, margin, v_max, v_min, a_max, corner_dev, v_start, v_end):
    fin = np.isfinite
    if not (fin(step) and step > 0):
        raise ValueError("step must be finite and > 0")
    if not (fin(margin) and margin >= 0):
        raise ValueError("margin must be finite and >= 0")
    if not (fin(v_max) and v_max > 0):
        raise ValueError("v_max must be finite and > 0")
    if not (fin(v_min) and 0 < v_min <= v_max):
        raise ValueError("v_min must be finite, 0 < v_min <= v_max")
    if not (fin(a_max) and a_max > 0):
        raise ValueError("a_max must be finite and > 0")
    if not corner_dev > 0:                                            # (a NaN fails the comparison; +inf: no corner rule)
        raise ValueError("corner_dev must be > 0")
    if not (fin(v_start) and v_start >= 0):
        raise ValueError("v_start must be finite and >= 0")
    if not (fin(v_end) and v_end >= 0):
        raise ValueError("v_end must be finite and >= 0")


def path_timing_model(query, waypoints, offsets, *, step, margin, v_max, v_min, a_max, corner_dev, v_start=0.0, v_end=0.0, detail=False):
    """fiesta_hip_path_timing in numpy.  `query(pos) -> (d, grad)` answers an (N, 3) batch: a map's GetDistWithGradTrilinear, or any
    callable (only d is used).  Returns a dict: the nine outputs (duration, length, n_samples, n_below, min_speed, min_index,
    status per path; time, speed per waypoint) and, for the tolerance of a comparison with another order of summation, the number
    of summed terms and the sum of their absolute values: duration_n / duration_abs per path, time_n / time_abs per waypoint.
    Two orders of summation differ by at most (n + 16) * 2^-52 * abs.  With detail=True out["detail"][p] holds the per-sample arrays of
    every timed path p (s, lq, q, v, d) and its per-interval h and dt.  Raises ValueError for the call's whole-call errors."""
    from .esdf_map import path_samples
    w = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    step, margin, v_max, v_min, a_max, corner_dev, v_start, v_end = (float(x) for x in (step, margin, v_max, v_min, a_max, corner_dev, v_start, v_end))
    _check_params(step, margin, v_max, v_min, a_max, corner_dev, v_start, v_end)
    if len(off) < 1 or off[0] != 0 or off[-1] != len(w) or np.any(np.diff(off) < 0):
        raise ValueError("offsets: n_paths + 1 non-decreasing entries from 0 to n_waypoints")
    n_paths = len(off) - 1
    A, Vq, Mq = 2.0 * a_max, v_max * v_max, v_min * v_min
    a_dev = a_max * corner_dev
    vs2, ve2 = v_start * v_start, v_end * v_end
    nan = np.nan
    out = {"duration": np.zeros(n_paths), "length": np.zeros(n_paths), "n_samples": np.zeros(n_paths, np.int64),
           "n_below": np.zeros(n_paths, np.int64), "min_speed": np.full(n_paths, np.inf), "min_index": np.full(n_paths, -1, np.int64),
           "status": np.zeros(n_paths, np.int32), "time": np.full(len(w), nan), "speed": np.full(len(w), nan),
           "duration_n": np.zeros(n_paths, np.int64), "duration_abs": np.zeros(n_paths),
           "time_n": np.zeros(len(w), np.int64), "time_abs": np.zeros(len(w))}
    if detail:
        out["detail"] = {}
    # ---- status, in the header's order: the waypoint count, the waypoints and segments, the sample count ----
    segs = {}
    for p in range(n_paths):
        o0, o1 = int(off[p]), int(off[p + 1])
        m = o1 - o0
        if m == 0:
            continue
        st = TIMING_OK
        if m > TIMING_MAX_WAYPOINTS:
            st = TIMING_TOO_LONG
        else:
            a = w[o0:o1]
            with np.errstate(invalid="ignore", over="ignore"):
                dd = a[1:] - a[:-1]
                L = np.sqrt(dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2])
                ratio = L / step
            if not np.all(np.isfinite(a)) or not np.all(ratio <= _MAX_RATIO):
                st = TIMING_INVALID
            else:
                S = np.maximum(1, np.ceil(ratio)).astype(np.int64)
                if int(S.sum()) + 1 > TIMING_MAX_SAMPLES:
                    st = TIMING_TOO_LONG
                else:
                    segs[p] = (dd, L, S)
        if st != TIMING_OK:
            out["status"][p] = st
            out["duration"][p] = out["length"][p] = out["min_speed"][p] = nan
            out["n_samples"][p] = out["n_below"][p] = -1
    # ---- the samples of the timed paths, by path clearance's rule, and their values ----
    timed = sorted(segs)
    if timed:
        sub_w = np.concatenate([w[off[p]:off[p + 1]] for p in timed])
        sub_off = np.concatenate([[0], np.cumsum([off[p + 1] - off[p] for p in timed])])
        pos, ns = path_samples(sub_w, sub_off, step)
        d = np.asarray(query(pos)[0], np.float64).reshape(-1) if len(pos) else np.zeros(0)
    at = 0
    for i, p in enumerate(timed):
        dd, L, S = segs[p]
        o0, o1 = int(off[p]), int(off[p + 1])
        m, n = o1 - o0, int(ns[i])
        assert n == int(S.sum()) + 1
        dv = d[at:at + n]
        at += n
        first = np.concatenate([[0], np.cumsum(S)]).astype(np.int64)   # the sample of every waypoint
        W = np.concatenate([[0.0], np.cumsum(L)])                       # (cumsum adds in segment order)
        sidx = np.repeat(np.arange(m - 1), S)                           # the segment of every sample but the final one
        kk = np.arange(n - 1) - first[sidx]
        Sd = S.astype(np.float64)
        s = np.concatenate([W[sidx] + L[sidx] * (kk.astype(np.float64) / Sd[sidx]), [W[m - 1]]])
        # clearance limit
        below = dv < margin
        lq = A * (dv - margin)
        lq = np.where(lq > Vq, Vq, lq)
        lq = np.where(lq < Mq, Mq, lq)
        lq = np.where(below, Mq, lq)
        # corner limit at the interior waypoints
        if np.isfinite(corner_dev) and m >= 3:
            L0, L1 = L[:-1], L[1:]
            ok = (L0 > 0) & (L1 > 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                u, v = dd[:-1] / L0[:, None], dd[1:] / L1[:, None]
                c = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
                c = np.where(c > 1.0, 1.0, c)
                c = np.where(c < -1.0, -1.0, c)
                sh = np.sqrt(0.5 * (1.0 + c))
                den = 1.0 - sh
                cq = (a_dev * sh) / den
            at_wp = first[1:m - 1]
            use = ok & (den > 0) & (cq < lq[at_wp])
            lq[at_wp[use]] = cq[use]
        # ends
        if vs2 < lq[0]:
            lq[0] = vs2
        if ve2 < lq[n - 1]:
            lq[n - 1] = ve2
        # profile
        P = A * s
        f = np.minimum.accumulate(lq - P) + P
        b = np.minimum.accumulate((lq + P)[::-1])[::-1] - P
        q = lq.copy()
        q = np.where(f < q, f, q)
        q = np.where(b < q, b, q)
        v = np.sqrt(q)
        # intervals
        h = (L / Sd)[sidx]
        sv = v[:-1] + v[1:]
        with np.errstate(invalid="ignore", divide="ignore"):
            dt = np.where(h == 0, 0.0, np.where(sv > 0, (2.0 * h) / sv, 2.0 * np.sqrt(h / a_max)))
        t = np.concatenate([[0.0], np.cumsum(dt)])                      # the time of every sample, added in sample order
        out["duration"][p] = t[-1]
        out["length"][p] = W[m - 1]
        out["n_samples"][p] = n
        out["n_below"][p] = int(np.count_nonzero(below))
        out["min_speed"][p] = v.min()
        out["min_index"][p] = int(np.argmin(v))                         # (the first index that attains the minimum)
        out["time"][o0:o1] = t[first]
        out["speed"][o0:o1] = v[first]
        out["duration_n"][p], out["duration_abs"][p] = n - 1, t[-1]     # (dt >= 0: the sum is its own absolute sum)
        out["time_n"][o0:o1], out["time_abs"][o0:o1] = first, t[first]
        if detail:
            out["detail"][p] = {"s": s, "lq": lq, "q": q, "v": v, "dt": dt, "h": h, "d": dv}
    return out
