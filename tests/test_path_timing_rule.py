"""The rule of fiesta_hip_path_timing (include/fiesta_hip.h) on analytic distance fields, without a device: fiesta_amd.path_timing_model
against a literal per-sample loop of the header's text, the scan form of the profile against the serial recurrence, the profile's
bounds, closed forms (trapezoid and triangle profiles, the corner rule), the special paths and argument errors, and the resources of
the k_timing kernels.
"""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = dict(step=0.07, margin=0.2, v_max=1.5, v_min=0.1, a_max=1.2, corner_dev=0.03, v_start=0.0, v_end=0.0)
FREE = 10000.0


def wall(p):
    """a plane wall at y = 0: the distance is y, capped at 10000"""
    return min(p[1], FREE)


def sphere(p):
    return min(math.sqrt((p[0] - 1.3) ** 2 + (p[1] - 0.9) ** 2 + (p[2] - 1.1) ** 2) - 0.5, FREE)


def free(p):
    return FREE


def batch(fn):
    return lambda pos: (np.array([fn(p) for p in pos]), None)


def model(fn, w, off, **par):
    import fiesta_amd
    return fiesta_amd.path_timing_model(batch(fn), np.asarray(w, float).reshape(-1, 3), off, detail=True, **par)


def literal(fn, w, step, margin, v_max, v_min, a_max, corner_dev, v_start, v_end):
    """one valid path, sample by sample, in the words of the header; the profile as running minima"""
    m = len(w)
    A, Vq, Mq = 2.0 * a_max, v_max * v_max, v_min * v_min
    d = [[w[j + 1][c] - w[j][c] for c in range(3)] for j in range(m - 1)]
    L = [math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) for x in d]
    S = [max(1, math.ceil(l / step)) for l in L]
    W = [0.0]
    for l in L:
        W.append(W[-1] + l)
    s, lq, seg, n_below = [], [], [], 0
    for j in range(m):
        for k in range(S[j] if j < m - 1 else 1):
            if j < m - 1:
                t = float(k) / float(S[j])
                pos = [w[j][c] + d[j][c] * t for c in range(3)]
                s.append(W[j] + L[j] * t)
                seg.append(j)
            else:
                pos = list(w[j])
                s.append(W[j])
            dist = fn(pos)
            if dist < margin:
                x = Mq
                n_below += 1
            else:
                x = A * (dist - margin)
                if x > Vq:
                    x = Vq
                if x < Mq:
                    x = Mq
            if k == 0 and 1 <= j <= m - 2 and math.isfinite(corner_dev) and L[j - 1] > 0 and L[j] > 0:
                u = [d[j - 1][c] / L[j - 1] for c in range(3)]
                v = [d[j][c] / L[j] for c in range(3)]
                c = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
                c = 1.0 if c > 1.0 else c
                c = -1.0 if c < -1.0 else c
                sh = math.sqrt(0.5 * (1.0 + c))
                den = 1.0 - sh
                if den > 0:
                    cq = ((a_max * corner_dev) * sh) / den
                    if cq < x:
                        x = cq
            lq.append(x)
    n = len(lq)
    if v_start * v_start < lq[0]:
        lq[0] = v_start * v_start
    if v_end * v_end < lq[n - 1]:
        lq[n - 1] = v_end * v_end
    P = [A * x for x in s]
    f, b, run = [0.0] * n, [0.0] * n, math.inf
    for k in range(n):
        run = min(run, lq[k] - P[k])
        f[k] = run + P[k]
    run = math.inf
    for k in range(n - 1, -1, -1):
        run = min(run, lq[k] + P[k])
        b[k] = run - P[k]
    q = [min(lq[k], f[k], b[k]) for k in range(n)]
    v = [math.sqrt(x) for x in q]
    dt = []
    for k in range(n - 1):
        h = L[seg[k]] / float(S[seg[k]])
        sv = v[k] + v[k + 1]
        dt.append(0.0 if h == 0 else ((2.0 * h) / sv if sv > 0 else 2.0 * math.sqrt(h / a_max)))
    first = [0]
    for x in S:
        first.append(first[-1] + x)
    time = [0.0]
    for x in dt:
        time.append(time[-1] + x)
    return dict(lq=lq, s=s, q=q, v=v, dt=dt, duration=time[-1], length=W[-1], n_samples=n, n_below=n_below, min_speed=min(v),
                min_index=v.index(min(v)), time=[time[i] for i in first], speed=[v[i] for i in first], h=[L[j] / float(S[j]) for j in seg])


def random_batch(rng, n_paths=12):
    paths = []
    for p in range(n_paths):
        m = int(rng.randint(1, 14))
        pts = np.array([0.6, 0.5, 0.6]) + np.cumsum(rng.randn(m, 3) * 0.25, axis=0)
        if p % 3 == 0 and m > 3:
            pts[2] = pts[1]                                               # a zero-length segment
            pts[m - 1] = pts[m - 3]                                       # ... and a reversal onto an earlier waypoint
        if p % 4 == 1 and m > 2:
            pts[2] = pts[1] + (pts[1] - pts[0]) * 0.7                     # a straight joint
        paths.append(pts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return np.concatenate(paths), off


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- 1. the model is the header's text -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [wall, sphere, free])
def test_model_equals_the_literal_loop(field):
    rng = np.random.RandomState(len(field.__name__))
    for trial in range(4):
        w, off = random_batch(rng)
        par = dict(PAR, v_start=[0.0, 0.3][trial % 2], v_end=[0.0, 2.0][trial // 2], corner_dev=[0.03, math.inf, 0.2, 0.001][trial])
        out = model(field, w, off, **par)
        assert (out["status"] == 0).all()
        for p in range(len(off) - 1):
            ref = literal(field, w[off[p]:off[p + 1]].tolist(), **par)
            det = out["detail"][p]
            for k in ("lq", "s", "q", "v", "dt"):
                assert np.array_equal(bits(det[k]), bits(ref[k])), (p, k)
            for k in ("duration", "length", "min_speed"):
                assert bits(out[k][p:p + 1])[0] == bits([ref[k]])[0], (p, k)
            for k in ("n_samples", "n_below", "min_index"):
                assert out[k][p] == ref[k], (p, k)
            for k in ("time", "speed"):
                assert np.array_equal(bits(out[k][off[p]:off[p + 1]]), bits(ref[k])), (p, k)
            assert out["duration_n"][p] == ref["n_samples"] - 1 and out["duration_abs"][p] == ref["duration"]


# ---- 2., 3. the scan form against the serial recurrence; the profile's bounds ------------------------------------------------------------
def test_scan_form_equals_the_serial_recurrence_and_keeps_its_bounds():
    rng = np.random.RandomState(11)
    worst = 0.0
    for trial in range(25):
        w, off = random_batch(rng)
        par = dict(PAR, a_max=float(rng.choice([0.3, 1.2, 4.0])), v_start=float(rng.choice([0.0, 0.5])), v_end=float(rng.choice([0.0, 0.5])))
        out = model([wall, sphere, free][trial % 3], w, off, **par)
        A, Vq = 2.0 * par["a_max"], par["v_max"] ** 2
        for p, det in out["detail"].items():
            lq, q, h = det["lq"], det["q"], det["h"]
            n = len(lq)
            tol = 4 * 2.0 ** -52 * (A * out["length"][p] + Vq)            # each q carries at most three roundings of magnitude <= M
            ser = lq.copy()
            for k in range(n - 1):
                ser[k + 1] = min(ser[k + 1], ser[k] + A * h[k])
            for k in range(n - 2, -1, -1):
                ser[k] = min(ser[k], ser[k + 1] + A * h[k])
            worst = max(worst, float(np.abs(q - ser).max()) / (2.0 ** -52 * (A * out["length"][p] + Vq)))
            assert np.abs(q - ser).max() <= tol, (trial, p)
            assert (q <= lq).all() and (q >= 0).all()
            if n > 1:
                assert (np.abs(np.diff(q)) <= A * h + tol).all(), (trial, p)
    print(f"scan form vs serial recurrence: worst {worst:.3g} * 2^-52 * M")


# ---- 4., 6. closed forms ------------------------------------------------------------------------------------------------------------------
def test_trapezoid_and_triangle_profiles():
    par = dict(step=0.25, margin=0.0, v_max=2.0, v_min=0.1, a_max=2.0, corner_dev=math.inf)
    out = model(free, [[0, 0, 0], [4, 0, 0]], [0, 2], **par)             # 1 m up, 2 m at 2 m/s, 1 m down: the switch points are samples
    assert out["n_samples"][0] == 17 and abs(out["duration"][0] - 3.0) <= 3e-12 and out["length"][0] == 4.0
    assert out["speed"].tolist() == [0.0, 0.0] and abs(out["time"][1] - 3.0) <= 3e-12 and out["min_index"][0] == 0
    assert out["detail"][0]["v"].max() == 2.0
    for L, a in ((0.2, 2.0), (0.25, 0.7), (1e-3, 5.0)):                   # one interval, rest to rest: the triangle
        out = model(free, [[1, 1, 1], [1, 1 + L, 1]], [0, 2], **dict(par, a_max=a, step=0.25))
        assert out["n_samples"][0] == 2 and out["duration"][0] == 2.0 * math.sqrt(((1 + L) - 1) / a)


# ---- 5. the corner rule -------------------------------------------------------------------------------------------------------------------
def test_corner_rule():
    par = dict(step=0.5, margin=0.0, v_max=3.0, v_min=0.1, a_max=2.0, corner_dev=0.05, v_start=3.0, v_end=3.0)
    a, dev = par["a_max"], par["corner_dev"]
    joint = lambda pts, **kw: model(free, pts, [0, len(pts)], **dict(par, **kw))  # noqa: E731
    straight = joint([[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    assert straight["speed"].tolist() == [3.0, 3.0, 3.0]
    right = joint([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    sh = math.sqrt(0.5)
    assert abs(right["speed"][1] / math.sqrt(((a * dev) * sh) / (1.0 - sh)) - 1.0) <= 1e-12 and right["speed"][0] > right["speed"][1]
    assert right["detail"][0]["lq"][2] == ((a * dev) * sh) / (1.0 - sh)
    back = joint([[0, 0, 0], [1, 0, 0], [0.25, 0, 0]])
    assert back["speed"][1] == 0.0 and back["min_index"][0] == 2 and np.isfinite(back["duration"][0]) and back["duration"][0] > 0
    zero = joint([[0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 1, 0]])           # a zero-length neighbour on both sides of the bend
    assert zero["speed"].tolist() == [3.0] * 4 and zero["n_samples"][0] == 6
    off_ = joint([[0, 0, 0], [1, 0, 0], [1, 1, 0]], corner_dev=math.inf)
    assert off_["speed"].tolist() == [3.0, 3.0, 3.0]


# ---- 7. below the margin ------------------------------------------------------------------------------------------------------------------
def test_samples_below_the_margin_run_at_v_min():
    par = dict(step=0.1, margin=0.3, v_max=2.0, v_min=0.2, a_max=50.0, corner_dev=math.inf, v_start=2.0, v_end=2.0)
    out = model(wall, [[0, 0.05, 0], [0, 1.05, 0]], [0, 2], **par)       # straight away from the wall: d = y
    det = out["detail"][0]
    below = det["d"] < 0.3
    # ((lq - P) + P may round one step below lq: v_min to rounding)
    assert out["n_below"][0] == below.sum() == 3 and (np.abs(det["v"][below] - 0.2) <= 1e-12).all() and (det["v"][~below] > 0.2 + 1e-3).all()
    assert abs(out["min_speed"][0] - 0.2) <= 1e-12 and out["min_index"][0] in (0, 1, 2) and out["speed"][1] == 2.0


# ---- 8. special paths and argument errors ---------------------------------------------------------------------------------------------------
def test_special_paths_and_argument_errors():
    import fiesta_amd
    from fiesta_amd import TIMING_INVALID, TIMING_MAX_SAMPLES, TIMING_MAX_WAYPOINTS, TIMING_OK, TIMING_TOO_LONG
    assert (TIMING_OK, TIMING_INVALID, TIMING_TOO_LONG, TIMING_MAX_WAYPOINTS, TIMING_MAX_SAMPLES) == (0, 1, 2, 1024, 4096)
    hdr = open(os.path.join(ROOT, "include", "fiesta_hip.h")).read()
    for name, value in (("OK", 0), ("INVALID", 1), ("TOO_LONG", 2), ("MAX_WAYPOINTS", 1024), ("MAX_SAMPLES", 4096)):
        assert f"#define FIESTA_HIP_TIMING_{name} {value}" in hdr
    many = np.cumsum(np.full((1025, 3), 1e-3), axis=0)
    paths = [np.zeros((0, 3)), [[1, 1, 1]], [[0, 1, 0], [np.nan, 1, 0]], [[0, 1, 0], [0.07 * 4096 + 0.01, 1, 0]], [[0, 1, 0], [0.07 * 4095, 1, 0]],
             many, [[0, 1, 0], [0.07 * 2.0 ** 24 * 1.01, 1, 0]], [[0, 1, 0], [np.inf, 1, 0]], [[0, 1, 0], [0.5, 1, 0]]]
    paths = [np.asarray(p, float).reshape(-1, 3) for p in paths]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])])
    out = model(wall, np.concatenate(paths), off, **PAR)
    assert out["status"].tolist() == [0, 0, 1, 2, 0, 2, 1, 1, 0]
    assert out["n_samples"].tolist() == [0, 1, -1, -1, 4096, -1, -1, -1, 9]
    assert out["duration"][0] == 0 and out["length"][0] == 0 and out["n_below"][0] == 0 and np.isinf(out["min_speed"][0]) and out["min_index"][0] == -1
    assert out["duration"][1] == 0 and out["min_index"][1] == 0 and out["speed"][0] == 0.0 and out["time"][0] == 0.0
    one = model(wall, [[1, 1, 1]], [0, 1], **dict(PAR, v_start=0.7, v_end=0.4))
    assert one["speed"][0] == math.sqrt(0.4 * 0.4)                        # a path of one sample takes both ends
    for p in (2, 3, 5, 6, 7):
        assert np.isnan([out["duration"][p], out["length"][p], out["min_speed"][p]]).all() and out["n_below"][p] == -1 and out["min_index"][p] == -1
        assert np.isnan(out["time"][off[p]:off[p + 1]]).all() and np.isnan(out["speed"][off[p]:off[p + 1]]).all()
    assert np.isfinite(out["duration"][[4, 8]]).all() and not np.isnan(out["time"][off[8]:off[9]]).any()
    nan, inf = math.nan, math.inf
    w, o = [[0, 1, 0], [1, 1, 0]], [0, 2]
    for wrong in (dict(step=0.0), dict(step=nan), dict(step=inf), dict(margin=-0.1), dict(margin=nan), dict(margin=inf), dict(v_max=0.0),
                  dict(v_max=inf), dict(v_min=0.0), dict(v_min=1.6), dict(v_min=nan), dict(a_max=0.0), dict(a_max=inf), dict(corner_dev=0.0),
                  dict(corner_dev=nan), dict(corner_dev=-inf), dict(v_start=-1.0), dict(v_start=inf), dict(v_end=-1.0), dict(v_end=nan)):
        with pytest.raises(ValueError):
            fiesta_amd.path_timing_model(batch(wall), w, o, **dict(PAR, **wrong))
    for bad_off in ([1, 2], [0, 1], [0, 3], [0, 2, 1, 2], []):
        with pytest.raises(ValueError):
            fiesta_amd.path_timing_model(batch(wall), w, bad_off, **PAR)


# ---- 9. the kernels' resources --------------------------------------------------------------------------------------------------------------
def test_timing_kernels_do_not_spill():
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_timing" in k}
    assert len(res) == 4, sorted(res)                                   # two team sizes x the dense and the hash-block evaluator
    assert sum("DensePathEval" in k for k in res) == 2 and sum("HashPathEval" in k for k in res) == 2
    for k, v in res.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
