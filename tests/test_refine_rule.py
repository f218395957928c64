"""CPU side of path refinement (fiesta_hip_path_refine, include/fiesta_hip.h): the definition.

fiesta_amd.path_refine_model (numpy) is the model the GPU tests compare the kernels with, so it must be the header's formulas: it is
checked against a literal per-waypoint, per-component Python loop over them, one float at a time, bit for bit; its G is checked to be
the derivative of its J by central differences on an analytic field (the comparison tests/test_path_cost_rule.py uses for path cost's
gradient); then the invariants the header states, every invalid-path case, every whole-call error through the built library (none
needs a device), fiesta_amd.corridor_bounds on hand-made corridors, and the resources of the k_refine kernels.
"""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE, RADIUS, CAP = (1.3, 0.9, 1.1), 0.5, 10000.0
PAR = dict(margin=1.2, w_obstacle=1.5, w_smooth=0.8, alpha=0.05, max_step=0.04, tolerance=0.0, iterations=5)


def sphere(p):
    """distance to one sphere, capped at 10000 (gradient 0 where capped), and its exact gradient"""
    d = [p[c] - CENTRE[c] for c in range(3)]
    r = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if r - RADIUS >= CAP:
        return CAP, [0.0, 0.0, 0.0]
    return r - RADIUS, [d[0] / r, d[1] / r, d[2] / r]


def batch(fn):
    def query(pos):
        res = [fn([float(v) for v in q]) for q in pos]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res]).reshape(-1, 3)
    return query


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def refine_loop(fn, waypoints, offsets, bounds, margin, w_obstacle, w_smooth, alpha, max_step, tolerance, iterations):
    """The header's formulas, one Python float at a time (IEEE f64, no contraction); J summed in waypoint order."""
    n_paths = len(offsets) - 1
    out = {"waypoints": [list(map(float, r)) for r in waypoints], "cost": [[0.0, 0.0] for _ in range(n_paths)], "last_move": [0.0] * n_paths,
           "iterations": [0] * n_paths, "n_below": [0] * n_paths, "min_dist": [math.inf] * n_paths, "status": [0] * n_paths}

    def sample(x):
        d, g = fn(x)
        if d < margin:
            e = margin - d
            psi = -2.0 * e
            return d, e * e, [psi * g[0], psi * g[1], psi * g[2]]
        return d, 0.0, [0.0, 0.0, 0.0]

    def second(w, j, c):
        if j <= 0 or j >= len(w) - 1:
            return 0.0
        return (w[j - 1][c] - 2.0 * w[j][c]) + w[j + 1][c]

    def J(w):
        total = 0.0
        for i in range(1, len(w) - 1):
            a = [second(w, i, c) for c in range(3)]
            total += w_obstacle * sample(w[i])[1] + w_smooth * ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        return total

    for p in range(n_paths):
        o0, o1 = int(offsets[p]), int(offsets[p + 1])
        w = [[float(c) for c in waypoints[i]] for i in range(o0, o1)]
        m = len(w)
        bad = m > 1024 or not all(abs(c) <= 2.0 ** 40 for v in w for c in v)
        if bounds is not None:
            for i in range(1, m - 1):
                b = [float(v) for v in bounds[o0 + i]]
                bad = bad or not all(b[c] <= b[3 + c] for c in range(3))
        if bad:
            out["cost"][p] = [math.nan, math.nan]
            out["last_move"][p] = out["min_dist"][p] = math.nan
            out["iterations"][p] = out["n_below"][p] = -1
            out["status"][p] = 1
            continue
        out["cost"][p][0] = J(w)
        if m > 2:
            for _ in range(iterations):
                new = [list(v) for v in w]
                last = 0.0
                for i in range(1, m - 1):
                    gam = sample(w[i])[2]
                    for c in range(3):
                        s = (second(w, i - 1, c) - 2.0 * second(w, i, c)) + second(w, i + 1, c)
                        G = w_obstacle * gam[c] + (2.0 * w_smooth) * s
                        delta = alpha * G
                        if delta > max_step:
                            delta = max_step
                        if delta < -max_step:
                            delta = -max_step
                        x = w[i][c] - delta
                        if bounds is not None:
                            lo, hi = float(bounds[o0 + i][c]), float(bounds[o0 + i][3 + c])
                            if x < lo:
                                x = lo
                            if x > hi:
                                x = hi
                        last = max(last, abs(x - w[i][c]))
                        new[i][c] = x
                w = new
                out["last_move"][p] = last
                out["iterations"][p] += 1
                if last <= tolerance:
                    break
        out["cost"][p][1] = J(w)
        for v in w:
            d = sample(v)[0]
            out["n_below"][p] += d < margin
            out["min_dist"][p] = min(out["min_dist"][p], d)
        out["waypoints"][o0:o1] = w
    return {k: np.array(v) for k, v in out.items()}


def assert_same(got, want, what, cost_model=None):
    for k in ("waypoints", "last_move", "min_dist"):
        assert np.array_equal(bits(got[k]).reshape(-1), bits(want[k]).reshape(-1)), (what, k, got[k], want[k])
    for k in ("iterations", "n_below", "status"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (what, k, got[k], want[k])
    a, b = np.asarray(got["cost"], np.float64).reshape(-1, 2), np.asarray(want["cost"], np.float64).reshape(-1, 2)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "cost")
    model = cost_model or got
    lim = (model["cost_n"] + 16.0) * 2.0 ** -52 * model["cost_abs"]
    assert (np.where(np.isnan(a), 0.0, np.abs(a - b)) <= lim).all(), (what, "cost", a, b)


def paths(lengths, seed, spread=0.9):
    rng = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    w = np.array(CENTRE) + rng.randn(int(off[-1]), 3) * spread
    return w, off


def boxes(w, seed):
    """bounds around the waypoints: finite boxes, some a single point, some sides infinite"""
    rng = np.random.RandomState(seed)
    b = np.concatenate([w - rng.rand(*w.shape) * 0.05, w + rng.rand(*w.shape) * 0.05], axis=1)
    b[::5, 0] = -np.inf
    b[1::5, 4] = np.inf
    b[2::7, :3] = b[2::7, 3:] = w[2::7]
    return b


# ---- 1. the model is the header's formulas ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounded", [False, True])
def test_the_model_equals_the_header_formulas(bounded):
    import fiesta_amd
    w, off = paths([0, 1, 2, 3, 4, 5, 9], 3)
    b = boxes(w, 4) if bounded else None
    for it, tol in ((0, 0.0), (1, 0.0), (6, 0.0), (6, 0.03)):
        par = dict(PAR, iterations=it, tolerance=tol)
        got = fiesta_amd.path_refine_model(batch(sphere), w, off, b, **par)
        want = refine_loop(sphere, w, off, b, **par)
        assert_same(got, want, f"bounded {bounded}, {it} iterations, tolerance {tol}")
        assert got["cost_n"].tolist() == [[max(0, n - 2)] * 2 for n in np.diff(off)]
    assert (got["iterations"] > 0).any() and (np.abs(got["waypoints"] - w) > 1e-3).any()


# ---- 2. G is the derivative of J -------------------------------------------------------------------------------------------------
def test_G_is_the_derivative_of_J():
    """central differences of J at eps = 1e-6 in every waypoint coordinate against G, to 1e-5 of the largest component of G: the
    comparison and the tolerance of tests/test_path_cost_rule.py::test_the_gradient_is_the_derivative_of_the_cost"""
    import fiesta_amd
    eps = 1e-6
    par = dict(margin=1.5, w_obstacle=1.5, w_smooth=0.8)
    w, off = paths([7, 3, 5, 4], 11, 0.8)
    query = batch(sphere)
    G, J = fiesta_amd.path_refine_gradient(query, w, off, **par)
    fd = np.zeros_like(w)
    for p in range(len(off) - 1):
        o0, o1 = off[p], off[p + 1]
        for i in range(o0 + 1, o1 - 1):
            for c in range(3):
                hi, lo = w[o0:o1].copy(), w[o0:o1].copy()
                hi[i - o0, c] += eps
                lo[i - o0, c] -= eps
                jh = fiesta_amd.path_refine_gradient(query, hi, [0, o1 - o0], **par)[1][0]
                jl = fiesta_amd.path_refine_gradient(query, lo, [0, o1 - o0], **par)[1][0]
                fd[i, c] = (jh - jl) / (2 * eps)
    ends = np.concatenate([off[:-1], off[1:] - 1])
    assert not G[ends].any() and G.any(axis=1).sum() == len(w) - len(ends)
    scale = np.abs(G).max()
    worst = np.abs(fd - G).max() / scale
    print(f"central differences: worst deviation {worst:.3g} of the largest component of G {scale:.3g}")
    assert scale > 0.1 and worst <= 1e-5
    # and the model's first step is alpha * G, where neither clamp binds
    got = fiesta_amd.path_refine_model(query, w, off, None, alpha=1e-3, max_step=1e3, iterations=1, **par)
    assert np.array_equal(bits(got["waypoints"]), bits(w - 1e-3 * G))
    assert np.array_equal(bits(got["cost"][:, 0]), bits(J))


# ---- 3. invariants --------------------------------------------------------------------------------------------------------------------
def test_invariants():
    import fiesta_amd
    query = batch(sphere)
    w, off = paths([9, 2, 17, 4, 3], 5)
    b = boxes(w, 6)
    ends = np.concatenate([off[:-1], off[1:] - 1])
    inner = np.setdiff1d(np.arange(len(w)), ends)
    full = fiesta_amd.path_refine_model(query, w, off, b, **dict(PAR, iterations=12))
    assert np.array_equal(bits(full["waypoints"][ends]), bits(w[ends]))                       # the ends never move
    assert (full["waypoints"][inner] >= b[inner, :3]).all() and (full["waypoints"][inner] <= b[inner, 3:]).all()
    zero = fiesta_amd.path_refine_model(query, w, off, b, **dict(PAR, iterations=0))
    assert np.array_equal(bits(zero["waypoints"]), bits(w)) and not zero["iterations"].any() and not zero["last_move"].any()
    assert np.array_equal(bits(zero["cost"][:, 0]), bits(zero["cost"][:, 1]))
    # per-iteration motion within max_step per component (free waypoints, large gradients)
    prev = w
    for k in range(1, 5):
        cur = fiesta_amd.path_refine_model(query, w, off, None, **dict(PAR, alpha=50.0, w_smooth=0.001, iterations=k))["waypoints"]
        assert (np.abs(cur - prev) <= PAR["max_step"] * (1 + 2.0 ** -50)).all() and np.abs(cur - prev).max() > 0.9 * PAR["max_step"]
        prev = cur
    # an equally spaced straight line clear of the margin is a fixed point (dyadic spacing: the second differences are exactly 0)
    line = np.array([8.0, 8.0, 8.0]) + np.arange(9)[:, None] * np.array([0.25, 0.5, -0.125])
    fix = fiesta_amd.path_refine_model(query, line, [0, 9], None, **dict(PAR, iterations=7))
    assert np.array_equal(bits(fix["waypoints"]), bits(line)) and fix["last_move"][0] == 0.0 and fix["n_below"][0] == 0
    assert fix["cost"].tolist() == [[0.0, 0.0]] and fix["iterations"][0] == 1                 # (0 <= tolerance: it stops)
    # early stop: iterations out is the first k with last_move <= tolerance, and the result is that of iterations = k
    tol = 0.02
    runs = [fiesta_amd.path_refine_model(query, w, off, b, **dict(PAR, iterations=k)) for k in range(0, 31)]
    stop = fiesta_amd.path_refine_model(query, w, off, b, **dict(PAR, iterations=30, tolerance=tol))
    assert len(set(stop["iterations"].tolist())) >= 3, stop["iterations"]                      # some early, some not
    for p in range(len(off) - 1):
        k = int(stop["iterations"][p])
        if off[p + 1] - off[p] <= 2:
            assert k == 0
            continue
        moves = [runs[j]["last_move"][p] for j in range(1, 31)]                                # last_move of iteration j
        first = next((j for j in range(1, 31) if moves[j - 1] <= tol), 30)
        assert k == first, (p, k, first)
        sl = slice(off[p], off[p + 1])
        assert np.array_equal(bits(stop["waypoints"][sl]), bits(runs[k]["waypoints"][sl]))
        assert bits(stop["last_move"][p:p + 1]) == bits(runs[k]["last_move"][p:p + 1])
        assert np.array_equal(bits(stop["cost"][p]), bits(runs[k]["cost"][p]))


# ---- 4. invalid paths, whole-call errors ------------------------------------------------------------------------------------------------
def test_every_invalid_path_case_leaves_the_others_alone():
    import fiesta_amd
    query = batch(sphere)
    w, off = paths([5, 4, 1025, 4, 3, 6, 4], 7)
    b = boxes(w, 8)
    w[off[1] + 3, 1] = np.nan                  # a non-finite END of path 1
    w[off[3] + 1, 2] = 2.0 ** 40 * (1 + 2.0 ** -50)   # beyond 2^40 (path 3); path 2 has 1025 waypoints
    b[off[4] + 1, 3] = np.nan                  # a NaN in an interior bounds row (path 4)
    b[off[5] + 2, 1], b[off[5] + 2, 4] = 1.0, 0.5    # lo > hi (path 5)
    b[off[6], :] = np.nan                      # an END's bounds row is not read (path 6 stays valid)
    b[off[6] + 3, 0], b[off[6] + 3, 3] = 2.0, 1.0
    got = fiesta_amd.path_refine_model(query, w, off, b, **PAR)
    assert got["status"].tolist() == [0, 1, 1, 1, 1, 1, 0]
    inv = got["status"] == 1
    assert np.isnan(got["cost"][inv]).all() and np.isnan(got["last_move"][inv]).all() and np.isnan(got["min_dist"][inv]).all()
    assert (got["iterations"][inv] == -1).all() and (got["n_below"][inv] == -1).all()
    rows = np.repeat(inv, np.diff(off))
    assert np.array_equal(bits(got["waypoints"][rows]), bits(w[rows]))
    for p in (0, 6):                            # the valid paths: as if they were alone
        sl = slice(off[p], off[p + 1])
        alone = fiesta_amd.path_refine_model(query, w[sl], [0, off[p + 1] - off[p]], b[sl], **PAR)
        assert np.array_equal(bits(alone["waypoints"]), bits(got["waypoints"][sl])) and alone["iterations"][0] == got["iterations"][p] > 0
    two = fiesta_amd.path_refine_model(query, [[np.inf, 0, 0], [1, 1, 1]], [0, 2], None, **PAR)   # ends are checked too
    assert two["status"].tolist() == [1]
    for bad in (dict(margin=np.nan), dict(w_obstacle=-1.0), dict(alpha=0.0), dict(max_step=np.inf), dict(tolerance=-1.0), dict(iterations=1025)):
        with pytest.raises(ValueError):
            fiesta_amd.path_refine_model(query, w, off, b, **dict(PAR, **bad))
    with pytest.raises(ValueError):
        fiesta_amd.path_refine_model(query, w, [0, 3, 2, len(w)], None, **PAR)


def test_whole_call_errors_need_no_device():
    """every whole-call error of the header, through the built library; the checks come before the map handle is looked at, so a
    NULL handle shows that each of them fires first (and a call with nothing wrong reports the handle)"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd._lib import RefineParams, RefineResult
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    w = np.zeros((3, 3))
    off = np.array([0, 3], np.int64)
    out = np.zeros((3, 3))
    res = RefineResult(out.ctypes.data, None, None, None, None, None, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = dict(margin=0.5, w_obstacle=1.0, w_smooth=1.0, alpha=0.1, max_step=0.1, tolerance=0.0, iterations=3, flags=0)

    def call(fn, par, wp=p(w), n_wp=3, offs=p(off), n_paths=1, r=C.byref(res)):
        st = fn(None, wp, n_wp, offs, n_paths, None, C.byref(RefineParams(**par)) if par else None, r)
        return st, fiesta_amd._lib.last_error()

    inf, nan, big = float("inf"), float("nan"), 2.0 ** 20 * (1 + 2.0 ** -50)
    bad_params = [dict(margin=nan), dict(margin=inf), dict(margin=-big), dict(w_obstacle=-0.1), dict(w_obstacle=big), dict(w_obstacle=nan),
                  dict(w_smooth=-0.1), dict(w_smooth=big), dict(w_smooth=nan), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=big), dict(alpha=nan),
                  dict(max_step=0.0), dict(max_step=big), dict(max_step=inf), dict(max_step=nan), dict(tolerance=-1e-9), dict(tolerance=inf),
                  dict(tolerance=nan), dict(iterations=-1), dict(iterations=1025), dict(flags=1), dict(flags=-1)]
    for fn in (lib.fiesta_hip_path_refine, lib.fiesta_hip_path_refine_dev):
        for bad in bad_params:
            st, msg = call(fn, dict(good, **bad))
            assert st == 1 and "path_refine" in msg and "handle" not in msg, (bad, st, msg)
        for kw in (dict(wp=None), dict(offs=None), dict(r=None), dict(n_wp=-1), dict(n_paths=-1)):
            st, msg = call(fn, good, **kw)
            assert st == 1 and "path_refine" in msg and "handle" not in msg, (kw, st, msg)
        st, msg = call(fn, None)
        assert st == 1 and "handle" not in msg
        st, msg = call(fn, good)                                       # nothing wrong but the handle
        assert st == 1 and "null map handle" in msg
        st, msg = call(fn, dict(good, margin=-2.0 ** 20, w_obstacle=0.0, w_smooth=2.0 ** 20, alpha=2.0 ** 20, max_step=2.0 ** 20, iterations=1024))
        assert "null map handle" in msg                                # the limits themselves are in range
    for offs in ([1, 3], [0, 2], [0, 4]):                              # the host variant checks the CSR rules
        st, msg = call(lib.fiesta_hip_path_refine, good, offs=p(np.array(offs, np.int64)))
        assert st == 1 and "offsets" in msg, (offs, msg)
    st, msg = call(lib.fiesta_hip_path_refine, good, offs=p(np.array([0, 2, 1, 3], np.int64)), n_paths=3)
    assert st == 1 and "offsets" in msg


def test_the_ctypes_mirrors_match_the_header():
    from fiesta_amd import _lib
    import fiesta_amd.esdf_map as em
    text = open(_lib.HEADER_PATH).read()
    for struct, mirror in (("fiesta_hip_refine_params", _lib.RefineParams), ("fiesta_hip_refine_result", _lib.RefineResult)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        decls = [d.strip() for d in body.split(";") if d.strip()]
        assert [d.split(None, 1)[1].lstrip("*").strip() for d in decls] == [f[0] for f in mirror._fields_], struct
        if mirror is _lib.RefineParams:
            ctype = {"double": C.c_double, "int32_t": C.c_int32}
            assert [ctype[d.split(None, 1)[0]] for d in decls] == [f[1] for f in mirror._fields_]
        else:
            assert all(d.split(None, 1)[1].startswith("*") for d in decls)
            names = {"double": np.float64, "int32_t": np.int32, "int64_t": np.int64}
            assert [names[d.split(None, 1)[0]] for d in decls] == [f[1] for f in em.REFINE_FIELDS]
            assert [f[0] for f in em.REFINE_FIELDS] == [f[0] for f in mirror._fields_]
    for name, value in (("MAX_WAYPOINTS", 1024), ("MAX_ITERATIONS", 1024), ("OK", 0), ("INVALID", 1)):
        assert re.search(r"#define FIESTA_HIP_REFINE_%s %d\b" % (name, value), text), name
    import fiesta_amd
    assert (fiesta_amd.REFINE_MAX_WAYPOINTS, fiesta_amd.REFINE_MAX_ITERATIONS, fiesta_amd.REFINE_OK, fiesta_amd.REFINE_INVALID) == (1024, 1024, 0, 1)


# ---- 5. corridor_bounds -----------------------------------------------------------------------------------------------------------------
def corridor(boxes_by_path, entries_by_path, status, res=0.5):
    bx = np.array([b for bs in boxes_by_path for b in bs], np.int32).reshape(-1, 6)
    pos = np.concatenate([bx[:, :3] * res, (bx[:, 3:] + 1.0) * res], axis=1)
    return {"offsets": np.concatenate([[0], np.cumsum([len(b) for b in boxes_by_path])]).astype(np.int64), "boxes": bx, "boxes_pos": pos,
            "entry": np.array([e for es in entries_by_path for e in es], np.int32), "status": np.array(status, np.int32)}


def test_corridor_bounds_on_hand_made_corridors():
    import fiesta_amd
    A, B, Cx, D = [0, 0, 0, 4, 3, 3], [3, 0, 0, 8, 2, 2], [7, 1, 0, 9, 9, 1], [0, 0, 0, 1, 1, 1]
    # path 0: chain indices 0 2 3 5 7 11 -- boxes A (entry 0), B (entry 4), C (entry 8)
    p0 = [[1, 1, 1], [3, 1, 1], [4, 1, 1], [6, 1, 1], [8, 1, 1], [8, 5, 1]]
    # path 1: jumps from its first box to its third (the second is entered and left between two waypoints)
    p1 = [[1, 1, 1], [8, 2, 1], [8, 6, 1]]
    # path 2: BLOCKED after its only box; path 3: empty; path 4: one waypoint
    p2 = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0]]
    p4 = [[8, 8, 1]]
    wv = np.array(p0 + p1 + p2 + p4, np.int32)
    off = np.array([0, 6, 9, 13, 13, 14], np.int64)
    cor = corridor([[A, B, Cx], [A, B, Cx], [D], [], [Cx]], [[0, 4, 8], [0, 4, 8], [0], [], [0]], [0, 0, 2, 0, 0])
    bounds, ok = fiesta_amd.corridor_bounds(wv, off, cor, inset=0.0)
    assert ok.tolist() == [True, False, False, True, True]
    pos = cor["boxes_pos"]
    both = lambda a, b: np.concatenate([np.maximum(pos[a, :3], pos[b, :3]), np.minimum(pos[a, 3:], pos[b, 3:])])  # noqa: E731
    # the box by entry index: c = 0 2 3 | 5 7 | 11; the intersection where the NEXT waypoint is in the next box
    want0 = [pos[0], pos[0], both(0, 1), pos[1], both(1, 2), pos[2]]
    assert np.array_equal(bounds[:6], np.array(want0))
    assert (bounds[2, :3] <= bounds[2, 3:]).all() and (bounds[4, :3] <= bounds[4, 3:]).all()
    assert np.array_equal(bounds[6:9], pos[[3, 5, 5]])                 # a skipped box: each waypoint keeps its own box
    assert np.array_equal(bounds[9:13], pos[[6, 6, 6, 6]])             # BLOCKED: the boxes made so far
    assert np.array_equal(bounds[13], pos[7])
    # by default the upper faces are pulled in by 2^-20 of a voxel: a clamped waypoint stays in the box's last voxel
    inner, ok_in = fiesta_amd.corridor_bounds(wv, off, cor)
    assert np.array_equal(ok_in, ok) and np.array_equal(inner[:, :3], bounds[:, :3]) and np.array_equal(inner[:, 3:], bounds[:, 3:] - 0.5 * 2.0 ** -20)
    assert (np.floor(inner[:, 3:] / 0.5) == np.floor(bounds[:, 3:] / 0.5) - 1).all()
    # a first waypoint outside the box its successor changes to cannot be covered: it never moves
    cor2 = corridor([[D, [1, 1, 1, 5, 5, 5]]], [[0, 3]], [0])
    _, ok2 = fiesta_amd.corridor_bounds([[0, 0, 0], [1, 1, 1], [2, 2, 2]], [0, 3], cor2)
    cor3 = corridor([[D, [0, 0, 0, 5, 5, 5]]], [[0, 3]], [0])
    _, ok3 = fiesta_amd.corridor_bounds([[0, 0, 0], [1, 1, 1], [2, 2, 2]], [0, 3], cor3)
    assert ok2.tolist() == [False] and ok3.tolist() == [True]
    # a path without any box (BLOCKED at its first waypoint): NaN rows, which the refinement reports as INVALID
    cor4 = corridor([[]], [[]], [2])
    b4, ok4 = fiesta_amd.corridor_bounds([[0, 0, 0], [1, 0, 0], [2, 0, 0]], [0, 3], cor4)
    assert ok4.tolist() == [False] and np.isnan(b4).all()
    with pytest.raises(ValueError):
        fiesta_amd.corridor_bounds(wv, off[:-1], cor)


# ---- 6. the kernels' resources ----------------------------------------------------------------------------------------------------------
def test_refine_kernels_do_not_spill():
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_refine" in k}
    assert len(res) == 4, sorted(res)                                   # two team sizes x the dense and the hash-block evaluator
    assert sum("DensePathEval" in k for k in res) == 2 and sum("HashPathEval" in k for k in res) == 2
    for k, v in res.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
