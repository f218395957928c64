"""CPU side of the batched path cost (fiesta_hip_path_cost, include/fiesta_hip.h): the definition.

fiesta_amd.path_cost_model (numpy) is the model the GPU tests compare the kernels with, so it must be the header's formulas: it is
checked against a plain Python loop over them, one float at a time, on the special cases the header names; its gradient is checked
to be the derivative of its cost by central differences on an analytic field.  Also: the ctypes mirror of
fiesta_hip_path_cost_result, and that the library's k_cost_* kernels use no scratch.

The tolerance of every float comparison between two orders of summation is the header's: (n + 16) * 2^-52 * A with n the number of
summed terms and A the sum of their absolute values on the output's scale, both from the model (`bound`).
"""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX_LO, BOX_HI = (-2.0, -2.0, -2.0), (6.0, 6.0, 6.0)
CENTRE, RADIUS = (1.3, 0.9, 1.1), 0.5


def sphere(p):
    """distance to one sphere and its exact gradient"""
    d = [p[c] - CENTRE[c] for c in range(3)]
    r = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return r - RADIUS, [d[0] / r, d[1] / r, d[2] / r]


def boxed_sphere(p):
    """the sphere inside a box, the point query's answer outside it: -1 and no gradient"""
    if not all(BOX_LO[c] <= p[c] < BOX_HI[c] for c in range(3)):
        return -1.0, [0.0, 0.0, 0.0]
    return sphere(p)


def batch(fn):
    def query(pos):
        res = [fn([float(v) for v in q]) for q in pos]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res]).reshape(-1, 3)
    return query


def bound(n, a):
    return (np.asarray(n, np.float64) + 16.0) * 2.0 ** -52 * np.asarray(a, np.float64)


def cost_loop(fn, waypoints, offsets, step, margin):
    """The header's formulas, one Python float at a time (IEEE f64, no contraction), every sum in sample / segment order."""
    n_paths = len(offsets) - 1
    out = {"cost": [0.0] * n_paths, "length": [0.0] * n_paths, "n_below": [0] * n_paths, "n_samples": [0] * n_paths,
           "grad": [[0.0, 0.0, 0.0] for _ in range(len(waypoints))]}

    def penalty(q):
        d, g = fn(q)
        if d < margin:
            e = margin - d
            psi = -2.0 * e
            return 1, e * e, [psi * g[0], psi * g[1], psi * g[2]]
        return 0, 0.0, [0.0, 0.0, 0.0]

    for p in range(n_paths):
        o0 = int(offsets[p])
        w = [tuple(float(c) for c in waypoints[i]) for i in range(o0, int(offsets[p + 1]))]
        segs, bad = [], not all(math.isfinite(c) for v in w for c in v)
        for a, b in zip(w[:-1], w[1:]):
            d = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
            L = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if not L / step <= 2.0 ** 24:
                bad = True
                break
            segs.append((a, d, L, max(1, int(math.ceil(L / step)))))
        if bad:
            out["cost"][p] = out["length"][p] = math.nan
            out["n_below"][p] = out["n_samples"][p] = -1
            continue
        if not w:
            continue
        nb, ends, sums = 0, [], []
        for a, d, L, S in segs:
            s = [0.0] * 7
            for k in range(S):
                t = float(k) / float(S)
                below, phi, gam = penalty([a[c] + d[c] * t for c in range(3)])
                nb += below
                if k == 0:
                    ends.append((phi, gam))
                else:
                    r = 1.0 - t
                    for c, x in enumerate([phi] + [r * v for v in gam] + [t * v for v in gam]):
                        s[c] += x
            sums.append(s)
        below, phi, gam = penalty(list(w[-1]))
        nb += below
        ends.append((phi, gam))
        cost = length = 0.0
        for j, (a, d, L, S) in enumerate(segs):
            length += L
            if not L > 0:
                continue
            Sd = float(S)
            h = L / Sd
            Q = (ends[j][0] * 0.5 + sums[j][0]) + ends[j + 1][0] * 0.5
            qs = Q / Sd
            cost += h * Q
            for c in range(3):
                u = d[c] / L
                out["grad"][o0 + j][c] += h * (ends[j][1][c] * 0.5 + sums[j][1 + c]) - qs * u
                out["grad"][o0 + j + 1][c] += h * (sums[j][4 + c] + ends[j + 1][1][c] * 0.5) + qs * u
        out["cost"][p], out["length"][p], out["n_below"][p] = cost, length, nb
        out["n_samples"][p] = sum(s[3] for s in segs) + 1
    return {k: np.array(v) for k, v in out.items()}


def assert_close(got, want, model, what=""):
    """integers exact; floats within the summation bound built from the model's (n, A); NaN where NaN"""
    for k in ("n_samples", "n_below"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("cost", "length", "grad"):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        n = model[k + "_n"] if k != "grad" else model["grad_n"][:, None]
        lim = bound(n, model[k + "_abs"])
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, k)
        err = np.where(np.isnan(a), 0.0, np.abs(a - b))
        print(f"{what} {k}: worst error / bound = {np.max(err / np.maximum(lim, 1e-300), initial=0.0):.3g}")
        bad = np.argwhere(err > lim)
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries beyond the bound, first {bad[:3].tolist()}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}"


def test_path_cost_model_equals_the_header_formulas_on_special_cases():
    import fiesta_amd
    step, margin = 0.1, 1.2
    W = np.array([[1.0, 2.0, 3.0],                                                      # 0: one waypoint
                  [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.33, 0.1, 0.0], [0.9, 0.7, 1.0],  # 1: a zero-length segment first
                  [1.0, 0.0, 1.0], [1.05, 0.02, 1.0], [1.1, 0.0, 1.03], [1.12, 0.05, 1.0],   # 2: S = 1 segments only
                  [0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [1.0, 1.0, 1.0],                 # 3: invalid, in the middle of the batch
                  [0.5, 0.5, 0.5], [2.5, 1.5, 1.0], [2.5, 1.5, 1.0], [0.2, 1.4, 1.7],   # 4: long segments, a zero-length one inside
                  [5.0, 5.0, 5.0], [7.5, 5.0, 5.0], [5.5, 7.0, 5.0], [5.0, 5.5, 5.5],   # 6: leaves the box and comes back
                  [0.0, 0.0, 0.0], [2.0 ** 24 * 0.1 * 1.5, 0.0, 0.0]])                  # 7: L / step > 2^24: invalid
    off = np.array([0, 1, 5, 9, 12, 16, 16, 20, 22])                                    # (5: empty)
    got = fiesta_amd.path_cost_model(batch(boxed_sphere), W, off, step, margin)
    want = cost_loop(boxed_sphere, W, off, step, margin)
    assert_close(got, want, got, "special cases")
    assert list(got["n_samples"]) == [1, 1 + 4 + 13 + 1, 4, -1, 23 + 1 + 25 + 1, 0, 25 + 29 + 17 + 1, -1], got["n_samples"]
    assert got["n_below"][3] == -1 and got["n_below"][7] == -1 and np.isnan(got["cost"][[3, 7]]).all() and np.isnan(got["length"][[3, 7]]).all()
    assert got["cost"][0] == 0 and got["length"][0] == 0 and got["n_below"][0] == 0 and not got["grad"][0].any()   # 1.9 m from the sphere
    assert got["cost"][5] == 0 and got["length"][5] == 0 and got["n_below"][5] == 0
    assert not got["grad"][9:12].any()                                                   # rows of an invalid path are 0
    assert got["cost"][2] > 0 and got["grad"][5:9].any(1).all()                          # S = 1 segments: the end samples alone carry it
    assert got["n_below"][6] > 20 and got["cost"][6] > 0                                 # outside the box: phi(-1), counted
    # outside the box the penalty is constant: only the segment lengths pull (the -+ Q / S * u terms)
    far = fiesta_amd.path_cost_model(batch(boxed_sphere), [[7, 7, 7], [9, 7, 7], [9, 8, 7]], [0, 3], 0.25, 1.0)
    assert far["cost"][0] == 4.0 * 3.0 and far["n_below"][0] == 13
    assert np.array_equal(far["grad"], [[-4.0, 0, 0], [4.0, -4.0, 0], [0, 4.0, 0]])
    # a margin below every value: nothing at all
    none = fiesta_amd.path_cost_model(batch(boxed_sphere), W, off, step, -2.0)
    assert not np.nan_to_num(none["cost"]).any() and not none["grad"].any() and (none["n_below"][[0, 1, 2, 4, 5, 6]] == 0).all()
    with pytest.raises(ValueError):
        fiesta_amd.path_cost_model(batch(boxed_sphere), W, off, step, float("inf"))


def test_path_cost_model_on_random_paths():
    import fiesta_amd
    rng = np.random.RandomState(4)
    lens = rng.randint(0, 9, 60)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    w = 1.0 + rng.randn(off[-1], 3) * rng.choice([0.05, 0.6, 3.0], (off[-1], 1))
    dup = np.nonzero(rng.rand(len(w)) < 0.1)[0]
    dup = dup[dup > 0]
    w[dup] = w[dup - 1]
    for step, margin in ((0.05, 0.8), (0.37, 3.0), (1.0, 0.1)):
        got = fiesta_amd.path_cost_model(batch(boxed_sphere), w, off, step, margin)
        assert_close(got, cost_loop(boxed_sphere, w, off, step, margin), got, f"random step {step}")


def test_the_gradient_is_the_derivative_of_the_cost():
    """central differences of the model's cost at eps = 1e-6 in every waypoint coordinate against its grad, to 1e-5 of the largest
    gradient component (truncation O(eps^2), round-off ~ 2^-52 * cost / eps ~ 1e-10 * cost)"""
    import fiesta_amd
    step, margin, eps = 0.07, 1.5, 1e-6
    off = np.arange(0, 25, 6)
    for seed in range(100):   # the first draw with no segment length within 1e-3 of a multiple of the step
        rng = np.random.RandomState(seed)
        w = np.array(CENTRE) + rng.randn(24, 3) * 0.8
        L = np.linalg.norm(np.diff(w.reshape(4, 6, 3), axis=1), axis=2).reshape(-1)
        frac = L / step - np.floor(L / step)
        if (np.minimum(frac, 1 - frac) * step > 1e-3).all():
            break
    assert (np.minimum(frac, 1 - frac) * step > 1e-3).all()             # S must not change under +-eps
    query = batch(sphere)
    base = fiesta_amd.path_cost_model(query, w, off, step, margin)
    assert (base["n_below"] > 0.5 * base["n_samples"]).all()             # most samples are penalised
    fd = np.zeros_like(w)
    for i in range(len(w)):
        p = i // 6
        for c in range(3):
            hi, lo = w.copy(), w.copy()
            hi[i, c] += eps
            lo[i, c] -= eps
            ch = fiesta_amd.path_cost_model(query, hi[6 * p:6 * p + 6], [0, 6], step, margin)
            cl = fiesta_amd.path_cost_model(query, lo[6 * p:6 * p + 6], [0, 6], step, margin)
            assert ch["n_samples"][0] == cl["n_samples"][0] == base["n_samples"][p]
            fd[i, c] = (ch["cost"][0] - cl["cost"][0]) / (2 * eps)
    scale = np.abs(base["grad"]).max()
    worst = np.abs(fd - base["grad"]).max() / scale
    print(f"central differences: worst deviation {worst:.3g} of the largest gradient component {scale:.3g}")
    assert scale > 0.1 and worst <= 1e-5


def test_path_cost_result_struct_matches_header():
    from fiesta_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct fiesta_hip_path_cost_result \{(.*?)\} fiesta_hip_path_cost_result;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [d.split(None, 1)[1].lstrip("*").strip() for d in decls]
    assert names == [f[0] for f in _lib.PathCostResult._fields_] == ["cost", "grad", "length", "n_below", "n_samples"]
    assert all(d.split(None, 1)[1].startswith("*") for d in decls)       # five pointers
    import fiesta_amd.esdf_map as em
    assert [f[0] for f in em.PATH_COST_FIELDS] == names
    types = [d.split(None, 1)[0] for d in decls]
    assert ["int64_t" if f[1] == np.int64 else "double" for f in em.PATH_COST_FIELDS] == types


def test_cost_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_cost_" in k}
    for kernel in ("k_cost_eval", "k_cost_segments", "k_cost_finish"):
        assert any(kernel in k for k in res), (kernel, sorted(res))
    assert sum("k_cost_eval" in k for k in res) == 2                     # the dense and the hash-block evaluator
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)


def test_the_library_exports_the_cost_calls_under_version_101():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    assert hasattr(lib, "fiesta_hip_path_cost") and hasattr(lib, "fiesta_hip_path_cost_dev")
