"""Path timing on the device (fiesta_hip_path_timing[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/timing_kernels.hpp).

The model is fiesta_amd.path_timing_model over GetDistWithGradTrilinear on the same map (the header's rule in numpy;
tests/test_path_timing_rule.py checks it against a literal loop, the serial recurrence and closed forms).  Everything but `duration`
and `time` is compared bit for bit (floats as int64 views); those two within (n + 16) * 2^-52 * a of the model's (n, abs), NaN
exactly where the model has NaN: every dt is bit-identical, only the order of the sums differs.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_path_cost import hash_map_scene
from test_gpu_path_queries import dense_map, wall_map
from test_gpu_refine import flagged_paths

pytestmark = pytest.mark.gpu
# SAMPLES per path.  0 .. 4: no, one, a few samples; 63 .. 66: a wave's lanes; 255 .. 258: the split between a wave and a work-group
# per path (kTimingWaveMax = 256) and the work-group's lanes; 4095, 4096: the cap; 4097: TOO_LONG
COUNTS = [0, 1, 2, 3, 4, 63, 64, 65, 66, 255, 256, 257, 258, 4095, 4096, 4097]
STEP = 0.001
PAR = dict(step=STEP, margin=0.3, v_max=1.2, v_min=0.05, a_max=1.5, corner_dev=0.01, v_start=0.0, v_end=0.0)
SENTINEL = -7
EXACT_F, EXACT_I, SUMS = ("length", "min_speed", "speed"), ("n_samples", "n_below", "min_index", "status"), ("duration", "time")
DIRS = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], float)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def seg_samples(d):
    return max(1, int(np.ceil(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / STEP)))


def rough_walk(n, start, rng):
    """n samples at STEP: moves along the 26 lattice directions (45 and 90 degree bends, one move in six a reversal), `scale` lattice
    steps long, and a last axis move that takes exactly what is left"""
    if n == 0:
        return np.zeros((0, 3))
    pts, left, scale, prev = [np.asarray(start, float)], n - 1, max(1, n // 250), None
    while left > 0:
        d = -prev if prev is not None and rng.rand() < 1 / 6 else DIRS[rng.randint(26)]
        move = d * (STEP * scale * 0.9)
        if seg_samples(move) > left:
            move = np.zeros(3)
            move[rng.randint(3)] = (left - 0.5) * STEP * rng.choice([-1, 1])
        left -= seg_samples(move)
        pts.append(pts[-1] + move)
        prev = d
    return np.array(pts)


def line(n, start, direction, rng):
    """n samples at STEP on a nearly straight line of up to eight segments"""
    if n == 0:
        return np.zeros((0, 3))
    k = min(n - 1, 8)
    S = np.full(k, (n - 1) // max(k, 1))
    S[:(n - 1) - int(S.sum())] += 1
    u = np.asarray(direction, float) / np.linalg.norm(direction)
    pts = [np.asarray(start, float)]
    for s in S:
        pts.append(pts[-1] + u * ((s - 0.5) * STEP) + rng.randn(3) * 1e-5)
    return np.array(pts)


def make_batch(lo, hi, seed):
    """one path per entry of COUNTS, twice (a rough walk and a nearly straight line), then: 1025 waypoints (TOO_LONG), a NaN waypoint
    (INVALID), a path with zero-length segments, a path outside the box [lo, hi] (a dense map's outside) and one that starts inside and
    walks out of it; shuffled"""
    import fiesta_amd
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    paths, want = [], []
    for n in COUNTS:
        paths.append(rough_walk(n, lo + (0.2 + 0.6 * rng.rand(3)) * (hi - lo), rng))
        a, b = lo + (0.08 + 0.1 * rng.rand(3)) * (hi - lo), lo + (0.82 + 0.1 * rng.rand(3)) * (hi - lo)
        paths.append(line(n, a if n > 1000 else lo + (0.2 + 0.6 * rng.rand(3)) * (hi - lo), b - a if n > 1000 else rng.randn(3), rng))
        want += [n, n]
    start = lo + 0.5 * (hi - lo)
    paths.append(start + np.cumsum(rng.randn(1025, 3) * 2e-4, axis=0))                    # 1025 waypoints of one sample each
    nanp = rough_walk(40, start, rng)
    nanp[3, 1] = np.nan
    paths.append(nanp)
    zl = rough_walk(30, start + 0.1, rng)
    paths.append(np.concatenate([zl[:1], zl[:5], zl[4:5], zl[4:5], zl[4:], zl[-1:]]))      # zero-length segments, also at both ends
    paths.append(line(120, hi + 3.0 * (hi - lo), rng.randn(3), rng))
    paths.append(line(900, hi - 0.1 * (hi - lo), [1.0, 0.7, 0.4], rng))
    special = {}
    order = rng.permutation(len(paths))
    for name, k in (("waypoints", -5), ("nan", -4), ("zero", -3), ("outside", -2), ("leaving", -1)):
        special[name] = int(np.nonzero(order == len(paths) + k)[0][0])
    counts = np.array(want + [-1] * 5)[order]
    paths = [paths[i] for i in order]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    w = np.concatenate(paths)
    _, ns = fiesta_amd.path_samples(w, off, STEP)
    assert (ns[counts >= 0] == counts[counts >= 0]).all(), (ns, counts)
    return w, off, special, counts


def expected(m, w, off, par, device_offsets=False):
    """the model's answer for the batch; with device_offsets the paths the offset rule flags are INVALID, the others are timed over
    the ranges they name, and every row outside them is NaN"""
    import fiesta_amd
    n_paths = len(off) - 1
    flagged = flagged_paths(off, len(w)) if device_offsets else np.zeros(n_paths, bool)
    keep = np.nonzero(~flagged)[0]
    rows = np.concatenate([np.arange(off[p], off[p + 1]) for p in keep] + [np.zeros(0, np.int64)]).astype(np.int64)
    sub_off = np.concatenate([[0], np.cumsum(off[keep + 1] - off[keep])]).astype(np.int64)
    sub = fiesta_amd.path_timing_model(m.GetDistWithGradTrilinear, w[rows], sub_off, **par)
    nan = np.nan
    out = {"duration": np.full(n_paths, nan), "length": np.full(n_paths, nan), "n_samples": np.full(n_paths, -1, np.int64),
           "n_below": np.full(n_paths, -1, np.int64), "min_speed": np.full(n_paths, nan), "min_index": np.full(n_paths, -1, np.int64),
           "status": np.ones(n_paths, np.int32), "time": np.full(len(w), nan), "speed": np.full(len(w), nan),
           "duration_n": np.zeros(n_paths, np.int64), "duration_abs": np.zeros(n_paths), "time_n": np.zeros(len(w), np.int64),
           "time_abs": np.zeros(len(w))}
    for k in ("duration", "length", "n_samples", "n_below", "min_speed", "min_index", "status", "duration_n", "duration_abs"):
        out[k][keep] = sub[k]
    for k in ("time", "speed", "time_n", "time_abs"):
        out[k][rows] = sub[k]
    return out


def assert_equals_model(got, want, what, skip=()):
    for k in EXACT_F:
        if k in skip:
            continue
        g, x = np.asarray(got[k], np.float64), want[k]
        assert np.array_equal(np.isnan(g), np.isnan(x)), f"{what} {k}: NaN pattern differs at {np.nonzero(np.isnan(g) != np.isnan(x))[0][:5]}"
        bad = np.nonzero(~np.isnan(x) & (bits(g) != bits(x)))[0]
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries differ, first {bad[:3]}: {g[bad[:3]]!r} vs {x[bad[:3]]!r}"
    for k in EXACT_I:
        if k in skip:
            continue
        bad = np.nonzero(np.asarray(got[k]).astype(np.int64) != want[k])[0]
        assert len(bad) == 0, f"{what} {k}: paths {bad[:5]} differ: {np.asarray(got[k])[bad[:5]]} vs {want[k][bad[:5]]}"
    for k in SUMS:
        if k in skip:
            continue
        g, x = np.asarray(got[k], np.float64), want[k]
        assert np.array_equal(np.isnan(g), np.isnan(x)), f"{what} {k}: NaN pattern differs at {np.nonzero(np.isnan(g) != np.isnan(x))[0][:5]}"
        lim = (want[k + "_n"] + 16.0) * 2.0 ** -52 * want[k + "_abs"]
        err = np.where(np.isnan(x), 0.0, np.abs(g - x))
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{what}: {k}, worst error / bound {np.nanmax(np.where(lim > 0, err / lim, 0.0), initial=0.0):.3g}")
        bad = np.nonzero(err > lim)[0]
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries beyond the bound, first {bad[:3]}: {g[bad[:3]]!r} vs {x[bad[:3]]!r}"


def params_struct(par):
    from fiesta_amd._lib import TimingParams
    from fiesta_amd.esdf_map import TIMING_PARAMS
    return TimingParams(*[float(par[k]) for k in TIMING_PARAMS])


def host_call(m, w, off, par, extra_rows=0, only=None):
    """fiesta_hip_path_timing through ctypes, every output pre-filled with the sentinel (extra_rows: sentinel rows past n_waypoints;
    only: the one output that is not NULL)"""
    from fiesta_amd._lib import TimingResult, check
    from fiesta_amd.esdf_map import TIMING_FIELDS
    w = np.ascontiguousarray(w, np.float64)
    n = len(off) - 1
    out = {name: np.full((n if per == "path" else len(w)) + extra_rows, SENTINEL, dt) for name, dt, per, _ in TIMING_FIELDS}
    res = TimingResult(*[out[name].ctypes.data if only in (None, name) else None for name, _, _, _ in TIMING_FIELDS])
    p = params_struct(par)
    check(m._lib.fiesta_hip_path_timing(m._h, w.ctypes.data_as(C.c_void_p), len(w), off.ctypes.data_as(C.c_void_p), n, C.byref(p), C.byref(res)))
    return out


def device_call(m, w, off, par, extra_rows=0, only=None):
    """fiesta_hip_path_timing_dev on torch tensors; every output pre-filled with the sentinel"""
    import torch
    from fiesta_amd.esdf_map import TIMING_FIELDS
    dev = torch.device("cuda", 0)
    tdt = {np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32}
    wt, ot = torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(dev)
    outs = {name: torch.full((((len(off) - 1) if per == "path" else len(w)) + extra_rows,), SENTINEL, dtype=tdt[dt], device=dev)
            for name, dt, per, _ in TIMING_FIELDS}
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the copies and fills above must have landed)
    m.PathTimingDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, out={k: v.data_ptr() for k, v in outs.items() if only in (None, k)}, **par)
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def same_bits(a, b, keys=EXACT_F + EXACT_I + SUMS):
    for k in keys:
        x, y = (bits(a[k]), bits(b[k])) if np.asarray(a[k]).dtype == np.float64 else (np.asarray(a[k]), np.asarray(b[k]))
        nan = np.isnan(a[k]) & np.isnan(b[k]) if np.asarray(a[k]).dtype == np.float64 else np.zeros(len(x), bool)
        assert ((x == y) | nan).all(), (k, np.nonzero((x != y) & ~nan)[0][:5])


@pytest.fixture(scope="module", params=["dense", "hash"])
def store(request, hip_lib):
    if request.param == "dense":
        m, _ = dense_map(48, obstacles=160, seed=3, hidden_blocks=4)      # (four 16^3 blocks never observed: +10000 at their corners)
        lo, hi = (0.0, 0.0, 0.0), (4.8, 4.8, 4.8)
    else:
        m, _ = hash_map_scene()
        lo, hi = (-2.0, -2.0, -1.0), (4.0, 3.0, 2.0)
    w, off, special, counts = make_batch(lo, hi, 5)
    want = expected(m, w, off, PAR)                                       # the reference, computed once and left unchanged
    yield m, w, off, special, counts, want, request.param
    m.close()


def test_the_sample_count_boundaries_equal_the_model(store):
    m, w, off, special, counts, want, kind = store
    st = want["status"]
    assert (st[counts == 4097] == 2).all() and st[special["waypoints"]] == 2 and st[special["nan"]] == 1 and (st != 0).sum() == 4
    assert st[special["zero"]] == 0 and want["n_samples"][special["zero"]] == 30 + 5
    assert (want["n_samples"][counts >= 0][counts[counts >= 0] <= 4096] == counts[counts >= 0][counts[counts >= 0] <= 4096]).all()
    ok = st == 0
    assert np.isnan(want["time"]).sum() == int(np.diff(off)[~ok].sum()) and np.isnan(want["duration"]).sum() == 4
    if kind == "dense":                                                   # -1 outside the array: below any margin
        assert want["n_below"][special["outside"]] == 120 and 0 < want["n_below"][special["leaving"]] < 900
    assert (want["n_below"][ok] > 0).any() and (want["n_below"][ok] == 0).sum() >= 5
    assert (want["min_speed"][ok & (counts > 1)] == 0).all()             # every path starts at rest
    assert np.isinf(want["min_speed"][counts == 0]).all() and (want["min_index"][counts == 0] == -1).all()
    for call in (host_call, device_call):
        got = call(m, w, off, PAR, extra_rows=3)
        for k in ("time", "speed"):
            assert (got[k][len(w):] == SENTINEL).all(), (call.__name__, k)   # rows past n_waypoints are not touched
            got[k] = got[k][:len(w)]
        for k in EXACT_F[:2] + EXACT_I + ("duration",):
            assert (got[k][len(off) - 1:] == SENTINEL).all(), (call.__name__, k)
            got[k] = got[k][:len(off) - 1]
        assert_equals_model(got, want, call.__name__)
    cls = m.PathTiming(w, off, **PAR)
    same_bits(cls, host_call(m, w, off, PAR))


def test_end_speeds_and_no_corner_rule(store):
    m, w, off, _, counts, base, _ = store
    for change in (dict(v_start=0.4, v_end=0.25), dict(corner_dev=np.inf), dict(v_start=5.0, v_end=5.0, corner_dev=np.inf, margin=0.0)):
        par = dict(PAR, **change)
        want = expected(m, w, off, par)
        ok = (want["status"] == 0) & (counts > 64)
        assert (bits(want["duration"][ok]) != bits(base["duration"][ok])).any(), change
        assert_equals_model(host_call(m, w, off, par), want, f"host {change}")
        assert_equals_model(device_call(m, w, off, par), want, f"device {change}")
    assert (want["min_speed"][ok] > 0).all()                              # (the last one: nothing forces a stop)


def test_device_offsets_and_launch_independence(store):
    m, w, off, _, _, want, _ = store
    good = device_call(m, w, off, PAR)
    # broken device offsets: a swapped pair, entries out of range, a shifted boundary; the flagged paths are INVALID, the others exact
    bad = off.copy()
    bad[5], bad[6] = off[6], off[5]
    bad[20] = len(w) + 5
    bad[30] = -3
    bad[12] = off[12] + 2
    flagged = flagged_paths(bad, len(w))
    assert 3 <= flagged.sum() <= 12
    exp = expected(m, w, bad, PAR, device_offsets=True)
    got = device_call(m, w, bad, PAR)
    assert_equals_model(got, exp, "device, broken offsets")
    assert (got["status"][flagged] == 1).all()
    # the same batch split into two calls: the same bits, duration and time included (their order follows the sample count alone)
    n = len(off) - 1
    cut = n // 2
    a = device_call(m, w[:off[cut]], off[:cut + 1], PAR)
    b = device_call(m, w[off[cut]:], off[cut:] - off[cut], PAR)
    both = {k: np.concatenate([a[k], b[k]]) for k in good}
    same_bits(both, good)
    perm = np.random.RandomState(2).permutation(n)
    rows = np.concatenate([np.arange(off[p], off[p + 1]) for p in perm]).astype(np.int64)
    off2 = np.concatenate([[0], np.cumsum(np.diff(off)[perm])]).astype(np.int64)
    other = host_call(m, w[rows], off2, PAR)
    same_bits(other, {k: (good[k][perm] if len(good[k]) == n else good[k][rows]) for k in good})
    same_bits(device_call(m, w, off, PAR), good)                          # and the same call again


def test_optional_outputs_and_argument_errors(hip_lib):
    from fiesta_amd._lib import TimingResult
    from fiesta_amd.esdf_map import TIMING_FIELDS
    m = wall_map(32, 0.1, wall_y=10)
    rng = np.random.RandomState(7)
    w = np.concatenate([rough_walk(300, [1.6, 1.3, 1.6], rng), line(70, [0.5, 2.5, 1.0], [1, 0.1, 0.3], rng), np.zeros((0, 3))])
    off = np.array([0, len(w) - 9, len(w), len(w)], np.int64)
    full = host_call(m, w, off, PAR)
    assert (full["status"] == 0).all() and full["n_samples"].tolist() == [300, 70, 0]
    for name, _, _, _ in TIMING_FIELDS:                                   # every output alone: written as in the full call, the others untouched
        for call in (host_call, device_call):
            one = call(m, w, off, PAR, only=name)
            same_bits(one, full, keys=(name,))
            assert all((one[k] == SENTINEL).all() for k in one if k != name), (call.__name__, name)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    dur = np.full(3, -7.0)
    res = TimingResult(dur.ctypes.data, *[None] * 8)
    lib, h = m._lib, m._h
    assert lib.fiesta_hip_path_timing(h, vp(w), 0, vp(np.zeros(1, np.int64)), 0, C.byref(params_struct(PAR)), C.byref(res)) == 0
    assert (dur == -7.0).all()                                            # n_paths = 0 does nothing
    nan, inf = np.nan, np.inf
    wrong = [dict(step=0.0), dict(step=nan), dict(step=inf), dict(step=-1.0), dict(margin=-0.1), dict(margin=nan), dict(margin=inf),
             dict(v_max=0.0), dict(v_max=inf), dict(v_max=nan), dict(v_min=0.0), dict(v_min=1.3), dict(v_min=nan), dict(a_max=0.0),
             dict(a_max=inf), dict(a_max=nan), dict(corner_dev=0.0), dict(corner_dev=-1.0), dict(corner_dev=nan), dict(v_start=-0.1),
             dict(v_start=inf), dict(v_start=nan), dict(v_end=-0.1), dict(v_end=inf), dict(v_end=nan)]
    p = params_struct(PAR)
    cases = [(vp(w), len(w), vp(off), 3, C.byref(params_struct(dict(PAR, **c))), C.byref(res)) for c in wrong]
    cases += [(None, len(w), vp(off), 3, C.byref(p), C.byref(res)), (vp(w), len(w), None, 3, C.byref(p), C.byref(res)),
              (vp(w), len(w), vp(off), 3, None, C.byref(res)), (vp(w), len(w), vp(off), 3, C.byref(p), None),
              (vp(w), -1, vp(off), 3, C.byref(p), C.byref(res)), (vp(w), len(w), vp(off), -1, C.byref(p), C.byref(res))]
    for o in ([1, 5, len(w), len(w)], [0, 5, 4, len(w)], [0, 5, len(w), len(w) - 1], [0, 5, len(w), len(w) + 1]):
        cases.append((vp(w), len(w), vp(np.array(o, np.int64)), 3, C.byref(p), C.byref(res)))
    for fn in (lib.fiesta_hip_path_timing, lib.fiesta_hip_path_timing_dev):
        for k, args in enumerate(cases):
            if fn is lib.fiesta_hip_path_timing_dev and k >= len(cases) - 4:
                continue                                                  # (device offsets are no whole-call error)
            assert fn(h, *args) == 1, (fn.__name__, k)                    # FIESTA_HIP_ERR_INVALID
        assert (dur == -7.0).all()
        assert m.GetDistWithGradTrilinear(w[:1])[0][0] > 0                # the map stays usable
    same_bits(host_call(m, w, off, PAR), full)
    m.close()


def test_chain_from_reach_paths_and_time_against_length(hip_lib):
    """ReachPathsDevice -> PathTimingDevice with nothing in between equals the host chain; and along a wall the nearest target in
    metres is not the nearest in seconds"""
    import torch

    import fiesta_amd
    m = wall_map(32, 0.1, wall_y=10)
    par = dict(step=0.1, margin=0.15, v_max=2.0, v_min=0.1, a_max=2.0, corner_dev=0.05)
    targets = np.array([(x, y, 16) for x in range(4, 30, 3) for y in range(12, 31, 3)], np.int32)
    m.ReachField([(5, 12, 16)], want_cost=False)
    for shortcut in (False, True):
        paths = m.ReachPaths(targets, shortcut=shortcut)
        w, off = paths["waypoints_pos"], paths["offsets"]
        assert (np.diff(off) >= 2).all()
        host = m.PathTiming(w, off, **par)
        assert (host["status"] == 0).all()
        model = fiesta_amd.path_timing_model(m.GetDistWithGradTrilinear, w, off, **par)
        assert_equals_model(host, model, f"host chain, shortcut {shortcut}")
        # the model alone: a pair of targets ordered differently by duration than by length (one path hugs the wall, one is free)
        L, T = model["length"], model["duration"]
        pairs = np.argwhere((L[:, None] < L[None, :]) & (T[:, None] > T[None, :]))
        assert len(pairs) >= 1, (L, T)
        i, j = pairs[np.argmax((T[:, None] - T[None, :])[pairs[:, 0], pairs[:, 1]])]
        print(f"shortcut {shortcut}: to {targets[i]} {L[i]:.2f} m in {T[i]:.2f} s, to {targets[j]} {L[j]:.2f} m in {T[j]:.2f} s")
        assert targets[i][1] < targets[j][1]                              # the slower, shorter one runs nearer the wall
        dev = torch.device("cuda", 0)
        tt = torch.from_numpy(targets).to(dev)
        offt = torch.zeros(len(targets) + 1, dtype=torch.int64, device=dev)
        post = torch.zeros((len(w), 3), dtype=torch.float64, device=dev)
        outs = {"duration": torch.zeros(len(targets), dtype=torch.float64, device=dev), "length": torch.zeros(len(targets), dtype=torch.float64, device=dev),
                "status": torch.full((len(targets),), -1, dtype=torch.int32, device=dev), "time": torch.zeros(len(w), dtype=torch.float64, device=dev),
                "speed": torch.zeros(len(w), dtype=torch.float64, device=dev)}
        torch.cuda.synchronize()
        m.ReachPathsDevice(tt.data_ptr(), len(targets), offt.data_ptr(), shortcut=shortcut, capacity=len(w), waypoints_pos_dev_ptr=post.data_ptr())
        m.PathTimingDevice(post.data_ptr(), len(w), offt.data_ptr(), len(targets), out={k: v.data_ptr() for k, v in outs.items()}, **par)
        m.synchronize()
        same_bits({k: v.cpu().numpy() for k, v in outs.items()}, host, keys=tuple(outs))
    m.close()
