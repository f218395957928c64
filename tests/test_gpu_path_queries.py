"""Batched path clearance (fiesta_hip_path_clearance[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/path_kernels.hpp).

The model is the point route a planner runs today: positions from fiesta_amd.path_samples (the header's sample rule in numpy),
values and gradients from GetDistWithGradTrilinear on the same map, the minimum / its first index / the first index below the
margin reduced in numpy.  Every check is exact (f64 bits, indices) unless it says otherwise.
"""
import ctypes as C
import json
import os
import subprocess
import time

import numpy as np
import pytest

from scenarios import P_DEFAULT, Both, all_voxels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = (0.0, 0.3, 1e9, -2.0)
FLOATS = ("min_dist", "min_pos", "min_grad", "first_below_pos")


def model(m, w, off, step, margin):
    import fiesta_amd
    pos, ns = fiesta_amd.path_samples(w, off, step)
    d, g = m.GetDistWithGradTrilinear(pos) if len(pos) else (np.zeros(0), np.zeros((0, 3)))
    n = len(ns)
    out = {"min_dist": np.full(n, np.inf), "min_index": np.full(n, -1, np.int64), "min_pos": np.full((n, 3), np.nan),
           "min_grad": np.zeros((n, 3)), "first_below": np.full(n, -1, np.int64), "first_below_pos": np.full((n, 3), np.nan),
           "n_samples": ns.copy()}
    at = 0
    for p, k in enumerate(ns):
        if k < 0:
            out["min_dist"][p] = np.nan
            continue
        if k == 0:
            continue
        v = d[at:at + k]
        i = int(np.argmin(v))
        out["min_dist"][p], out["min_index"][p], out["min_pos"][p], out["min_grad"][p] = v[i], i, pos[at + i], g[at + i]
        below = np.nonzero(v < margin)[0]
        if len(below):
            out["first_below"][p], out["first_below_pos"][p] = below[0], pos[at + below[0]]
        at += k
    return out


def assert_same(got, want, what=""):
    for k, v in want.items():
        a, b = np.asarray(got[k]), np.asarray(v)
        if k in FLOATS:
            bad = np.nonzero((a.view(np.int64) != b.view(np.int64)).reshape(len(a), -1).any(1))[0]
        else:
            bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, f"{what} {k}: {len(bad)} paths differ, first {bad[:5]}: got {a[bad[:3]]} want {b[bad[:3]]}"


def dense_map(n, res=0.1, origin=(0.0, 0.0, 0.0), obstacles=200, seed=1, hidden_blocks=0, engine=None):
    """a dense map, observed everywhere (or but for `hidden_blocks` random 16^3 blocks), with random obstacle voxels"""
    import fiesta_amd
    shape = (n, n, n) if np.isscalar(n) else tuple(n)
    m = fiesta_amd.ESDFMap(origin, res, tuple(s * res for s in shape), update_engine=engine)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    rng = np.random.RandomState(seed)
    V = all_voxels(shape)
    if hidden_blocks:
        blk = V // 16
        nb = np.array(shape) // 16
        hide = rng.choice(int(np.prod(nb)), hidden_blocks, replace=False)
        keep = ~np.isin((blk[:, 0] * nb[1] + blk[:, 1]) * nb[2] + blk[:, 2], hide)
        V = V[keep]
    m.SetOccupancy(V, 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    S = V[rng.choice(len(V), obstacles, replace=False)]
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m, S


def make_paths(rng, lo, hi, res, n_paths=120, long_path=True):
    """random walks of 1 ... 200 waypoints (some leave the map), paths on voxel-centre planes and on faces, empty paths,
    single waypoints, and one path of ~10^5 samples at the smallest step"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    span = hi - lo
    paths = []
    for k in range(n_paths):
        nw = int(rng.choice([1, 2, 3, 7, 20, 64, 200]))
        start = lo + rng.rand(3) * span
        steps = rng.randn(nw - 1, 3) * rng.choice([0.3, 2.0, 6.0]) * res
        pts = np.concatenate([start[None], start + np.cumsum(steps, 0)]) if nw > 1 else start[None]
        if k % 11 == 0:   # out of the map and back
            pts = pts + (span * 0.6) * np.sin(np.arange(nw) / 5.0)[:, None]
        paths.append(pts)
    for k in range(12):   # exactly on voxel-centre planes / on voxel faces, along each axis
        ax = k % 3
        c = lo + (rng.randint(1, 10, 3) + (0.5 if k < 6 else 0.0)) * res
        a, b = c.copy(), c.copy()
        a[ax], b[ax] = lo[ax] + 0.5 * res, hi[ax] - 0.5 * res
        paths.append(np.stack([a, b]))
    paths += [np.zeros((0, 3)), np.zeros((0, 3)), (lo + span / 3)[None], (lo + span / 2)[None]]
    if long_path:
        paths.append(lo + 0.1 * span + rng.rand(2000, 3) * 0.8 * span)
    rng.shuffle(paths)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return np.concatenate(paths).reshape(-1, 3), off


@pytest.mark.parametrize("scene", ["scatter64", "partial64", "ragged32"])
def test_path_clearance_equals_the_point_route(hip_lib, scene):
    if scene == "scatter64":
        m, _ = dense_map(64)
        lo, res = np.zeros(3), 0.1
        hi = lo + 6.4
    elif scene == "partial64":
        m, _ = dense_map(64, obstacles=300, seed=2, hidden_blocks=12)
        lo, res = np.zeros(3), 0.1
        hi = lo + 6.4
    else:   # the grid of test_queries_bit_exact: res 0.2, origin (-3.2, -3.2, 0)
        m, _ = dense_map(32, res=0.2, origin=(-3.2, -3.2, 0.0), obstacles=120, seed=11)
        lo, res = np.array([-3.2, -3.2, 0.0]), 0.2
        hi = lo + 6.4
    rng = np.random.RandomState(len(scene))
    w, off = make_paths(rng, lo, hi, res)
    saw_long = False
    for step in (0.25 * res, res, 3.7 * res):
        for margin in MARGINS:
            want = model(m, w, off, step, margin)
            got = m.PathClearance(w, off, step, margin)
            assert_same(got, want, f"{scene} step {step} margin {margin}")
            saw_long |= bool(want["n_samples"].max() >= 100_000)
            if margin == 1e9:
                assert np.all(got["first_below"][got["n_samples"] > 0] == 0)
            if margin == -2.0:
                assert np.all(got["first_below"] == -1)
    assert saw_long
    m.close()


def test_sample_counts_pin_sqrt_division_and_ceil(hip_lib):
    """10^5 random single-segment paths: n_samples is numpy's (the device's sqrt, division and ceil), and the 2^24 limit"""
    import fiesta_amd
    m, _ = dense_map(32, obstacles=20)
    rng = np.random.RandomState(9)
    n = 100_000
    a = rng.rand(n, 3) * 3.2
    b = a + rng.randn(n, 3) * rng.choice([0.0, 1e-3, 0.05, 0.3, 2.0], (n, 1))
    w = np.stack([a, b], 1).reshape(-1, 3)
    off = np.arange(0, 2 * n + 1, 2)
    for step in (0.01, 0.0731, 0.1):
        _, want = fiesta_amd.path_samples(w, off, step)
        got = m.PathClearance(w, off, step)["n_samples"]
        assert np.array_equal(got, want), step
    # L / step = 2^24 exactly is valid (2^24 + 1 samples, 16 385 pieces), one ulp more is not
    lim = 2.0 ** 24
    got = m.PathClearance([[0, 0, 0], [lim, 0, 0], [0, 0, 0], [np.nextafter(lim, np.inf), 0, 0]], [0, 2, 4], 1.0)
    assert list(got["n_samples"]) == [2 ** 24 + 1, -1], got["n_samples"]
    assert got["min_dist"][0] == -1.0 and got["min_index"][0] == 4 and got["first_below"][0] == 4   # x = 4 m: off the 3.2 m map
    m.close()


def test_hash_block_map(hip_lib):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, reserve_size=100000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((-20, -20, -10), (40, 30, 20), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    rng = np.random.RandomState(4)
    S = np.stack([rng.randint(-20, 41, 150), rng.randint(-20, 31, 150), rng.randint(-10, 21, 150)], 1).astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    # inside the observed box, and out through unallocated blocks (corners read +10000)
    w, off = make_paths(rng, (-1.5, -1.5, -0.5), (3.5, 2.5, 1.5), 0.1, n_paths=80)
    for step in (0.025, 0.1, 0.37):
        for margin in MARGINS:
            want = model(m, w, off, step, margin)
            assert_same(m.PathClearance(w, off, step, margin), want, f"hash step {step} margin {margin}")
    assert (want["min_dist"] < 10000).any()
    far_w = [[10.0, 10.0, 10.0], [12.0, 10.0, 10.0]]                     # no page anywhere near: every corner reads +10000
    far = m.PathClearance(far_w, [0, 2], 0.1, 0.0)
    assert far["min_dist"][0] == 10000.0
    assert_same(far, model(m, far_w, [0, 2], 0.1, 0.0), "hash, unallocated")
    m.close()


def test_host_and_device_variants_agree(hip_lib):
    import torch
    m, _ = dense_map(64, obstacles=250, seed=5)
    rng = np.random.RandomState(6)
    w, off = make_paths(rng, np.zeros(3), np.full(3, 6.4), 0.1, n_paths=60)
    dev = torch.device("cuda", 0)
    from fiesta_amd.esdf_map import PATH_FIELDS
    for step, margin in ((0.05, 0.3), (0.37, 0.0)):
        host = m.PathClearance(w, off, step, margin)
        wt = torch.from_numpy(w).to(dev)
        ot = torch.from_numpy(off).to(dev)
        outs = {name: torch.full((len(off) - 1,) + shape, -7, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
                for name, dt, shape in PATH_FIELDS}
        torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the fills above must have landed)
        m.PathClearanceDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, step, margin,
                              {k: v.data_ptr() for k, v in outs.items()})
        m.synchronize()
        assert_same({k: v.cpu().numpy() for k, v in outs.items()}, host, "device vs host")
        # only some outputs requested: the others are not written
        md = torch.full((len(off) - 1,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        m.PathClearanceDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, step, margin, {"min_dist": md.data_ptr()})
        m.synchronize()
        assert np.array_equal(md.cpu().numpy().view(np.int64), host["min_dist"].view(np.int64))
    # below kHostPathSamples (256) the host variant answers from the brick cache: same bits, bricks fetched, nothing else
    small_w = np.array([[1.0, 1.0, 1.0], [1.5, 1.2, 1.1], [2.0, 2.2, 1.3], [3.0, 3.0, 3.0]])
    grew = []
    for off_s, step in (([0, 3, 4], 0.05), ([0, 4], 0.02)):   # 36 samples / 193 samples
        off_s = np.array(off_s)
        _, ns = __import__("fiesta_amd").path_samples(small_w[:off_s[-1]], off_s, step)
        assert 0 < ns.sum() <= 256
        before = m.host_cache_fetches
        got = m.PathClearance(small_w[:off_s[-1]], off_s, step, 0.4)
        grew.append(m.host_cache_fetches > before)
        assert_same(got, model(m, small_w[:off_s[-1]], off_s, step, 0.4), "host cache")
        wt = torch.from_numpy(np.ascontiguousarray(small_w[:off_s[-1]])).to(dev)
        ot = torch.from_numpy(off_s.astype(np.int64)).to(dev)
        outs = {name: torch.empty((len(off_s) - 1,) + shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
                for name, dt, shape in PATH_FIELDS}
        m.PathClearanceDevice(wt.data_ptr(), off_s[-1], ot.data_ptr(), len(off_s) - 1, step, 0.4, {k: v.data_ptr() for k, v in outs.items()})
        m.synchronize()
        assert_same({k: v.cpu().numpy() for k, v in outs.items()}, got, "small batch: device vs host cache")
    assert grew[0]
    # just above: the device route (no brick fetched)
    big = np.array([[0.5, 0.5, 0.5], [5.5, 5.5, 5.5]])
    before = m.host_cache_fetches
    got = m.PathClearance(big, [0, 2], 0.02, 0.0)
    assert got["n_samples"][0] > 256 and m.host_cache_fetches == before
    assert_same(got, model(m, big, [0, 2], 0.02, 0.0), "just above the host limit")
    m.close()


def test_against_the_reference(hip_lib, oracle_libs, best_oracle_kind):
    """a 32^3 GPU / oracle pair as test_queries_bit_exact builds it: interior paths (the reference reads out of bounds at the +1
    faces); the GPU min_dist is the minimum of the oracle's GetDistWithGradTrilinear over the same samples"""
    import fiesta_amd
    n, res, origin = 32, 0.2, (-3.2, -3.2, 0.0)
    gpu = fiesta_amd.ESDFMap(origin, res, (n * res,) * 3)
    cpu = oracle_libs.OracleMap(origin, res, (n * res,) * 3, kind=best_oracle_kind)
    b = Both(gpu, cpu)
    b.params()
    gpu.SetOriginalRange()
    cpu.SetOriginalRange()
    b.observe(all_voxels(n), 0)
    b.fuse()
    b.esdf()
    rng = np.random.RandomState(11)
    b.make_occupied(rng.randint(0, n, (120, 3)).astype(np.int32))
    b.esdf()
    lo = np.array(origin)
    paths = [lo + 0.2 + rng.rand(int(rng.randint(1, 30)), 3) * (n * res - 0.6) for _ in range(150)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    w = np.concatenate(paths)
    for step in (0.05, 0.2, 0.74):
        got = gpu.PathClearance(w, off, step, 0.3)
        pos, ns = fiesta_amd.path_samples(w, off, step)
        dc, _ = cpu.GetDistWithGradTrilinear(pos)
        want = np.minimum.reduceat(dc, np.concatenate([[0], np.cumsum(ns)[:-1]]))
        assert np.array_equal(got["min_dist"], want), step
    gpu.close()
    cpu.close()


def test_no_stale_state_after_an_incremental_update(hip_lib):
    """free the obstacle nearest to a path and run UpdateESDF on the incremental cell transform: the path query follows the
    new field exactly as the point route does"""
    import fiesta_amd
    m, S = dense_map(160, obstacles=1200, seed=8, engine="cells")
    w = np.array([[0.5, 0.5, 0.5], [15.0, 15.0, 15.0], [0.5, 15.0, 4.0]])
    off = np.array([0, 3])
    pos, _ = fiesta_amd.path_samples(w, off, 0.05)
    d0, _ = m.GetDistWithGradTrilinear(pos)
    before = m.PathClearance(w, off, 0.05, 0.2)
    assert_same(before, model(m, w, off, 0.05, 0.2), "before")
    # the obstacle under the path's closest sample
    vox = np.floor(before["min_pos"][0] / 0.1).astype(np.int64)
    k = int(np.argmin(((S - vox) ** 2).sum(1)))
    for _ in range(6):
        m.SetOccupancy(S[k:k + 1], 0, want_ret=False)
        m.UpdateOccupancy(True)
    st = m.UpdateESDF()
    assert st["cells"] == 1 and st["nn_incremental"] == 1, st
    after = m.PathClearance(w, off, 0.05, 0.2)
    assert_same(after, model(m, w, off, 0.05, 0.2), "after")
    d1, _ = m.GetDistWithGradTrilinear(pos)
    assert (d1 != d0).any() and after["min_dist"][0] >= before["min_dist"][0]    # the field moved under the path
    m.close()


def test_invalid_inputs(hip_lib):
    import torch
    import fiesta_amd
    from fiesta_amd._lib import PathResult
    m, _ = dense_map(32, obstacles=30)
    lib = m._lib
    probe = np.array([[1.0, 1.0, 1.0]] * 9)
    ref = m.GetDistWithGradTrilinear(probe)

    def still_works():
        d, g = m.GetDistWithGradTrilinear(probe)
        assert np.array_equal(d, ref[0]) and np.array_equal(g, ref[1])

    w = np.array([[0.5, 0.5, 0.5], [2.0, 2.0, 2.0], [1.0, 2.0, 0.5]])
    out = np.zeros(16)
    res = PathResult(out.ctypes.data, None, None, None, None, None, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    off = np.array([0, 3], np.int64)
    off_start, off_end, off_down = np.array([1, 3], np.int64), np.array([0, 2], np.int64), np.array([0, 2, 1, 3], np.int64)
    bad_calls = [(p(w), 3, p(off), 1, 0.0, 0.0, C.byref(res)), (p(w), 3, p(off), 1, -0.1, 0.0, C.byref(res)),
                 (p(w), 3, p(off), 1, float("inf"), 0.0, C.byref(res)), (p(w), 3, p(off), 1, float("nan"), 0.0, C.byref(res)),
                 (p(w), 3, p(off), 1, 0.1, float("nan"), C.byref(res)),
                 (p(w), 3, p(off_start), 1, 0.1, 0.0, C.byref(res)),
                 (p(w), 3, p(off_end), 1, 0.1, 0.0, C.byref(res)),
                 (p(w), 3, p(off_down), 3, 0.1, 0.0, C.byref(res)),
                 (None, 3, p(off), 1, 0.1, 0.0, C.byref(res)), (p(w), 3, None, 1, 0.1, 0.0, C.byref(res)),
                 (p(w), 3, p(off), 1, 0.1, 0.0, None)]
    for args in bad_calls:
        assert lib.fiesta_hip_path_clearance(m._h, *args) == 1, args       # FIESTA_HIP_ERR_INVALID
        still_works()
    assert lib.fiesta_hip_path_clearance_dev(m._h, None, 3, None, 1, 0.1, 0.0, C.byref(res)) == 1
    assert lib.fiesta_hip_path_clearance_dev(m._h, p(w), 3, p(off), 1, 0.1, float("nan"), C.byref(res)) == 1
    still_works()
    off0 = np.array([0], np.int64)
    assert lib.fiesta_hip_path_clearance(m._h, p(w), 0, p(off0), 0, 0.1, 0.0, C.byref(res)) == 0   # n_paths = 0: nothing to do
    # device variant: offsets out of order flag their paths only; a NaN waypoint flags its path only
    rng = np.random.RandomState(3)
    W = 0.3 + rng.rand(40, 3) * 2.5
    W[23] = [np.nan, 1.0, 1.0]
    off = np.array([0, 5, 10, 15, 20, 25, 30, 35, 40], np.int64)
    swapped = off.copy()
    swapped[2], swapped[3] = 15, 10          # entries 2 and 3 swapped: paths 2 ([15, 10)) and 3 (starts below entry 2) flagged
    dev = torch.device("cuda", 0)
    from fiesta_amd.esdf_map import PATH_FIELDS
    outs = {name: torch.empty((8,) + shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
            for name, dt, shape in PATH_FIELDS}
    wt, ot = torch.from_numpy(W).to(dev), torch.from_numpy(swapped).to(dev)
    m.PathClearanceDevice(wt.data_ptr(), len(W), ot.data_ptr(), 8, 0.05, 0.2, {k: v.data_ptr() for k, v in outs.items()})
    m.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    assert list(got["n_samples"][[2, 3, 4]]) == [-1, -1, -1], got["n_samples"]   # (4: the NaN waypoint)
    assert np.isnan(got["min_dist"][[2, 3, 4]]).all() and (got["min_index"][[2, 3, 4]] == -1).all()
    assert (got["first_below"][[2, 3, 4]] == -1).all() and np.isnan(got["min_pos"][[2, 3, 4]]).all()
    for q in (0, 1, 5, 6, 7):                # the others as if asked alone
        a, b = swapped[q], swapped[q + 1]
        alone = m.PathClearance(W[a:b], [0, b - a], 0.05, 0.2)
        assert_same({k: v[q:q + 1] for k, v in got.items()}, alone, f"path {q}")
    # the host variant: the NaN path alone is flagged
    host = m.PathClearance(W, off, 0.05, 0.2)
    assert host["n_samples"][4] == -1 and (host["n_samples"][[0, 1, 2, 3, 5, 6, 7]] > 0).all()
    still_works()
    m.close()


def test_scale_against_the_device_point_route(hip_lib):
    """8192 paths x 128 waypoints on a 256^3 map of config 2's density (~8 M samples): equal to the point route through
    GetDistWithGradTrilinearDevice and torch; timings printed, not asserted"""
    import torch
    import fiesta_amd
    G, res = 256, 0.1
    m, _ = dense_map(G, obstacles=int(round(50000 * (G / 512.0) ** 3)), seed=12)
    rng = np.random.RandomState(13)
    T, K = 8192, 128
    start = 0.5 + rng.rand(T, 1, 3) * (G * res - 1.0)
    dirs = rng.randn(T, 1, 3) + np.cumsum(rng.randn(T, K, 3) * 0.2, 1)
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    path = start + np.cumsum(dirs * 8 * 0.4 * res, 1)
    lo, span = 0.3, G * res - 0.6
    path = lo + span - np.abs(np.remainder(path - lo, 2 * span) - span)
    w = np.ascontiguousarray(path.reshape(-1, 3))
    off = np.arange(0, T * K + 1, K).astype(np.int64)
    step = 0.4 * res
    pos, ns = fiesta_amd.path_samples(w, off, step)
    assert ns.sum() > 7_000_000
    dev = torch.device("cuda", 0)
    wt, ot, pt = torch.from_numpy(w).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(pos).to(dev)
    dist = torch.empty(len(pos), dtype=torch.float64, device=dev)
    grad = torch.empty((len(pos), 3), dtype=torch.float64, device=dev)
    from fiesta_amd.esdf_map import PATH_FIELDS
    outs = {name: torch.empty((T,) + shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
            for name, dt, shape in PATH_FIELDS}
    ptrs = {k: v.data_ptr() for k, v in outs.items()}
    for _ in range(2):
        m.PathClearanceDevice(wt.data_ptr(), len(w), ot.data_ptr(), T, step, 0.3, ptrs)
        m.GetDistWithGradTrilinearDevice(pt.data_ptr(), len(pos), dist.data_ptr(), grad.data_ptr())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.PathClearanceDevice(wt.data_ptr(), len(w), ot.data_ptr(), T, step, 0.3, ptrs)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m.GetDistWithGradTrilinearDevice(pt.data_ptr(), len(pos), dist.data_ptr(), grad.data_ptr())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"\n{T} paths, {int(ns.sum())} samples: fused {1e3 * (t1 - t0):.3f} ms, point queries alone {1e3 * (t2 - t1):.3f} ms")
    d, g = dist.cpu().numpy(), grad.cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    starts = np.concatenate([[0], np.cumsum(ns)[:-1]])
    mins = np.minimum.reduceat(d, starts)
    assert np.array_equal(got["min_dist"], mins)
    seg = np.repeat(np.arange(T), ns)
    first = np.full(T, len(d))
    np.minimum.at(first, seg[d == mins[seg]], np.nonzero(d == mins[seg])[0])
    assert np.array_equal(got["min_index"], first - starts)
    assert np.array_equal(got["min_grad"].view(np.int64), g[first].view(np.int64))
    assert np.array_equal(got["min_pos"].view(np.int64), pos[first].view(np.int64))
    fb = np.full(T, len(d))
    np.minimum.at(fb, seg[d < 0.3], np.nonzero(d < 0.3)[0])
    assert np.array_equal(got["first_below"], np.where(fb < len(d), fb - starts, -1))
    assert np.array_equal(got["n_samples"], ns)
    m.close()


def test_cpp_facade_example_matches_python(hip_lib, tmp_path):
    import __graft_entry__ as g
    import fiesta_amd
    g.build_hip()
    exe = str(tmp_path / "path_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "path_check.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    out = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
    h = lambda k: np.array([float.fromhex(v) for v in out[k]])   # noqa: E731
    m = fiesta_amd.ESDFMap((-4.0, -4.0, 0.0), 0.2, (8.0, 8.0, 4.0))
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancy(all_voxels((40, 40, 20)), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    pil = np.array([[10, 10], [20, 25], [30, 12], [14, 31]])
    S = np.concatenate([np.stack([np.full(20, x), np.full(20, y), np.arange(20)], 1) for x, y in pil]).astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    one = np.array([[-3.0, -2.0, 1.0], [-1.5, -1.0, 1.1], [0.5, -1.9, 1.2]])
    r1 = m.PathClearance(one, [0, 3], 0.05, 0.5)
    assert r1["n_samples"][0] <= 256
    assert h("one_min_dist")[0] == r1["min_dist"][0] and np.array_equal(h("one_min_grad"), r1["min_grad"][0])
    assert out["one_first_below"] == r1["first_below"][0]
    assert np.array_equal(h("one_first_below_pos"), r1["first_below_pos"][0], equal_nan=True)
    w = np.array([-3.5, -3.5, 1.0, 3.5, 3.5, 1.0, -3.0, 2.0, 0.5, -1.0, -2.0, 1.5, 1.0, 2.0, 2.5, 2.0, -3.0, 3.5, 3.0, 0.0, 0.3,
                  0.0, 0.0, 2.0, 2.0, 1.0, 2.0, 6.0, 1.0, 2.0]).reshape(-1, 3)
    r = m.PathClearance(w, [0, 2, 7, 10], 0.05, 0.5)
    assert r["n_samples"].sum() > 256
    assert_same({"min_dist": h("min_dist"), "min_pos": h("min_pos").reshape(3, 3), "min_grad": h("min_grad").reshape(3, 3),
                 "first_below_pos": h("first_below_pos").reshape(3, 3), "min_index": np.array(out["min_index"]),
                 "first_below": np.array(out["first_below"]), "n_samples": np.array(out["n_samples"])}, r, "C++ example")
    assert np.array_equal(h("path_sample_of_min").reshape(3, 3), r["min_pos"])
    assert r["first_below"][2] >= 0   # the path that leaves the map contacts where it leaves
    m.close()


# ---- segments of ONE sample each (waypoint spacing <= step): the evaluation kernel's 64-sample groups then cover 64 segments ----
def wall_map(n=64, res=0.1, wall_y=10):
    """every voxel observed, a wall of obstacles across the plane y = wall_y: the distance grows with y alone"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), res, (n * res,) * 3)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((0, 0, 0), (n - 1,) * 3, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    for _ in range(3):
        m.SetOccupancyBox((0, wall_y, 0), (n - 1, wall_y, n - 1), 1)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


def zigzag(runs, y0=2.6, amp=0.04):
    """waypoints along +x whose y alternates between y0 and y0 + amp; segments of S = 1 ... 5 at step 0.05 by their x advance"""
    dx = {1: 0.0015, 2: 0.07, 3: 0.12, 4: 0.17, 5: 0.22}
    x, y, pts = 0.5, y0, [[0.5, y0, 3.25]]
    for S, count in runs:
        for _ in range(count):
            x += dx[S]
            y = y0 + amp if y == y0 else y0
            pts.append([x, y, 3.25])
    return np.array(pts)


def test_runs_of_one_sample_segments_every_sample_in_place(hip_lib):
    """segments of ONE sample (waypoint spacing <= step): a group of 64 samples then spans 64 segments.  Zig-zag paths over a wall:
    every rule sample lies in the band y0 ... y0 + amp, so any sample evaluated off its rule position -- beyond a vertex, where an
    extrapolation along the wrong segment leads -- reads below the band's distances and shows in min_dist / first_below.  One path
    with runs of exactly 63, 64, 65, 128 and 200 one-sample segments between segments of S = 2 ... 5 (two pieces), one of 3000
    one-sample segments (three pieces)"""
    import torch
    import fiesta_amd
    m = wall_map()
    step = 0.05
    runs = [(3, 2), (1, 64), (4, 1), (1, 63), (2, 2), (1, 65), (5, 1), (1, 200), (3, 2), (1, 128), (2, 2)] * 2
    paths = [zigzag(runs), zigzag([(1, 2999)])]
    S = np.maximum(1, np.ceil(np.linalg.norm(np.diff(paths[0], axis=0), axis=1) / step)).astype(int)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], (S == 1).astype(int), [0]])))
    assert {63, 64, 65, 128, 200} <= set(np.diff(edges)[::2].tolist()) and set(S.tolist()) == {1, 2, 3, 4, 5}
    w = np.concatenate(paths)
    off = np.array([0, len(paths[0]), len(w)], np.int64)
    pos, ns = fiesta_amd.path_samples(w, off, step)
    assert ns[0] > 1024 and ns[1] == 3000
    d, _ = m.GetDistWithGradTrilinear(pos)
    band = d.min()
    dev = torch.device("cuda", 0)
    wt, ot = torch.from_numpy(w).to(dev), torch.from_numpy(off).to(dev)
    from fiesta_amd.esdf_map import PATH_FIELDS
    for margin in (band - 0.01, band + 1e-9, band + 0.02, 1e9):
        want = model(m, w, off, step, margin)
        assert_same(m.PathClearance(w, off, step, margin), want, f"one-sample runs, margin {margin}")
        outs = {name: torch.empty((2,) + shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
                for name, dt, shape in PATH_FIELDS}
        m.PathClearanceDevice(wt.data_ptr(), len(w), ot.data_ptr(), 2, step, margin, {k: v.data_ptr() for k, v in outs.items()})
        m.synchronize()
        assert_same({k: v.cpu().numpy() for k, v in outs.items()}, want, f"one-sample runs, device variant, margin {margin}")
    m.close()


def test_densely_sampled_rollouts(hip_lib):
    """a planner's own rollout passed as waypoints, spacing below the step (every segment S = 1), 3000 waypoints = three pieces:
    the path and every 7th prefix of it against the point route"""
    m, _ = dense_map(64, obstacles=250, seed=21)
    rng = np.random.RandomState(22)
    dirs = rng.randn(3000, 3) * 0.3 + np.array([1.0, 0.4, 0.2])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    walk = 0.5 + np.cumsum(dirs * 0.016, 0)
    walk = 0.3 + 5.8 - np.abs(np.remainder(walk - 0.3, 2 * 5.8) - 5.8)      # (reflected into the map)
    paths = [walk] + [walk[:k] for k in range(1, 3000, 7)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    w = np.concatenate(paths)
    for margin in (0.0, 0.15, 0.3, 0.6):
        want = model(m, w, off, 0.05, margin)
        assert want["n_samples"][0] == 3000
        assert_same(m.PathClearance(w, off, 0.05, margin), want, f"rollout margin {margin}")
    m.close()


def test_host_cache_threshold_is_256_samples(hip_lib):
    """exactly 256 samples: the host brick cache; 257: the device -- the same bits either side"""
    m, _ = dense_map(64, obstacles=250, seed=23)
    step = 0.01
    for n, host in ((256, True), (257, False)):
        w = np.array([[0.5, 1.0, 1.5], [0.5 + (n - 1) * step * 0.999, 1.0, 1.5]])   # one segment of S = n - 1, plus the end
        before = m.host_cache_fetches
        got = m.PathClearance(w, [0, 2], step, 0.2)
        assert got["n_samples"][0] == n
        assert (m.host_cache_fetches > before) == host, (n, before, m.host_cache_fetches)
        assert_same(got, model(m, w, [0, 2], step, 0.2), f"{n} samples")
    m.close()


def test_a_garbage_offset_costs_its_own_two_paths(hip_lib):
    """device variant: an entry far outside [0, n_waypoints] (or negative) flags the two paths that share it, nothing else"""
    import torch
    from fiesta_amd.esdf_map import PATH_FIELDS
    m, _ = dense_map(32, obstacles=30)
    rng = np.random.RandomState(24)
    W = 0.3 + rng.rand(60, 3) * 2.5
    off = np.arange(0, 61, 5).astype(np.int64)                   # 12 paths of 5 waypoints
    bad = off.copy()
    bad[3], bad[8] = 10 ** 9, -7
    dev = torch.device("cuda", 0)
    outs = {name: torch.empty((12,) + shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
            for name, dt, shape in PATH_FIELDS}
    wt, ot = torch.from_numpy(W).to(dev), torch.from_numpy(bad).to(dev)
    m.PathClearanceDevice(wt.data_ptr(), len(W), ot.data_ptr(), 12, 0.05, 0.2, {k: v.data_ptr() for k, v in outs.items()})
    m.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    flagged = [2, 3, 7, 8]
    assert list(np.nonzero(got["n_samples"] < 0)[0]) == flagged, got["n_samples"]
    good = m.PathClearance(W, off, 0.05, 0.2)
    keep = [q for q in range(12) if q not in flagged]
    assert_same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in good.items()}, "the other paths")
    m.close()


def test_path_counts_around_the_1024_thread_trip(hip_lib):
    """device variant, 1023 / 1024 / 1025 paths of two waypoints: k_path_check and k_path_pieces take 1024 paths per trip.  First the
    offsets as they are (at 1025 the last path's first piece is the carry alone); then the LAST path's first offset is set to 5: in
    range, so within its own trip (at 1025 it is alone there) it is the largest entry so far -- only the running maximum carried
    over from the trip before shows that it lies below an earlier offset.  It flags the two paths that share it, nothing else"""
    import torch
    from fiesta_amd.esdf_map import PATH_FIELDS
    m, _ = dense_map(32, obstacles=30)
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(26)
    for n in (1023, 1024, 1025):
        a = 0.4 + rng.rand(n, 3) * 2.2
        W = np.ascontiguousarray(np.stack([a, a + rng.randn(n, 3) * 0.15], 1).reshape(-1, 3))
        off = np.arange(0, 2 * n + 1, 2).astype(np.int64)
        want = model(m, W, off, 0.05, 0.25)
        assert (want["n_samples"] >= 2).all() and (want["first_below"] >= 0).any() and (want["first_below"] < 0).any()
        bad = off.copy()
        bad[n - 1] = 5
        wt = torch.from_numpy(W).to(dev)
        for offsets, flagged in ((off, []), (bad, [n - 2, n - 1])):
            outs = {name: torch.full((n,) + shape, -7, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
                    for name, dt, shape in PATH_FIELDS}
            ot = torch.from_numpy(offsets).to(dev)
            torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the fills above must have landed)
            m.PathClearanceDevice(wt.data_ptr(), len(W), ot.data_ptr(), n, 0.05, 0.25, {k: v.data_ptr() for k, v in outs.items()})
            m.synchronize()
            got = {k: v.cpu().numpy() for k, v in outs.items()}
            assert list(np.nonzero(got["n_samples"] < 0)[0]) == flagged, (n, got["n_samples"][-3:])
            keep = [q for q in range(n) if q not in flagged]
            assert_same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in want.items()}, f"{n} paths, flagged {flagged}")
    m.close()


def test_hash_block_map_device_variant_and_host_cache(hip_lib):
    """hash-block map: the device variant with its offset check, and the host brick cache over a field that varies"""
    import torch
    import fiesta_amd
    from fiesta_amd.esdf_map import PATH_FIELDS
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, reserve_size=100000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((-20, -20, -10), (40, 30, 20), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    rng = np.random.RandomState(25)
    S = np.stack([rng.randint(-20, 41, 200), rng.randint(-20, 31, 200), rng.randint(-10, 21, 200)], 1).astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    w, off = make_paths(rng, (-1.5, -1.5, -0.5), (3.5, 2.5, 1.5), 0.1, n_paths=60, long_path=False)
    host = m.PathClearance(w, off, 0.05, 0.3)
    assert_same(host, model(m, w, off, 0.05, 0.3), "hash host variant")
    dev = torch.device("cuda", 0)
    swapped = off.copy()
    q = len(off) // 2
    swapped[q], swapped[q + 1] = off[q + 1], off[q]
    outs = {name: torch.empty((len(off) - 1,) + shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
            for name, dt, shape in PATH_FIELDS}
    wt, ot = torch.from_numpy(w).to(dev), torch.from_numpy(swapped).to(dev)
    m.PathClearanceDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, 0.05, 0.3, {k: v.data_ptr() for k, v in outs.items()})
    m.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    moved = {q - 1, q, q + 1} if off[q + 1] != off[q] else set()
    keep = [p for p in range(len(off) - 1) if p not in moved]
    assert_same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in host.items()}, "hash device variant")
    if moved:   # (path q - 1 now spans paths q - 1 and q: a valid range; q is reversed, q + 1 starts below an earlier entry)
        assert got["n_samples"][q] < 0 and got["n_samples"][q + 1] < 0
    # <= 256 samples near obstacles: the host brick cache, a field that varies along the path
    near = S[:6].astype(float) * 0.1 + 0.05                       # obstacle voxel centres; a short path beside each
    small = np.concatenate([[c + [0.13, 0.0, 0.0], c + [0.13, 0.2, 0.0], c + [0.25, 0.2, 0.1]] for c in near])
    off_s = np.arange(0, 19, 3)
    before = m.host_cache_fetches
    got_s = m.PathClearance(small, off_s, 0.05, 0.12)
    assert 0 < got_s["n_samples"].sum() <= 256 and m.host_cache_fetches > before
    want_s = model(m, small, off_s, 0.05, 0.12)
    assert_same(got_s, want_s, "hash host cache")
    assert (want_s["min_dist"] < 0.3).all()                       # (close to obstacles: not the 10000 of unallocated corners)
    m.close()
