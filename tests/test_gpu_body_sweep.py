"""Body sweeps on the device (fiesta_hip_body_sweep / _dev, include/fiesta_hip.h) against fiesta_amd.body_sweep_model over the map's
own point query: every output by bits, the NaN pattern included -- nothing is summed, so there is no tolerance anywhere.

Then independently of the new model's reductions (the existing body query on the rule's sample poses, reduced with numpy), the
shape edges (team sizes, pieces, runs of one-sample segments, ties), both variants and both stores, null outputs, the whole-call
errors, the device variant's offset rules, what the call is for (a rod that yaws into a wall while its centre stays clear), and the
stale field.  The resource test needs the built library only.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_gpu_body_query import random_body
from test_gpu_path_cost import hash_map_scene
from test_gpu_path_queries import dense_map, wall_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("min_clearance", "min_sample", "min_sphere", "min_pose", "min_pos", "min_grad", "first_below", "first_below_sphere",
          "first_below_pose", "n_below", "n_samples")
KS = (1, 3, 8, 64, 65, 130, 1024)
SENTINEL = -7
STEP = 0.05


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_bits(got, want, keys=FIELDS, what=""):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries differ in bits, first {bad[:3].tolist()}: got {a[tuple(bad[0])]!r} want {b[tuple(bad[0])]!r}"


def model_of(m, sph, poses, off, step, margin):
    import fiesta_amd
    return fiesta_amd.body_sweep_model(m.GetDistWithGradTrilinear, sph, poses, off, step, margin)


def device_call(m, sph, poses, off, step, margin, rows=None, skip=(), fill=SENTINEL, n_poses=None):
    """fiesta_hip_body_sweep_dev on torch tensors of `rows` rows (default: one per path), every output pre-filled with `fill`; the
    fields named in `skip` are passed as null"""
    import torch
    from fiesta_amd.esdf_map import SWEEP_FIELDS
    dev = torch.device("cuda", 0)
    sph = np.ascontiguousarray(sph, np.float64).reshape(-1, 4)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    off = np.ascontiguousarray(off, np.int64).reshape(-1)
    n = len(off) - 1
    rows = n if rows is None else rows
    pt = torch.from_numpy(P).to(dev) if len(P) else torch.zeros((1, 7), dtype=torch.float64, device=dev)
    ot = torch.from_numpy(off).to(dev)
    kinds = {np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32}
    outs = {name: torch.full((rows,) + shape, fill, dtype=kinds[dt], device=dev) for name, dt, shape in SWEEP_FIELDS}
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the uploads and fills above must have landed)
    m.BodySweepDevice(sph, pt.data_ptr(), len(P) if n_poses is None else n_poses, ot.data_ptr(), n, step, margin,
                      {k: v.data_ptr() for k, v in outs.items() if k not in skip})
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def random_quats(rng, n):
    q = rng.randn(n, 4)
    return q * (10.0 ** rng.uniform(-1, 1, n) / np.linalg.norm(q, axis=1))[:, None]


def random_sweeps(rng, n_paths, lo, hi, leg=0.3, inset=0.7, lo_poses=2, hi_poses=9, query=None):
    """n_paths polylines of lo_poses .. hi_poses poses: random walks of ~leg metres per segment from a start inside the box [lo, hi]
    shrunk by `inset` (every eighth path starts on the box's surface and leaves it), random quaternions of norm 0.1 .. 10; every
    few poses keep their predecessor's position (a turn in place) or its rotation (a pure translation).  With a map's point
    `query`, every other path starts at the most open of 40 candidate starts and walks a sixth as far: paths that stay clear"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    rows, off = [], [0]
    for p in range(n_paths):
        nw = int(rng.randint(lo_poses, hi_poses + 1))
        pos = lo + inset + rng.rand(3) * (hi - lo - 2 * inset)
        far = leg
        if p % 8 == 7:
            c = rng.randint(3)
            pos[c] = lo[c] if rng.rand() < 0.5 else hi[c]
        elif query is not None and p % 2 == 0:
            cand = lo + inset + rng.rand(40, 3) * (hi - lo - 2 * inset)
            d = np.asarray(query(cand)[0])
            pos, far = cand[int(np.argmax(np.where(d < 1000.0, d, -1.0)))], leg / 6
        q = random_quats(rng, 1)[0]
        for j in range(nw):
            kind = rng.randint(0, 8) if j else 7
            if kind != 0:
                pos = pos + rng.randn(3) * far
            if kind != 1:
                q = random_quats(rng, 1)[0]
            rows.append(list(pos) + list(q))
        off.append(len(rows))
    return np.array(rows, np.float64), np.array(off, np.int64)


def scene_of(name):
    if name == "scatter64":
        m, _ = dense_map(64)
        return m, np.zeros(3), np.full(3, 6.4)
    if name == "partial64":
        m, _ = dense_map(64, obstacles=300, seed=2, hidden_blocks=12)
        return m, np.zeros(3), np.full(3, 6.4)
    if name == "ragged32":
        m, _ = dense_map(32, res=0.2, origin=(-3.2, -3.2, 0.0), obstacles=120, seed=11)
        return m, np.array([-3.2, -3.2, 0.0]), np.array([3.2, 3.2, 6.4])
    m, _ = hash_map_scene()
    return m, np.array([-2.0, -2.0, -1.0]), np.array([4.1, 3.1, 2.1])          # the observed box


def body_for(rng, K):
    """small bodies for the small tables, so that a good share of the paths stays clear of everything"""
    return random_body(rng, K, across={1: 0.2, 3: 0.3, 8: 0.4, 64: 0.6}.get(K, 0.8))


def per_sample(m, sph, poses, off, step, margin):
    """the existing body query on the rule's sample poses: (its outputs per sample, n_samples, first row of every path)"""
    import fiesta_amd
    samples, n = fiesta_amd.sweep_poses(poses, off, step, fiesta_amd.body_reach(sph))
    bq = m.BodyQuery(sph, samples, margin)
    return bq, n, np.cumsum(np.maximum(n, 0)) - np.maximum(n, 0)


# ---- 1. against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["scatter64", "partial64", "ragged32", "hash"])
def test_body_sweep_equals_the_model(hip_lib, scene):
    m, lo, hi = scene_of(scene)
    rng = np.random.RandomState(len(scene) + 40)
    paths = contact = outside = unknown = 0
    for K in KS:
        sph = body_for(rng, K)
        poses, off = random_sweeps(rng, 9 if K == 1024 else 65, lo, hi, query=m.GetDistWithGradTrilinear)
        for margin in (0.4, -2.0):
            want = model_of(m, sph, poses, off, STEP, margin)
            assert_bits(m.BodySweep(sph, poses, off, STEP, margin), want, what=f"{scene} K {K} margin {margin}")
            if margin == -2.0:
                assert np.all(want["first_below"] == -1) and not want["n_below"].any()
                continue
            assert np.all(want["n_samples"] > 1)
            paths += len(off) - 1
            contact += int(np.count_nonzero(want["first_below"] >= 0))
        bq, _, _ = per_sample(m, sph, poses, off, STEP, 0.4)
        d = bq["sphere_clearance"] + sph[None, :, 3]
        outside += int(np.count_nonzero(np.abs(d + 1.0) < 1e-9))
        unknown += int(np.count_nonzero(d > 1000.0))
    # against an empty test: paths in contact and paths that stay clear, spheres that left the map, spheres in never-observed blocks
    print(f"{scene}: {contact} of {paths} paths in contact at margin 0.4; sphere samples outside the map {outside}, in unknown space {unknown}")
    assert 4 * contact >= paths and 4 * (paths - contact) >= paths, (contact, paths)
    assert (outside > 100 or scene == "hash") and (unknown > 100 or scene in ("scatter64", "ragged32")), (outside, unknown)
    m.close()


# ---- 2. against the existing call ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["dense", "hash"])
def test_body_sweep_equals_the_body_query_reduced_with_numpy(hip_lib, store):
    m, lo, hi = scene_of("partial64" if store == "dense" else "hash")
    rng = np.random.RandomState(21)
    for K in (1, 8, 65):
        sph = body_for(rng, K)
        poses, off = random_sweeps(rng, 65, lo, hi, query=m.GetDistWithGradTrilinear)
        got = m.BodySweep(sph, poses, off, STEP, 0.4)
        bq, n, first = per_sample(m, sph, poses, off, STEP, 0.4)
        assert np.array_equal(got["n_samples"], n) and n.min() > 1
        hits = 0
        for p in range(65):
            rows = slice(first[p], first[p] + n[p])
            mc = bq["min_clearance"][rows]
            i = int(np.argmin(mc))                                   # the first (lowest) sample of the minimum
            below = np.nonzero(bq["n_below"][rows] > 0)[0]
            assert bits(got["min_clearance"][p:p + 1])[0] == bits(mc[i:i + 1])[0], (K, p)
            assert got["min_sample"][p] == i and got["min_sphere"][p] == bq["min_sphere"][rows][i], (K, p)
            assert got["first_below"][p] == (below[0] if len(below) else -1) and got["n_below"][p] == len(below), (K, p)
            hits += len(below) > 0
        assert 5 < hits < 65, hits
    m.close()


# ---- 3. shape edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_sizes_and_a_paths_place_in_the_batch(hip_lib):
    m, lo, hi = scene_of("scatter64")
    rng = np.random.RandomState(31)
    sph = body_for(rng, 8)
    poses, off = random_sweeps(rng, 257, lo, hi, hi_poses=4)
    big = device_call(m, sph, poses, off, STEP, 0.4)
    assert_bits(big, model_of(m, sph, poses, off, STEP, 0.4), what="257 paths")
    assert_bits(device_call(m, sph, poses, off, STEP, 0.4), big, what="the same call again")
    for p in (0, 100, 256):                                          # n_paths = 1: a path's bits do not depend on the batch
        one = device_call(m, sph, poses[off[p]:off[p + 1]], [0, off[p + 1] - off[p]], STEP, 0.4, rows=3)
        assert_bits({k: v[:1] for k, v in one.items()}, {k: v[p:p + 1] for k, v in big.items()}, what=f"path {p} alone")
        assert all(np.all(v[1:] == SENTINEL) for v in one.values())                              # nothing written past n_paths
    order = rng.permutation(257)
    moved = np.concatenate([poses[off[p]:off[p + 1]] for p in order])
    moved_off = np.concatenate([[0], np.cumsum(np.diff(off)[order])])
    assert_bits(device_call(m, sph, moved, moved_off, STEP, 0.4), {k: v[order] for k, v in big.items()}, what="permuted batch")
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 8, 65])
def test_pieces_runs_of_one_sample_segments_and_special_paths(hip_lib, K):
    """one batch: a path of 6.5 m at step 0.002 (3266 samples: several pieces at every team size), a path of 130 one-sample segments
    (a trip's samples lie on as many segments), turns in place, repeated poses, and an empty, a one-pose and an invalid path in the
    middle"""
    m = wall_map()
    rng = np.random.RandomState(K)
    sph = random_body(rng, K, across=0.5)
    q = [0.5, 0.5, -0.5, 0.5]
    long_path = [[0.3, 2.6, 0.4] + q, [6.1, 1.1, 3.0] + q]      # (the body stays inside the map: wall_map is 6.4 m wide)
    runs = [[0.5 + 0.0015 * i, 2.0 + 0.001 * (i % 2), 3.2] + q for i in range(131)]
    turns = [[3.0, 1.6, 3.0] + list(random_quats(rng, 1)[0]) for _ in range(6)]
    repeat = [[2.0, 1.5, 3.0, 0.0, 3.0, 0.0, 0.0]] * 3 + [[2.0, 1.5, 3.0, 0.0, -1.0, 0.0, 0.0]] * 2
    invalid = [[1.0, 2.0, 3.0] + q, [1.5, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0], [2.0, 2.0, 3.0] + q]
    single = [[4.0, 1.3, 3.0, 0.0, 0.0, 7.0, 0.0]]
    batch = [long_path, runs, [], turns, invalid, single, repeat, []]
    poses = np.array([r for path in batch for r in path], np.float64)
    off = np.concatenate([[0], np.cumsum([len(path) for path in batch])])
    step = 0.002
    want = model_of(m, sph, poses, off, step, 0.5)
    assert want["n_samples"][1] == 131 and want["n_samples"][2] == 0 and want["n_samples"][4] == -1 and want["n_samples"][5] == 1
    assert want["n_samples"][6] == 5 and want["n_samples"][7] == 0 and want["n_samples"][3] > 6
    assert want["n_samples"][0] > 2 * 1024 + 2                       # more than two of the largest pieces
    for got in (m.BodySweep(sph, poses, off, step, 0.5), device_call(m, sph, poses, off, step, 0.5)):
        assert_bits(got, want, what=f"K {K}")
    assert want["first_below"][0] > 1024                              # the long path comes down to the wall: contact in a later piece
    # the special rows, spelled out
    for p in (2, 7):
        assert got["min_clearance"][p] == np.inf and got["n_below"][p] == 0
    assert np.isnan(got["min_clearance"][4]) and got["n_below"][4] == -1
    for p in (2, 4, 7):
        assert got["min_sample"][p] == got["min_sphere"][p] == got["first_below"][p] == got["first_below_sphere"][p] == -1
        assert np.isnan(got["min_pose"][p]).all() and np.isnan(got["min_pos"][p]).all() and np.isnan(got["first_below_pose"][p]).all()
        assert not got["min_grad"][p].any()
    assert got["min_sample"][5] == 0 and got["min_pose"][5].tolist() == [4.0, 1.3, 3.0, 0.0, 0.0, 1.0, 0.0]
    m.close()


@pytest.mark.gpu
def test_ties_name_the_lowest_sample_then_the_lowest_sphere(hip_lib):
    """out and back: the first and the last pose are the same bits, so the samples there tie exactly, and the path is closest to the
    wall there; spheres 1 and 3 of the table are the same sphere, the one nearest the wall and the only one below the margin there"""
    m = wall_map()
    q = [2.0, 0.0, 0.0, 0.0]
    for K, T in ((4, "teams of 4, one piece"), (70, "a team of 64, many pieces")):
        sph = np.zeros((K, 4))
        sph[:, 0] = np.linspace(-0.3, 0.3, K)
        sph[:, 3] = 0.05
        sph[1] = sph[3] = [0.1, -0.4, 0.0, 0.05]                      # nearest the wall (the wall lies towards -y)
        a, b = [3.0, 2.0, 3.0] + q, [3.2, 2.6, 3.1] + q
        for poses in ([a, b, a], [a, b, a, b, a]):
            poses, off = np.array(poses), np.array([0, len(poses)])
            want = model_of(m, sph, poses, off, 0.01, 0.7)
            for got in (m.BodySweep(sph, poses, off, 0.01, 0.7), device_call(m, sph, poses, off, 0.01, 0.7)):
                assert_bits(got, want, what=f"ties, {T}")
                assert got["min_sample"][0] == 0 and got["min_sphere"][0] == 1 and got["n_samples"][0] > 128
                assert got["first_below"][0] == 0 and got["first_below_sphere"][0] == 1
            bq, n, _ = per_sample(m, sph, poses, off, 0.01, 0.7)
            at_min = np.nonzero(bq["min_clearance"] == want["min_clearance"][0])[0]
            assert len(at_min) >= 2 and at_min[0] == 0 and at_min[-1] == n[0] - 1                  # the tie across samples is real
            assert bq["sphere_clearance"][0, 1] == bq["sphere_clearance"][0, 3] == want["min_clearance"][0]   # and across spheres
    m.close()


@pytest.mark.gpu
def test_the_sample_limit_on_the_device(hip_lib):
    """exactly 2^24 samples in a segment is valid, one ulp more is not (one sphere at the origin: W = 0)"""
    m, _ = dense_map(32, obstacles=30)
    q = [1.0, 0.0, 0.0, 0.0]
    lim = 2.0 ** 24
    poses = np.array([[0.0, 1.0, 1.0] + q, [lim, 1.0, 1.0] + q, [0.0, 1.0, 1.0] + q, [np.nextafter(lim, np.inf), 1.0, 1.0] + q])
    got = m.BodySweep([[0.0, 0.0, 0.0, 0.1]], poses, [0, 2, 4], 1.0, 0.3)
    assert got["n_samples"].tolist() == [2 ** 24 + 1, -1] and got["min_clearance"][0] < 10 and np.isnan(got["min_clearance"][1])
    m.close()


# ---- 4. variants, null outputs, errors, offsets --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["dense", "hash"])
def test_both_variants_and_null_outputs(hip_lib, store):
    from fiesta_amd._lib import SweepResult
    m, lo, hi = scene_of("scatter64" if store == "dense" else "hash")
    rng = np.random.RandomState(41)
    sph = body_for(rng, 8)
    poses, off = random_sweeps(rng, 70, lo, hi, hi_poses=5)
    poses[off[9] + 1, 3:] = 0.0                                      # (an invalid path: its rows honour the nulls too)
    full = device_call(m, sph, poses, off, STEP, 0.4)
    assert_bits(m.BodySweep(sph, poses, off, STEP, 0.4), full, what=f"{store}: the variants")
    assert_bits(full, model_of(m, sph, poses, off, STEP, 0.4), what=store)
    assert full["n_samples"][9] == -1
    for name in FIELDS:
        got = device_call(m, sph, poses, off, STEP, 0.4, skip=(name,))
        assert np.all(got[name] == SENTINEL), name
        assert_bits(got, full, [k for k in FIELDS if k != name], f"without {name}")
    none = device_call(m, sph, poses, off, STEP, 0.4, skip=FIELDS)
    assert all(np.all(v == SENTINEL) for v in none.values())
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    empty = SweepResult()
    assert m._lib.fiesta_hip_body_sweep(m._h, p(sph), 8, p(poses), len(poses), p(off), 70, STEP, 0.4, C.byref(empty)) == 0   # host, all null
    fb = np.zeros(70, np.int64)
    only = SweepResult(first_below=fb.ctypes.data)
    assert m._lib.fiesta_hip_body_sweep(m._h, p(sph), 8, p(poses), len(poses), p(off), 70, STEP, 0.4, C.byref(only)) == 0
    assert np.array_equal(fb, full["first_below"])
    m.close()


@pytest.mark.gpu
def test_whole_call_errors(hip_lib):
    from fiesta_amd._lib import SweepResult
    m, lo, hi = scene_of("scatter64")
    lib = m._lib
    rng = np.random.RandomState(9)
    sph = body_for(rng, 3)
    poses, off = random_sweeps(rng, 6, lo, hi, hi_poses=4)
    n = len(poses)
    ref = m.BodySweep(sph, poses, off, STEP, 0.4)
    out = np.zeros(6)
    res = SweepResult(min_clearance=out.ctypes.data)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    many = np.zeros((1025, 4))

    def with_sphere(row, col, v):
        t = sph.copy()
        t[row, col] = v
        return t

    def with_off(i, v):
        t = off.copy()
        t[i] = v
        return t
    inf, nan = float("inf"), float("nan")
    r = C.byref(res)
    both = [("null", (None, p(sph), 3, p(poses), n, p(off), 6, STEP, 0.4, r)),
            ("null", (m._h, None, 3, p(poses), n, p(off), 6, STEP, 0.4, r)),
            ("null", (m._h, p(sph), 3, None, n, p(off), 6, STEP, 0.4, r)),
            ("null", (m._h, p(sph), 3, p(poses), n, None, 6, STEP, 0.4, r)),
            ("null", (m._h, p(sph), 3, p(poses), n, p(off), 6, STEP, 0.4, None)),
            ("n_spheres", (m._h, p(sph), 0, p(poses), n, p(off), 6, STEP, 0.4, r)),
            ("n_spheres", (m._h, p(many), 1025, p(poses), n, p(off), 6, STEP, 0.4, r)),
            ("negative count", (m._h, p(sph), 3, p(poses), -1, p(off), 6, STEP, 0.4, r)),
            ("negative count", (m._h, p(sph), 3, p(poses), n, p(off), -1, STEP, 0.4, r)),
            ("not finite", (m._h, p(with_sphere(2, 0, nan)), 3, p(poses), n, p(off), 6, STEP, 0.4, r)),
            ("not finite", (m._h, p(with_sphere(0, 3, inf)), 3, p(poses), n, p(off), 6, STEP, 0.4, r)),
            ("radius is negative", (m._h, p(with_sphere(1, 3, -1e-9)), 3, p(poses), n, p(off), 6, STEP, 0.4, r)),
            ("step", (m._h, p(sph), 3, p(poses), n, p(off), 6, 0.0, 0.4, r)),
            ("step", (m._h, p(sph), 3, p(poses), n, p(off), 6, -STEP, 0.4, r)),
            ("step", (m._h, p(sph), 3, p(poses), n, p(off), 6, nan, 0.4, r)),
            ("step", (m._h, p(sph), 3, p(poses), n, p(off), 6, inf, 0.4, r)),
            ("margin", (m._h, p(sph), 3, p(poses), n, p(off), 6, STEP, nan, r)),
            ("margin", (m._h, p(sph), 3, p(poses), n, p(off), 6, STEP, inf, r)),
            ("margin", (m._h, p(sph), 3, p(poses), n, p(off), 6, STEP, -inf, r))]
    host_only = [("offsets[0]", (m._h, p(sph), 3, p(poses), n, p(with_off(0, 1)), 6, STEP, 0.4, r)),
                 ("offsets[0]", (m._h, p(sph), 3, p(poses), n, p(with_off(6, n - 1)), 6, STEP, 0.4, r)),
                 ("offsets[0]", (m._h, p(sph), 3, p(poses), n + 1, p(off), 6, STEP, 0.4, r)),
                 ("non-decreasing", (m._h, p(sph), 3, p(poses), n, p(with_off(3, off[2] - 1)), 6, STEP, 0.4, r))]
    for fn, calls in ((lib.fiesta_hip_body_sweep, both + host_only), (lib.fiesta_hip_body_sweep_dev, both)):   # (the checks come before any pointer is used)
        for word, args in calls:
            out[:] = SENTINEL
            assert fn(*args) == 1, (word, args)                                  # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
            assert np.all(out == SENTINEL)
            assert_bits(m.BodySweep(sph, poses, off, STEP, 0.4), ref, what=f"a good call after '{word}'")      # the map is still usable
    zero = np.zeros(1, np.int64)
    assert lib.fiesta_hip_body_sweep(m._h, p(sph), 3, p(poses), 0, p(zero), 0, STEP, 0.4, r) == 0           # n_paths = 0 does nothing
    assert lib.fiesta_hip_body_sweep_dev(m._h, p(sph), 3, p(poses), 0, p(zero), 0, STEP, 0.4, r) == 0 and np.all(out == SENTINEL)
    assert lib.fiesta_hip_version() == 101
    m.close()


def checked_ranges(off, n_poses):
    """path clearance's device rule: path p is valid iff its range is in order, inside [0, n_poses] and starts at the largest
    in-range offset seen so far"""
    ok, seen = [], None
    for p in range(len(off) - 1):
        o0, o1 = int(off[p]), int(off[p + 1])
        if 0 <= o0 <= n_poses:
            seen = o0 if seen is None else max(seen, o0)
        ok.append(o0 >= 0 and o0 == seen and o0 <= o1 <= n_poses)
    return ok


@pytest.mark.gpu
def test_device_variant_offset_rules(hip_lib):
    m, lo, hi = scene_of("scatter64")
    rng = np.random.RandomState(51)
    sph = body_for(rng, 8)
    poses, off = random_sweeps(rng, 40, lo, hi, hi_poses=4)
    n = len(poses)
    clean = device_call(m, sph, poses, off, STEP, 0.4)
    cases = {"reversed": (5, off[4] - 1), "beyond the end": (9, n + 3), "negative": (12, -2), "huge": (20, 2 ** 62), "back to an earlier path": (30, off[3]),
             "first not 0": (0, 1), "last short": (40, n - 1)}
    for what, (i, v) in cases.items():
        bad = off.copy()
        bad[i] = v
        ok = checked_ranges(bad, n)
        assert all(ok) == (what in ("first not 0", "last short")) and sum(ok) >= 35, (what, ok)      # (those two only move a range)
        got = device_call(m, sph, poses, bad, STEP, 0.4)
        for p in range(40):
            if not ok[p]:
                assert got["n_samples"][p] == -1 and np.isnan(got["min_clearance"][p]) and got["n_below"][p] == -1, (what, p)
                assert got["min_sample"][p] == -1 and got["first_below"][p] == -1 and np.isnan(got["min_pose"][p]).all(), (what, p)
            elif bad[p] == off[p] and bad[p + 1] == off[p + 1]:
                assert_bits({k: v[p:p + 1] for k, v in got.items()}, {k: v[p:p + 1] for k, v in clean.items()}, what=f"{what}: path {p}")
            else:                                                       # a valid range that is not the original one
                alone = device_call(m, sph, poses[bad[p]:bad[p + 1]], [0, bad[p + 1] - bad[p]], STEP, 0.4)
                assert_bits({k: v[p:p + 1] for k, v in got.items()}, alone, what=f"{what}: path {p} with its new range")
    short = device_call(m, sph, poses, off, STEP, 0.4, n_poses=n - 1)        # n_poses smaller than the offsets say: the last path only
    assert short["n_samples"][39] == -1
    assert_bits({k: v[:39] for k, v in short.items()}, {k: v[:39] for k, v in clean.items()}, what="n_poses one short")
    m.close()


# ---- 5. meaning ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_rod_that_yaws_into_the_wall_while_its_centre_stays_clear(hip_lib):
    """wall_map's wall fills the voxel layer y = 1.0 .. 1.1 m.  A rod of five spheres along the body x axis (half-length 0.5 m) flies
    along x at y = 1.8: parallel to the wall, 0.7 m off.  Over the middle segment it yaws by 90 degrees about z, which points its
    sphere 0 at the wall"""
    m = wall_map()
    rod = np.array([[0.25 * i, 0.0, 0.0, 0.05] for i in range(-2, 3)])
    half = math.sqrt(0.5)
    straight, across = [1.0, 0.0, 0.0, 0.0], [half, 0.0, 0.0, half]
    xs = (1.5, 2.5, 3.5, 4.5)
    poses = np.array([[xs[0], 1.8, 3.2] + straight, [xs[1], 1.8, 3.2] + straight, [xs[2], 1.8, 3.2] + across, [xs[3], 1.8, 3.2] + across])
    off, margin = np.array([0, 4]), 0.4
    got = m.BodySweep(rod, poses, off, STEP, margin)
    assert_bits(got, model_of(m, rod, poses, off, STEP, margin), what="the rod")
    first_seg = 20                                                     # 1 m at step 0.05, no rotation: W = 0
    turning = math.ceil((1.0 + 2.25 * 0.5 * 2.0 * math.sin(math.pi / 8)) / STEP)
    assert got["n_samples"][0] == first_seg + turning + 20 + 1
    fb = got["first_below"][0]
    assert first_seg < fb < first_seg + turning and got["first_below_sphere"][0] == 0, (fb, got["first_below_sphere"])
    assert xs[1] < got["first_below_pose"][0, 0] < xs[2] and got["first_below_pose"][0, 1] == 1.8
    assert got["min_sphere"][0] == 0 and got["min_sample"][0] >= first_seg + turning and 0.1 < got["min_clearance"][0] < 0.25
    assert got["min_pos"][0, 1] < 1.31 and got["min_grad"][0, 1] > 0.9                          # the tip, and the wall lies towards -y
    # the point robot on the same positions keeps the margin everywhere
    point = m.PathClearance(poses[:, :3], off, STEP, margin)
    assert point["first_below"][0] == -1 and point["min_dist"][0] > 0.6
    # the same flight without the yaw is free
    poses[:, 3:] = straight
    free = m.BodySweep(rod, poses, off, STEP, margin)
    assert free["first_below"][0] == -1 and free["n_below"][0] == 0 and free["min_clearance"][0] > 0.6 and free["n_samples"][0] == 61
    m.close()


# ---- 6. stale field ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["dense", "hash"])
def test_field_not_yet_updated(hip_lib, store):
    """a bar of five spheres turns in place; an obstacle appears three voxels beside it: before UpdateESDF the call answers from the
    old field, afterwards from the new one"""
    if store == "dense":
        m, _ = dense_map(64, obstacles=1)
        cands = [(32, 32, 32), (12, 12, 12), (50, 50, 12), (12, 50, 50)]
    else:
        m, _ = hash_map_scene(obstacles=1)
        cands = [(10, 5, 5), (-10, -10, 0), (30, 20, 10), (30, -10, 10)]
    vox = np.array(max(cands, key=lambda v: m.GetDistance(np.array([v], np.int32))[0]), np.int32)     # far from the scene's obstacle
    centre = (vox + 0.5) * 0.1
    sph = np.array([[-0.4, 0, 0, 0.05], [-0.2, 0, 0, 0.05], [0.0, 0, 0, 0.05], [0.2, 0, 0, 0.05], [0.4, 0, 0, 0.05]])
    half = math.sqrt(0.5)
    poses = np.array([[centre[0] - 0.3, centre[1], centre[2], 2.0, 0.0, 0.0, 0.0], [centre[0], centre[1], centre[2], half, 0.0, 0.0, half],
                      [centre[0] + 0.3, centre[1], centre[2], 1.0, 0.0, 0.0, 0.0]])
    off = np.array([0, 3])
    before = m.BodySweep(sph, poses, off, STEP, 0.5)
    assert_bits(before, model_of(m, sph, poses, off, STEP, 0.5), what=f"{store} before")
    assert before["min_clearance"][0] > 0.5 and before["first_below"][0] == -1
    new = (vox + (0, 7, 0))[None].astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(new, 1, want_ret=False)
        m.UpdateOccupancy(True)
    stale = m.BodySweep(sph, poses, off, STEP, 0.5)
    assert_bits(stale, before, what=f"{store} before UpdateESDF")
    assert_bits(stale, model_of(m, sph, poses, off, STEP, 0.5), what=f"{store} before UpdateESDF, against the map's own point query")
    assert_bits(device_call(m, sph, poses, off, STEP, 0.5), before, what=f"{store} before UpdateESDF, device variant")
    m.UpdateESDF()
    after = m.BodySweep(sph, poses, off, STEP, 0.5)
    assert_bits(after, model_of(m, sph, poses, off, STEP, 0.5), what=f"{store} after")
    # crosswise (the middle waypoint) the bar's sphere 4 points at the new obstacle, 0.7 m from the bar's centre
    assert after["first_below"][0] > 0 and after["min_sphere"][0] == 4 and 0.2 < after["min_clearance"][0] < 0.3, after
    assert after["n_below"][0] < after["n_samples"][0]
    m.close()


# ---- 7. resources (the built library only: no GPU) ----------------------------------------------------------------------------------
def test_sweep_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_sweep_" in k}
    assert len(res) == 6 and sum("DensePathEval" in k for k in res) == 2 and sum("HashPathEval" in k for k in res) == 2, sorted(res)
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    copies = check_kernel_resources.kernel_copies(so)
    assert all(len(copies[k]) == 1 for k in res)        # compiled once, in planner.hip
