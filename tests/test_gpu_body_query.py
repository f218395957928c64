"""Body queries on the device (fiesta_hip_body_query / _dev, include/fiesta_hip.h) against fiesta_amd.body_query_model over the
map's own point query.

The exact outputs (sphere_clearance, min_clearance, min_sphere, min_pos, min_grad, n_below) are compared by bits, cost and grad
within the header's bound (n + 16) * 2^-52 * A, the NaN pattern exactly.  Then what the rule cannot show: team sizes and batch edges,
both variants and both stores, every UpdateESDF engine, the stale field, invalid poses inside a batch, the whole-call errors and
what the gradient is for.  The resource test needs the built library only.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_gpu_path_cost import hash_map_scene
from test_gpu_path_queries import dense_map, wall_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "sphere_clearance")
ALL = EXACT + ("cost", "grad")
KS = (1, 2, 3, 5, 8, 63, 64, 65, 130, 1024)
SENTINEL = -7


def bound(n, a):
    return (np.asarray(n, np.float64) + 16.0) * 2.0 ** -52 * np.asarray(a, np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_bits(got, want, keys=ALL, what=""):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, f"{what} {k}: {len(bad)} entries differ in bits, first {bad[:3].tolist()}: got {a[tuple(bad[0])]!r} want {b[tuple(bad[0])]!r}"


def model_of(m, sph, poses, margin):
    import fiesta_amd
    return fiesta_amd.body_query_model(m.GetDistWithGradTrilinear, sph, poses, margin)


def assert_model(got, model, what=""):
    """the exact outputs by bits (NaN included), cost and grad within the bound of the model's (n, A), NaN exactly where the model has it"""
    assert_bits(got, model, EXACT, what)
    worst = {}
    for k in ("cost", "grad"):
        a, b = np.asarray(got[k], np.float64), model[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        lim = bound(model[k + "_n"] if k == "cost" else model["grad_n"][:, None], model[k + "_abs"])
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what} {k}: NaN pattern differs"
        err = np.where(np.isnan(b), 0.0, np.abs(a - b))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[k] = float(np.nanmax(np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0)), initial=0.0))
        bad = np.argwhere(err > lim)
        assert len(bad) == 0, (f"{what} {k}: {len(bad)} entries beyond the bound, first {bad[:3].tolist()}: got {a[tuple(bad[0])]!r} "
                               f"want {b[tuple(bad[0])]!r} bound {lim[tuple(bad[0])]!r}")
    print(f"{what}: worst error / bound  " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def device_call(m, sph, poses, margin, rows=None, skip=(), fill=SENTINEL):
    """fiesta_hip_body_query_dev on torch tensors of `rows` rows (default: one per pose), every output pre-filled with `fill`;
    the fields named in `skip` are passed as null"""
    import torch
    from fiesta_amd.esdf_map import BODY_FIELDS
    dev = torch.device("cuda", 0)
    sph = np.ascontiguousarray(sph, np.float64).reshape(-1, 4)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    rows = len(P) if rows is None else rows
    pt = torch.from_numpy(P).to(dev) if len(P) else torch.zeros((1, 7), dtype=torch.float64, device=dev)
    outs = {name: torch.full((rows,) + tuple(len(sph) if d == "K" else d for d in shape), fill,
                             dtype=torch.float64 if dt == np.float64 else torch.int32, device=dev) for name, dt, shape in BODY_FIELDS}
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the fills above must have landed)
    m.BodyQueryDevice(sph, pt.data_ptr(), len(P), margin, {k: v.data_ptr() for k, v in outs.items() if k not in skip})
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def random_body(rng, K, across=1.5):
    """K spheres inside a ball `across` metres wide, radii up to 0.15 m"""
    c = rng.randn(K, 3)
    c *= (0.5 * across * rng.rand(K) ** (1 / 3) / np.linalg.norm(c, axis=1))[:, None]
    return np.concatenate([c, rng.rand(K, 1) * 0.15], axis=1)


def random_poses(rng, N, lo, hi, out=0.4):
    """positions in the box [lo, hi] grown by `out` metres on every side, quaternions of norm 0.1 .. 10"""
    lo, hi = np.asarray(lo, float) - out, np.asarray(hi, float) + out
    q = rng.randn(N, 4)
    q *= (10.0 ** rng.uniform(-1, 1, N) / np.linalg.norm(q, axis=1))[:, None]
    return np.concatenate([lo + rng.rand(N, 3) * (hi - lo), q], axis=1)


# ---- 1. against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["scatter64", "partial64", "ragged32"])
def test_body_query_equals_the_model(hip_lib, scene):
    if scene == "scatter64":
        m, _ = dense_map(64)
        lo, hi = np.zeros(3), np.full(3, 6.4)
    elif scene == "partial64":
        m, _ = dense_map(64, obstacles=300, seed=2, hidden_blocks=12)
        lo, hi = np.zeros(3), np.full(3, 6.4)
    else:
        m, _ = dense_map(32, res=0.2, origin=(-3.2, -3.2, 0.0), obstacles=120, seed=11)
        lo = np.array([-3.2, -3.2, 0.0])
        hi = lo + 6.4
    rng = np.random.RandomState(len(scene))
    outside = unknown = below = 0
    for K in KS:
        sph = random_body(rng, K)
        poses = random_poses(rng, 33 if K == 1024 else 257, lo, hi)
        for margin in ((0.4,) if K in (130, 1024) else (0.4, -2.0)):
            want = model_of(m, sph, poses, margin)
            assert_model(m.BodyQuery(sph, poses, margin), want, f"{scene} K {K} margin {margin}")
            if margin == -2.0:
                assert not want["cost"].any() and not want["grad"].any() and not want["n_below"].any()
                continue
            s = want["sphere_clearance"] + sph[None, :, 3]
            outside += int(np.count_nonzero(np.abs(s + 1.0) < 1e-9))
            unknown += int(np.count_nonzero(s > 1000.0))
            below += int(np.count_nonzero(want["n_below"] > 0))
    # against an empty test: spheres left the map, sat in never-observed blocks, and many poses are penalised
    assert outside > 100 and below > 500 and (unknown > 100 or scene != "partial64"), (outside, unknown, below)
    m.close()


# ---- 2. team and batch edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_team_and_batch_edges_and_both_variants(hip_lib):
    m, _ = dense_map(64)
    rng = np.random.RandomState(7)
    for K in (1, 3, 8, 65):
        sph = random_body(rng, K)
        poses = random_poses(rng, 257, np.zeros(3), np.full(3, 6.4))
        big = device_call(m, sph, poses, 0.4)
        assert_model(big, model_of(m, sph, poses, 0.4), f"K {K}")
        assert_bits(device_call(m, sph, poses, 0.4), big, what=f"K {K} the same call again")            # repeatability
        for n in (1, 63, 64, 65, 257):
            part = device_call(m, sph, poses[:n], 0.4, rows=260)
            assert_bits({k: v[:n] for k, v in part.items()}, {k: v[:n] for k, v in big.items()}, what=f"K {K} first {n} poses")
            for k, v in part.items():
                assert np.all(v[n:] == SENTINEL), f"K {K} first {n} poses: {k} written past n_poses"
            assert_bits(m.BodyQuery(sph, poses[:n], 0.4), {k: v[:n] for k, v in big.items()}, what=f"K {K} host variant, {n} poses")
        # a pose's bits do not depend on where it stands in the batch
        perm = rng.permutation(257)
        moved = device_call(m, sph, poses[perm], 0.4)
        assert_bits(moved, {k: v[perm] for k, v in big.items()}, what=f"K {K} permuted batch")
    m.close()


def modal(a):
    """the entries that hold the array's most frequent value"""
    vals, counts = np.unique(a, return_counts=True)
    return a == vals[np.argmax(counts)]


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_name_the_lowest_sphere(hip_lib):
    """the wall map's distance grows with y alone: spheres on one plane y = const under the identity rotation tie wherever the
    interpolation returns the plane's value exactly.  Such spheres are picked with the map's own point query, 130 of them"""
    m = wall_map()
    rng = np.random.RandomState(3)
    pose = np.array([[3.2, 2.6, 3.2, 1.0, 0.0, 0.0, 0.0], [3.0, 3.4, 3.1, 7.5, 0.0, 0.0, 0.0]])
    cand = np.stack([rng.uniform(-0.7, 0.7, 600), np.full(600, 0.25), rng.uniform(-0.7, 0.7, 600), np.full(600, 0.1)], 1)
    s = model_of(m, cand, pose, 0.5)["sphere_clearance"]
    tied = modal(s[0]) & modal(s[1])
    assert tied.sum() >= 130, tied.sum()
    sph = cand[tied][:130]
    for table in (sph, sph[rng.permutation(130)], sph[::-1]):
        want = model_of(m, table, pose, 0.5)
        assert np.all(want["sphere_clearance"] == want["sphere_clearance"][:, :1]) and np.all(want["min_sphere"] == 0)
        for got in (m.BodyQuery(table, pose, 0.5), device_call(m, table, pose, 0.5)):
            assert_model(got, want, "ties")
            assert np.all(got["min_sphere"] == 0) and np.array_equal(got["min_pos"], pose[:, :3] + table[0, :3])
    sph[77, 1] = 0.2      # one sphere strictly closer to the wall: it wins wherever it stands
    assert np.all(m.BodyQuery(sph, pose, 0.5)["min_sphere"] == 77)
    m.close()


# ---- 4. null outputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_null_outputs(hip_lib):
    from fiesta_amd._lib import BodyResult
    m, _ = dense_map(32, obstacles=40)
    rng = np.random.RandomState(4)
    sph, poses = random_body(rng, 5, across=1.0), random_poses(rng, 70, np.zeros(3), np.full(3, 3.2))
    poses[9, 3:] = 0.0       # (an invalid pose: its branch honours the nulls too)
    full = device_call(m, sph, poses, 0.4)
    for name in ALL:
        got = device_call(m, sph, poses, 0.4, skip=(name,))
        assert np.all(got[name] == SENTINEL), name
        assert_bits(got, full, [k for k in ALL if k != name], f"without {name}")
    none = device_call(m, sph, poses, 0.4, skip=ALL)
    assert all(np.all(v == SENTINEL) for v in none.values())
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    empty = BodyResult()
    assert m._lib.fiesta_hip_body_query(m._h, p(sph), 5, p(poses), 70, 0.4, C.byref(empty)) == 0       # the host variant, all null
    cost = np.zeros(70)
    only = BodyResult(None, None, None, None, None, cost.ctypes.data, None, None)
    assert m._lib.fiesta_hip_body_query(m._h, p(sph), 5, p(poses), 70, 0.4, C.byref(only)) == 0
    assert np.array_equal(bits(cost), bits(full["cost"]))
    m.close()


# ---- 5. hash-block map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hash_block_map_both_variants(hip_lib):
    m, rng = hash_map_scene()
    lo, hi = np.array([-2.0, -2.0, -1.0]), np.array([4.1, 3.1, 2.1])          # the observed box; the poses' box is 1 m larger
    unknown = 0
    for K in (1, 8, 65, 130):
        sph = random_body(rng, K)
        poses = random_poses(rng, 257, lo, hi, out=1.0)
        want = model_of(m, sph, poses, 0.4)
        assert_model(m.BodyQuery(sph, poses, 0.4), want, f"hash host K {K}")
        dev = device_call(m, sph, poses, 0.4)
        assert_model(dev, want, f"hash dev K {K}")
        assert_bits(dev, m.BodyQuery(sph, poses, 0.4), what=f"hash K {K} variants")
        unknown += int(np.count_nonzero(want["sphere_clearance"] > 1000.0))
    assert unknown > 1000 and np.count_nonzero(want["n_below"] > 0) > 50        # spheres on tiles without a page; penalised poses
    m.close()


# ---- 6. every engine -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["cells", "envelope", "rounds", "levels", "masked"])
def test_engines(hip_lib, engine):
    from planner_probe import RES, SHAPE
    from test_gpu_planner_map_states import dense_for
    m = dense_for(engine, full=engine in ("cells", "envelope"))    # (these two serve fully observed maps only)
    rng = np.random.RandomState(len(engine))
    for K in (8, 65):
        sph = random_body(rng, K, across=1.0)
        poses = random_poses(rng, 150, np.zeros(3), np.array(SHAPE) * RES, out=0.2)
        want = model_of(m, sph, poses, 0.4)
        assert np.count_nonzero(want["n_below"] > 0) > 20
        assert_model(m.BodyQuery(sph, poses, 0.4), want, f"{engine} K {K}")
    m.close()


# ---- 7. stale field ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["dense", "hash"])
def test_field_not_yet_updated(hip_lib, store):
    """a bar of five spheres along x; an obstacle appears three voxels beside sphere 3: before UpdateESDF the call answers from the
    old field, afterwards from the new one, and min_sphere names sphere 3"""
    if store == "dense":
        m, _ = dense_map(64, obstacles=1)
        cands = [(32, 32, 32), (12, 12, 12), (50, 50, 12), (12, 50, 50)]
    else:
        m, _ = hash_map_scene(obstacles=1)
        cands = [(10, 5, 5), (-10, -10, 0), (30, 20, 10), (30, -10, 10)]
    vox = np.array(max(cands, key=lambda v: m.GetDistance(np.array([v], np.int32))[0]), np.int32)     # far from the scene's obstacle
    centre = (vox + 0.5) * 0.1                      # sphere 3 stands on this voxel's centre
    sph = np.array([[-0.4, 0, 0, 0.05], [-0.2, 0, 0, 0.05], [0.0, 0, 0, 0.05], [0.2, 0, 0, 0.05], [0.4, 0, 0, 0.05]])
    pose = np.array([[centre[0] - 0.2, centre[1], centre[2], 2.0, 0.0, 0.0, 0.0]])
    before = m.BodyQuery(sph, pose, 0.6)
    assert_model(before, model_of(m, sph, pose, 0.6), f"{store} before")
    assert before["min_clearance"][0] > 0.6 and before["cost"][0] == 0
    new = (vox + (0, 3, 0))[None].astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(new, 1, want_ret=False)
        m.UpdateOccupancy(True)
    stale = m.BodyQuery(sph, pose, 0.6)
    assert_bits(stale, before, what=f"{store} before UpdateESDF")
    assert_bits(device_call(m, sph, pose, 0.6), before, what=f"{store} before UpdateESDF, device variant")
    m.UpdateESDF()
    after = m.BodyQuery(sph, pose, 0.6)
    assert_model(after, model_of(m, sph, pose, 0.6), f"{store} after")
    assert after["min_sphere"][0] == 3 and 0.2 < after["min_clearance"][0] < 0.3 and after["n_below"][0] >= 3 and after["cost"][0] > 0
    assert after["grad"][0, 1] > 0          # the cost falls as the body moves away from the obstacle, towards -y
    m.close()


# ---- 8. invalid poses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_poses_inside_a_batch(hip_lib):
    m, _ = dense_map(64)
    rng = np.random.RandomState(8)
    for K in (3, 8, 65):
        sph = random_body(rng, K)
        poses = random_poses(rng, 257, np.zeros(3), np.full(3, 6.4))
        clean = device_call(m, sph, poses, 0.4)
        bad = poses.copy()
        bad[0, 3:] = 0.0                 # a zero quaternion
        bad[63, 1] = np.nan
        bad[64, 5] = np.inf
        bad[256, 3:] = (1e-160, 0, 0, 0)  # k overflows
        bad[100, 0] = -np.inf
        bad[101, 3:] = 1e-200            # s underflows to 0
        where = [0, 63, 64, 100, 101, 256]
        want = model_of(m, sph, bad, 0.4)
        for got in (device_call(m, sph, bad, 0.4), m.BodyQuery(sph, bad, 0.4)):
            assert_model(got, want, f"invalid poses K {K}")
            keep = np.setdiff1d(np.arange(257), where)
            assert_bits({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()}, what=f"K {K} the valid poses")
            assert np.all(got["min_sphere"][where] == -1) and np.all(got["n_below"][where] == -1) and not got["grad"][where].any()
            assert np.isnan(got["min_clearance"][where]).all() and np.isnan(got["cost"][where]).all()
            assert np.isnan(got["min_pos"][where]).all() and np.isnan(got["min_grad"][where]).all() and np.isnan(got["sphere_clearance"][where]).all()
    m.close()


# ---- 9. whole-call errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_call_errors(hip_lib):
    from fiesta_amd._lib import BodyResult
    m, _ = dense_map(32, obstacles=30)
    lib = m._lib
    rng = np.random.RandomState(9)
    sph, poses = random_body(rng, 4, across=1.0), random_poses(rng, 20, np.zeros(3), np.full(3, 3.2))
    ref = m.BodyQuery(sph, poses, 0.4)
    cost = np.zeros(20)
    res = BodyResult(None, None, None, None, None, cost.ctypes.data, None, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    many = np.zeros((1025, 4))

    def with_sphere(row, col, v):
        t = sph.copy()
        t[row, col] = v
        return t
    inf, nan = float("inf"), float("nan")
    bad_calls = [("null map", (None, p(sph), 4, p(poses), 20, 0.4, C.byref(res))),
                 ("n_spheres", (m._h, p(sph), 0, p(poses), 20, 0.4, C.byref(res))),
                 ("n_spheres", (m._h, p(sph), -1, p(poses), 20, 0.4, C.byref(res))),
                 ("n_spheres", (m._h, p(many), 1025, p(poses), 20, 0.4, C.byref(res))),
                 ("negative count", (m._h, p(sph), 4, p(poses), -1, 0.4, C.byref(res))),
                 ("spheres is null", (m._h, None, 4, p(poses), 20, 0.4, C.byref(res))),
                 ("poses is null", (m._h, p(sph), 4, None, 20, 0.4, C.byref(res))),
                 ("result is null", (m._h, p(sph), 4, p(poses), 20, 0.4, None)),
                 ("not finite", (m._h, p(with_sphere(2, 0, nan)), 4, p(poses), 20, 0.4, C.byref(res))),
                 ("not finite", (m._h, p(with_sphere(3, 2, inf)), 4, p(poses), 20, 0.4, C.byref(res))),
                 ("not finite", (m._h, p(with_sphere(0, 3, inf)), 4, p(poses), 20, 0.4, C.byref(res))),
                 ("not finite", (m._h, p(with_sphere(1, 3, nan)), 4, p(poses), 20, 0.4, C.byref(res))),
                 ("radius is negative", (m._h, p(with_sphere(1, 3, -1e-9)), 4, p(poses), 20, 0.4, C.byref(res))),
                 ("margin", (m._h, p(sph), 4, p(poses), 20, nan, C.byref(res))),
                 ("margin", (m._h, p(sph), 4, p(poses), 20, inf, C.byref(res))),
                 ("margin", (m._h, p(sph), 4, p(poses), 20, -inf, C.byref(res)))]
    for fn in (lib.fiesta_hip_body_query, lib.fiesta_hip_body_query_dev):       # (the checks come before any pointer is used)
        for word, args in bad_calls:
            cost[:] = SENTINEL
            assert fn(*args) == 1, (word, args)                                  # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
            assert np.all(cost == SENTINEL)
            assert_bits(m.BodyQuery(sph, poses, 0.4), ref, what=f"a good call after '{word}'")      # the map is still usable
    assert lib.fiesta_hip_body_query(m._h, p(sph), 4, None, 0, 0.4, C.byref(res)) == 0                # n_poses = 0 does nothing
    assert lib.fiesta_hip_body_query_dev(m._h, p(sph), 4, None, 0, 0.4, C.byref(res)) == 0 and np.all(cost == SENTINEL)
    assert lib.fiesta_hip_body_query(m._h, p(many[:1024]), 1024, p(poses), 20, 0.4, C.byref(res)) == 0   # 1024 spheres of radius 0 are fine
    assert lib.fiesta_hip_version() == 101
    m.close()


# ---- 10. what the gradient is for ----------------------------------------------------------------------------------------------------
def turned(pose, theta):
    """the pose after R <- exp([theta]x) R"""
    ang = float(np.linalg.norm(theta))
    w, v = math.cos(ang / 2), math.sin(ang / 2) * np.asarray(theta) / ang
    qw, q = pose[3], pose[4:7]
    out = np.array(pose, np.float64)
    out[3] = w * qw - v @ q
    out[4:7] = w * q + qw * v + np.cross(v, q)
    return out


@pytest.mark.gpu
def test_gradient_descends(hip_lib):
    """the bar of examples/body_check.cpp diagonally in its doorway, a little off the middle: 1 cm along -grad[:3], and separately
    0.01 rad about -grad[3:], each lowers the cost the call reports"""
    from test_cpp_skeleton import example_scene
    m = example_scene()
    bar = np.array([[0.1 * i, 0.0, 0.0, 0.15] for i in range(-3, 4)])
    pose = np.array([0.1, 0.08, 2.0, math.cos(math.pi / 8), 0.0, 0.0, math.sin(math.pi / 8)])
    r = m.BodyQuery(bar, pose[None], 0.4)
    g = r["grad"][0]
    assert r["cost"][0] > 0.05 and np.linalg.norm(g[:3]) > 0.1 and np.linalg.norm(g[3:]) > 0.05, (r["cost"], g)
    moved = pose.copy()
    moved[:3] -= 0.01 * g[:3] / np.linalg.norm(g[:3])
    after = m.BodyQuery(bar, np.stack([moved, turned(pose, -0.01 * g[3:] / np.linalg.norm(g[3:]))]), 0.4)["cost"]
    print(f"cost {r['cost'][0]:.6f}; after the step {after[0]:.6f}, after the turn {after[1]:.6f}")
    assert after[0] < r["cost"][0] and after[1] < r["cost"][0]
    m.close()


# ---- 11. resources (the built library only: no GPU) ----------------------------------------------------------------------------------
def test_body_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_body_" in k}
    assert len(res) == 2 and sum("DensePathEval" in k for k in res) == 1 and sum("HashPathEval" in k for k in res) == 1, sorted(res)
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    copies = check_kernel_resources.kernel_copies(so)
    assert all(len(copies[k]) == 1 for k in res)        # compiled once, in planner.hip
