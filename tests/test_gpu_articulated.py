"""Articulated body queries on the device (fiesta_hip_articulated_query / _dev, include/fiesta_hip.h) against
fiesta_amd.articulated_query_model over the map's own point query.

The exact outputs (sphere_clearance, frame_clearance, min_clearance, min_sphere, min_pos, min_grad, n_below) are compared by bits,
cost, frame_cost and frame_grad within the header's bound (n + 16) * 2^-52 * A, the NaN pattern exactly.  Then what the rule cannot
show: frame layouts against the team size and the pass boundaries, batch edges, both variants and both stores, the rigid call on one
frame, ties across frames, the stale field, invalid frame poses inside a batch, the whole-call errors and what the per-frame
gradient is for.  The resource test needs the built library only.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_gpu_body_query import assert_bits as assert_bits_of, bits, bound, modal, random_body, random_poses, turned
from test_gpu_path_cost import hash_map_scene
from test_gpu_path_queries import dense_map, wall_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "frame_clearance", "sphere_clearance")
SUMS = ("cost", "frame_cost", "frame_grad")
ALL = EXACT + SUMS
SENTINEL = -7


def assert_bits(got, want, keys=ALL, what=""):
    assert_bits_of(got, want, keys, what)


def sizes(*counts):
    """the frame index per sphere of frames with these sphere counts"""
    return np.repeat(np.arange(len(counts)), counts).astype(np.int32)


def only(frame, n_frames):
    """one sphere, on `frame` of n_frames"""
    counts = [0] * n_frames
    counts[frame] = 1
    return sizes(*counts)


# (K, F, frame index per sphere): the team sizes 1 .. 64, one and many passes, frame boundaries on and inside a pass, empty frames
LAYOUTS = [("1x1", sizes(1)), ("1 of 64", only(37, 64)), ("3 on 2", sizes(2, 1)), ("8 on 8", sizes(*[1] * 8)), ("64 on 64", sizes(*[1] * 64)),
           ("65: 64|1", sizes(64, 1)), ("65: 41|24", sizes(41, 24)), ("130 on 7", sizes(30, 1, 0, 45, 20, 33, 1)), ("1024 on 64", sizes(*[16] * 64))]
N_FRAMES = {"1x1": 1, "1 of 64": 64, "3 on 2": 2, "8 on 8": 8, "64 on 64": 64, "65: 64|1": 2, "65: 41|24": 2, "130 on 7": 7, "1024 on 64": 64}


def model_of(m, sph, frm, F, poses, margin):
    import fiesta_amd
    return fiesta_amd.articulated_query_model(m.GetDistWithGradTrilinear, sph, frm, F, poses, margin)


def assert_model(got, model, what=""):
    """the exact outputs by bits (NaN included), the sums within the bound of the model's (n, A), NaN exactly where the model has it"""
    assert_bits(got, model, EXACT, what)
    worst = {}
    for k in SUMS:
        a, b = np.asarray(got[k], np.float64), model[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        n = model[k + "_n"]
        lim = bound(n[:, :, None] if k == "frame_grad" else n, model[k + "_abs"])
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what} {k}: NaN pattern differs"
        err = np.where(np.isnan(b), 0.0, np.abs(a - b))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[k] = float(np.nanmax(np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0)), initial=0.0))
        bad = np.argwhere(err > lim)
        assert len(bad) == 0, (f"{what} {k}: {len(bad)} entries beyond the bound, first {bad[:3].tolist()}: got {a[tuple(bad[0])]!r} "
                               f"want {b[tuple(bad[0])]!r} bound {lim[tuple(bad[0])]!r}")
    print(f"{what}: worst error / bound  " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def device_call(m, sph, frm, F, poses, margin, rows=None, skip=(), fill=SENTINEL):
    """fiesta_hip_articulated_query_dev on torch tensors of `rows` rows (default: one per configuration), every output pre-filled
    with `fill`; the fields named in `skip` are passed as null"""
    import torch
    from fiesta_amd.esdf_map import ARTICULATED_FIELDS
    dev = torch.device("cuda", 0)
    sph = np.ascontiguousarray(sph, np.float64).reshape(-1, 4)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, F, 7)
    rows = len(P) if rows is None else rows
    dims = {"K": len(sph), "F": F}
    pt = torch.from_numpy(P).to(dev) if len(P) else torch.zeros((1, F, 7), dtype=torch.float64, device=dev)
    outs = {name: torch.full((rows,) + tuple(dims.get(d, d) for d in shape), fill,
                             dtype=torch.float64 if dt == np.float64 else torch.int32, device=dev) for name, dt, shape in ARTICULATED_FIELDS}
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the fills above must have landed)
    m.ArticulatedQueryDevice(sph, frm, F, pt.data_ptr(), len(P), margin, {k: v.data_ptr() for k, v in outs.items() if k not in skip})
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def random_links(rng, frm, across=0.8):
    """per sphere a centre inside a ball `across` metres wide about its frame's origin, radii up to 0.15 m"""
    return random_body(rng, len(frm), across)


def random_configs(rng, N, F, lo, hi, out=0.4, reach=0.5):
    """a base position per configuration in the box [lo, hi] grown by `out`; every frame within `reach` metres of it on every axis,
    with a quaternion of its own of norm 0.1 .. 10"""
    base = random_poses(rng, N, lo, hi, out)[:, None, :3]
    poses = random_poses(rng, N * F, np.zeros(3), np.zeros(3), out=reach).reshape(N, F, 7)
    poses[:, :, :3] += base
    return poses


# ---- 1. against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["scatter64", "partial64", "ragged32"])
def test_articulated_query_equals_the_model(hip_lib, scene):
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
    for name, frm in LAYOUTS:
        K, F = len(frm), N_FRAMES[name]
        sph = random_links(rng, frm)
        poses = random_configs(rng, 33 if K == 1024 else 257, F, lo, hi)
        for margin in (0.4, -2.0):
            want = model_of(m, sph, frm, F, poses, margin)
            got = m.ArticulatedQuery(sph, frm, poses, margin)
            assert_model(got, want, f"{scene} {name} margin {margin}")
            empty = np.bincount(frm, minlength=F) == 0
            assert np.all(got["frame_clearance"][:, empty] == np.inf) and not got["frame_cost"][:, empty].any()
            if margin == -2.0:      # nothing is penalised: every sum is exactly 0
                assert not got["cost"].any() and not got["frame_cost"].any() and not got["frame_grad"].any() and not got["n_below"].any()
                continue
            s = want["sphere_clearance"] + sph[None, :, 3]
            outside += int(np.count_nonzero(np.abs(s + 1.0) < 1e-9))
            unknown += int(np.count_nonzero(s > 1000.0))
            below += int(np.count_nonzero(want["n_below"] > 0))
    print(f"{scene}: {outside} spheres outside the map, {unknown} in never-observed space, {below} configurations penalised")
    # against an empty test: spheres left the map, sat in never-observed blocks, and many configurations are penalised
    assert outside > 100 and below > 500 and (unknown > 100 or scene != "partial64"), (outside, unknown, below)
    m.close()


# ---- 2. one frame is the rigid call --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_frame_equals_the_body_query(hip_lib):
    m, _ = dense_map(64)
    rng = np.random.RandomState(2)
    for K in (1, 8, 65, 130):
        sph = random_body(rng, K)
        poses = random_poses(rng, 257, np.zeros(3), np.full(3, 6.4))
        poses[5, 3:] = 0.0
        rigid = m.BodyQuery(sph, poses, 0.4)
        got = m.ArticulatedQuery(sph, np.zeros(K, np.int32), poses[:, None, :], 0.4)
        assert_bits(got, rigid, ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "sphere_clearance"), f"K {K}")
        assert np.array_equal(bits(got["frame_clearance"][:, 0]), bits(rigid["min_clearance"]))
        from fiesta_amd import body_query_model
        ref = body_query_model(m.GetDistWithGradTrilinear, sph, poses, 0.4)
        for mine, theirs, lim in ((got["cost"], rigid["cost"], bound(K, ref["cost_abs"])), (got["frame_cost"][:, 0], rigid["cost"], bound(K, ref["cost_abs"])),
                                  (got["frame_grad"][:, 0], rigid["grad"], bound(K, ref["grad_abs"]))):
            assert np.array_equal(np.isnan(mine), np.isnan(theirs))
            assert np.all(np.where(np.isnan(theirs), 0.0, np.abs(mine - theirs)) <= lim), K
        assert np.count_nonzero(rigid["n_below"] > 0) > 20
    m.close()


# ---- 3. batch edges and variants -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_edges_and_both_variants(hip_lib):
    m, _ = dense_map(64)
    rng = np.random.RandomState(7)
    for name in ("1 of 64", "3 on 2", "8 on 8", "65: 41|24"):
        frm, F = dict(LAYOUTS)[name], N_FRAMES[name]
        sph = random_links(rng, frm)
        poses = random_configs(rng, 257, F, np.zeros(3), np.full(3, 6.4))
        big = device_call(m, sph, frm, F, poses, 0.4)
        assert_model(big, model_of(m, sph, frm, F, poses, 0.4), name)
        assert_bits(device_call(m, sph, frm, F, poses, 0.4), big, what=f"{name} the same call again")            # repeatability
        for n in (1, 63, 64, 65, 257):
            part = device_call(m, sph, frm, F, poses[:n], 0.4, rows=260)
            assert_bits({k: v[:n] for k, v in part.items()}, {k: v[:n] for k, v in big.items()}, what=f"{name} first {n} configurations")
            for k, v in part.items():
                assert np.all(v[n:] == SENTINEL), f"{name} first {n} configurations: {k} written past n_configs"
            assert_bits(m.ArticulatedQuery(sph, frm, poses[:n], 0.4), {k: v[:n] for k, v in big.items()}, what=f"{name} host variant, {n}")
        # a configuration's bits do not depend on where it stands in the batch
        perm = rng.permutation(257)
        moved = device_call(m, sph, frm, F, poses[perm], 0.4)
        assert_bits(moved, {k: v[perm] for k, v in big.items()}, what=f"{name} permuted batch")
    m.close()


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_name_the_lowest_sphere_across_frames(hip_lib):
    """the rigid tie test's construction (spheres on one plane y = const of the wall map, identity rotation, picked where the map's
    own point query ties), the 130 tied spheres split over three frames of identical pose"""
    m = wall_map()
    rng = np.random.RandomState(3)
    pose = np.array([[3.2, 2.6, 3.2, 1.0, 0.0, 0.0, 0.0], [3.0, 3.4, 3.1, 7.5, 0.0, 0.0, 0.0]])
    cand = np.stack([rng.uniform(-0.7, 0.7, 600), np.full(600, 0.25), rng.uniform(-0.7, 0.7, 600), np.full(600, 0.1)], 1)
    from fiesta_amd import body_query_model
    s = body_query_model(m.GetDistWithGradTrilinear, cand, pose, 0.5)["sphere_clearance"]
    tied = modal(s[0]) & modal(s[1])
    assert tied.sum() >= 130, tied.sum()
    sph, frm = cand[tied][:130], sizes(43, 43, 44)
    poses = np.repeat(pose[:, None, :], 3, axis=1)
    for table in (sph, sph[rng.permutation(130)], sph[::-1]):
        want = model_of(m, table, frm, 3, poses, 0.5)
        assert np.all(want["sphere_clearance"] == want["sphere_clearance"][:, :1]) and np.all(want["min_sphere"] == 0)
        for got in (m.ArticulatedQuery(table, frm, poses, 0.5), device_call(m, table, frm, 3, poses, 0.5)):
            assert_model(got, want, "ties")
            assert np.all(got["min_sphere"] == 0) and np.array_equal(got["min_pos"], pose[:, :3] + table[0, :3])
            assert np.all(got["frame_clearance"] == got["min_clearance"][:, None])
    sph[77, 1] = 0.2      # one sphere of the middle frame strictly closer to the wall: it wins wherever it stands
    got = m.ArticulatedQuery(sph, frm, poses, 0.5)
    assert np.all(got["min_sphere"] == 77) and np.all(got["frame_clearance"][:, 1] < got["frame_clearance"][:, 0])
    m.close()


# ---- 5. null outputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_null_outputs(hip_lib):
    from fiesta_amd._lib import ArticulatedResult
    m, _ = dense_map(32, obstacles=40)
    rng = np.random.RandomState(4)
    frm, F = sizes(2, 0, 3), 3
    sph, poses = random_links(rng, frm), random_configs(rng, 70, F, np.zeros(3), np.full(3, 3.2))
    poses[9, 1, 3:] = 0.0       # (an invalid configuration: its branch honours the nulls too)
    full = device_call(m, sph, frm, F, poses, 0.4)
    assert np.isnan(full["cost"][9]) and np.isnan(full["frame_cost"][9]).all()
    for name in ALL:
        got = device_call(m, sph, frm, F, poses, 0.4, skip=(name,))
        assert np.all(got[name] == SENTINEL), name
        assert_bits(got, full, [k for k in ALL if k != name], f"without {name}")
    none = device_call(m, sph, frm, F, poses, 0.4, skip=ALL)
    assert all(np.all(v == SENTINEL) for v in none.values())
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    empty = ArticulatedResult()
    assert m._lib.fiesta_hip_articulated_query(m._h, p(sph), p(frm), 5, F, p(poses), 70, 0.4, C.byref(empty)) == 0    # the host variant, all null
    cost = np.zeros(70)
    one = ArticulatedResult(None, None, None, None, None, cost.ctypes.data, None, None, None, None)
    assert m._lib.fiesta_hip_articulated_query(m._h, p(sph), p(frm), 5, F, p(poses), 70, 0.4, C.byref(one)) == 0
    assert np.array_equal(bits(cost), bits(full["cost"]))
    m.close()


# ---- 6. hash-block map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hash_block_map_both_variants(hip_lib):
    m, rng = hash_map_scene()
    lo, hi = np.array([-2.0, -2.0, -1.0]), np.array([4.1, 3.1, 2.1])          # the observed box; the base positions' box is 1 m larger
    unknown = 0
    for name in ("1 of 64", "8 on 8", "65: 41|24", "130 on 7"):
        frm, F = dict(LAYOUTS)[name], N_FRAMES[name]
        sph = random_links(rng, frm)
        poses = random_configs(rng, 257, F, lo, hi, out=1.0)
        want = model_of(m, sph, frm, F, poses, 0.4)
        host = m.ArticulatedQuery(sph, frm, poses, 0.4)
        assert_model(host, want, f"hash host {name}")
        dev = device_call(m, sph, frm, F, poses, 0.4)
        assert_model(dev, want, f"hash dev {name}")
        assert_bits(dev, host, what=f"hash {name} variants")
        unknown += int(np.count_nonzero(want["sphere_clearance"] > 1000.0))
    assert unknown > 1000 and np.count_nonzero(want["n_below"] > 0) > 50        # spheres on tiles without a page; penalised configurations
    m.close()


# ---- 7. stale field ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["dense", "hash"])
def test_field_not_yet_updated(hip_lib, store):
    """a bar in two parts: frame 0 (three spheres) stands far off, frame 1 (two spheres) where an obstacle appears three voxels
    beside its first sphere.  Before UpdateESDF the call answers from the old field; afterwards min_sphere lies on frame 1, and
    frame 0, which is closer to the scene's old obstacle than to the new one, reads what it read before"""
    if store == "dense":
        m, _ = dense_map(64, obstacles=1)
        cands = [(32, 32, 32), (12, 12, 12), (50, 50, 12), (12, 50, 50)]
    else:
        m, _ = hash_map_scene(obstacles=1)
        cands = [(10, 5, 5), (-10, -10, 0), (30, 20, 10), (30, -10, 10)]
    cands = np.array(cands, np.int32)
    d_old = m.GetDistance(cands)
    vox = cands[np.argmax(d_old)]                   # frame 1: far from the scene's obstacle
    new = (vox + (0, 3, 0))[None].astype(np.int32)
    score = np.linalg.norm(cands - new[0], axis=1) * 0.1 - d_old
    other = cands[np.argmax(score)]                 # frame 0: much closer to the old obstacle than to the new one
    assert score.max() > 1.2 and d_old[np.argmax(score)] > 0.9, (score, d_old)
    frm = sizes(3, 2)
    sph = np.array([[-0.2, 0, 0, 0.05], [0.0, 0, 0, 0.05], [0.2, 0, 0, 0.05], [0.0, 0, 0, 0.05], [0.2, 0, 0, 0.05]])
    poses = np.array([[list((other + 0.5) * 0.1) + [2.0, 0.0, 0.0, 0.0], list((vox + 0.5) * 0.1) + [2.0, 0.0, 0.0, 0.0]]])
    before = m.ArticulatedQuery(sph, frm, poses, 0.6)
    assert_model(before, model_of(m, sph, frm, 2, poses, 0.6), f"{store} before")
    assert before["min_clearance"][0] > 0.6 and before["cost"][0] == 0
    for _ in range(3):
        m.SetOccupancy(new, 1, want_ret=False)
        m.UpdateOccupancy(True)
    stale = m.ArticulatedQuery(sph, frm, poses, 0.6)
    assert_bits(stale, before, what=f"{store} before UpdateESDF")
    assert_bits(device_call(m, sph, frm, 2, poses, 0.6), before, what=f"{store} before UpdateESDF, device variant")
    m.UpdateESDF()
    after = m.ArticulatedQuery(sph, frm, poses, 0.6)
    assert_model(after, model_of(m, sph, frm, 2, poses, 0.6), f"{store} after")
    assert after["min_sphere"][0] == 3 and frm[after["min_sphere"][0]] == 1 and 0.2 < after["min_clearance"][0] < 0.3
    assert after["n_below"][0] == 2 and after["cost"][0] > 0 and after["frame_cost"][0, 1] > 0 and after["frame_cost"][0, 0] == 0
    assert np.array_equal(bits(after["frame_clearance"][:, 0]), bits(before["frame_clearance"][:, 0]))
    assert after["frame_grad"][0, 1, 1] > 0 and not after["frame_grad"][0, 0].any()     # the cost falls as frame 1 moves towards -y
    m.close()


# ---- 8. invalid configurations -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_configurations_inside_a_batch(hip_lib):
    m, _ = dense_map(64)
    rng = np.random.RandomState(8)
    for frm in (sizes(2, 0, 1), sizes(3, 0, 2, 3), sizes(30, 0, 20, 15)):
        F, K = int(frm.max()) + 1, len(frm)
        sph = random_links(rng, frm)
        poses = random_configs(rng, 257, F, np.zeros(3), np.full(3, 6.4))
        clean = device_call(m, sph, frm, F, poses, 0.4)
        bad = poses.copy()
        bad[0, 0, 3:] = 0.0                     # a zero quaternion
        bad[63, 2, 1] = np.nan
        bad[64, F - 1, 5] = np.inf
        bad[256, 0, 3:] = (1e-160, 0, 0, 0)     # k overflows
        bad[100, 1, 0] = -np.inf                # frame 1 owns no sphere: it counts all the same
        bad[101, 2, 3:] = 1e-200                # s underflows to 0
        where = [0, 63, 64, 100, 101, 256]
        want = model_of(m, sph, frm, F, bad, 0.4)
        for got in (device_call(m, sph, frm, F, bad, 0.4), m.ArticulatedQuery(sph, frm, bad, 0.4)):
            assert_model(got, want, f"invalid configurations K {K}")
            keep = np.setdiff1d(np.arange(257), where)
            assert_bits({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()}, what=f"K {K} the valid configurations")
            assert np.all(got["min_sphere"][where] == -1) and np.all(got["n_below"][where] == -1) and not got["frame_grad"][where].any()
            assert np.isnan(got["min_clearance"][where]).all() and np.isnan(got["cost"][where]).all()
            assert np.isnan(got["min_pos"][where]).all() and np.isnan(got["min_grad"][where]).all() and np.isnan(got["sphere_clearance"][where]).all()
            assert np.isnan(got["frame_clearance"][where]).all() and np.isnan(got["frame_cost"][where]).all()
    m.close()


# ---- 9. whole-call errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_call_errors(hip_lib):
    from fiesta_amd._lib import ArticulatedResult
    m, _ = dense_map(32, obstacles=30)
    lib = m._lib
    rng = np.random.RandomState(9)
    frm, F = sizes(1, 2, 1), 3
    sph, poses = random_links(rng, frm), random_configs(rng, 20, F, np.zeros(3), np.full(3, 3.2))
    ref = m.ArticulatedQuery(sph, frm, poses, 0.4)
    cost = np.zeros(20)
    res = ArticulatedResult(None, None, None, None, None, cost.ctypes.data, None, None, None, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    many, many_f = np.zeros((1025, 4)), np.zeros(1025, np.int32)
    wide = np.tile(poses[:, :1], (1, 65, 1))

    def with_sphere(row, col, v):
        t = sph.copy()
        t[row, col] = v
        return t

    def frames(*v):
        return np.array(v, np.int32)
    inf, nan = float("inf"), float("nan")
    r = C.byref(res)
    bad_calls = [("null map", (None, p(sph), p(frm), 4, F, p(poses), 20, 0.4, r)),
                 ("n_spheres", (m._h, p(sph), p(frm), 0, F, p(poses), 20, 0.4, r)),
                 ("n_spheres", (m._h, p(sph), p(frm), -1, F, p(poses), 20, 0.4, r)),
                 ("n_spheres", (m._h, p(many), p(many_f), 1025, F, p(poses), 20, 0.4, r)),
                 ("n_frames", (m._h, p(sph), p(frm), 4, 0, p(poses), 20, 0.4, r)),
                 ("n_frames", (m._h, p(sph), p(frm), 4, -3, p(poses), 20, 0.4, r)),
                 ("n_frames", (m._h, p(sph), p(frm), 4, 65, p(wide), 20, 0.4, r)),
                 ("negative count", (m._h, p(sph), p(frm), 4, F, p(poses), -1, 0.4, r)),
                 ("spheres is null", (m._h, None, p(frm), 4, F, p(poses), 20, 0.4, r)),
                 ("sphere_frame is null", (m._h, p(sph), None, 4, F, p(poses), 20, 0.4, r)),
                 ("frame_poses is null", (m._h, p(sph), p(frm), 4, F, None, 20, 0.4, r)),
                 ("result is null", (m._h, p(sph), p(frm), 4, F, p(poses), 20, 0.4, None)),
                 ("not finite", (m._h, p(with_sphere(2, 0, nan)), p(frm), 4, F, p(poses), 20, 0.4, r)),
                 ("not finite", (m._h, p(with_sphere(3, 2, inf)), p(frm), 4, F, p(poses), 20, 0.4, r)),
                 ("not finite", (m._h, p(with_sphere(0, 3, inf)), p(frm), 4, F, p(poses), 20, 0.4, r)),
                 ("not finite", (m._h, p(with_sphere(1, 3, nan)), p(frm), 4, F, p(poses), 20, 0.4, r)),
                 ("radius is negative", (m._h, p(with_sphere(1, 3, -1e-9)), p(frm), 4, F, p(poses), 20, 0.4, r)),
                 ("frame index", (m._h, p(sph), p(frames(0, 1, 1, 3)), 4, F, p(poses), 20, 0.4, r)),
                 ("frame index", (m._h, p(sph), p(frames(-1, 1, 1, 2)), 4, F, p(poses), 20, 0.4, r)),
                 ("not grouped by frame", (m._h, p(sph), p(frames(0, 1, 0, 2)), 4, F, p(poses), 20, 0.4, r)),
                 ("not grouped by frame", (m._h, p(sph), p(frames(2, 1, 1, 0)), 4, F, p(poses), 20, 0.4, r)),
                 ("margin", (m._h, p(sph), p(frm), 4, F, p(poses), 20, nan, r)),
                 ("margin", (m._h, p(sph), p(frm), 4, F, p(poses), 20, inf, r)),
                 ("margin", (m._h, p(sph), p(frm), 4, F, p(poses), 20, -inf, r))]
    for fn in (lib.fiesta_hip_articulated_query, lib.fiesta_hip_articulated_query_dev):       # (the checks come before any pointer is used)
        for word, args in bad_calls:
            cost[:] = SENTINEL
            assert fn(*args) == 1, (word, args)                                  # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
            assert np.all(cost == SENTINEL)
            assert_bits(m.ArticulatedQuery(sph, frm, poses, 0.4), ref, what=f"a good call after '{word}'")      # the map is still usable
    assert lib.fiesta_hip_articulated_query(m._h, p(sph), p(frm), 4, F, None, 0, 0.4, r) == 0               # n_configs = 0 does nothing
    assert lib.fiesta_hip_articulated_query_dev(m._h, p(sph), p(frm), 4, F, None, 0, 0.4, r) == 0 and np.all(cost == SENTINEL)
    assert lib.fiesta_hip_articulated_query(m._h, p(many[:1024]), p(many_f[:1024]), 1024, F, p(poses), 20, 0.4, r) == 0   # 1024 spheres of radius 0
    assert lib.fiesta_hip_version() == 101
    m.close()


# ---- 10. what the per-frame gradient is for ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frame_gradient_descends(hip_lib):
    """the bar of examples/body_check.cpp cut in two links that meet in the doorway of its scene, each a little askew: for either
    link, 1 cm along -frame_grad[f, :3], and separately 0.01 rad about -frame_grad[f, 3:], with the other link fixed, lowers the
    cost the call reports"""
    from test_cpp_skeleton import example_scene
    m = example_scene()
    sph = np.array([[0.1 * i, 0.0, 0.0, 0.15] for i in range(1, 5)] * 2)
    frm = sizes(4, 4)
    a0, a1 = math.pi / 8, math.pi + math.pi / 3
    config = np.array([[0.1, 0.08, 2.0, math.cos(a0 / 2), 0.0, 0.0, math.sin(a0 / 2)],
                       [0.1, 0.08, 2.0, math.cos(a1 / 2), 0.0, 0.0, math.sin(a1 / 2)]])
    r = m.ArticulatedQuery(sph, frm, config[None], 0.4)
    cost = r["cost"][0]
    assert cost > 0.05 and np.all(r["frame_cost"][0] > 0.01), (cost, r["frame_cost"])
    trials = []
    for f in range(2):
        g = r["frame_grad"][0, f]
        assert np.linalg.norm(g[:3]) > 0.05 and np.linalg.norm(g[3:]) > 0.01, (f, g)
        moved, spun = config.copy(), config.copy()
        moved[f, :3] -= 0.01 * g[:3] / np.linalg.norm(g[:3])
        spun[f] = turned(config[f], -0.01 * g[3:] / np.linalg.norm(g[3:]))
        trials += [moved, spun]
    after = m.ArticulatedQuery(sph, frm, np.stack(trials), 0.4)["cost"]
    print(f"cost {cost:.6f}; after the steps and turns {after}")
    assert np.all(after < cost), (cost, after)
    m.close()


# ---- 11. resources (the built library only: no GPU) ----------------------------------------------------------------------------------
def test_articulated_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_artic_" in k}
    assert len(res) == 2 and sum("DensePathEval" in k for k in res) == 1 and sum("HashPathEval" in k for k in res) == 1, sorted(res)
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    copies = check_kernel_resources.kernel_copies(so)
    assert all(len(copies[k]) == 1 for k in res)        # compiled once, in planner.hip
    assert not any("k_body_" in k for k in res)
