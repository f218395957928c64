"""Batched path cost and waypoint gradients (fiesta_hip_path_cost[_dev], include/fiesta_hip.h; kernels:
fiesta_amd/csrc/path_cost_kernels.hpp).

The model is the point route an optimiser runs today: fiesta_amd.path_cost_model over GetDistWithGradTrilinear on the same map (the
header's formulas in numpy; tests/test_path_cost_rule.py checks it against a plain loop and against central differences).  Integers
are compared exactly.  Every float output X is compared with the model's (n, A) -- the number of summed terms and the sum of their
absolute values on X's scale: |X - X_model| <= (n + 16) * 2^-52 * A, the bound for reordering a sum of n identical terms with 16
terms' worth of room for the few operations after the sums.  It is derived, not measured: the terms themselves are bit-identical
by the header's operation order, only the order of summation differs.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from scenarios import P_DEFAULT
from test_gpu_path_queries import dense_map, make_paths, wall_map, zigzag

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = (1.0, 0.3, -2.0)
FLOATS = ("cost", "length", "grad")


def bound(n, a):
    return (np.asarray(n, np.float64) + 16.0) * 2.0 ** -52 * np.asarray(a, np.float64)


def model_of(m, w, off, step, margin):
    import fiesta_amd
    return fiesta_amd.path_cost_model(m.GetDistWithGradTrilinear, w, off, step, margin)


def assert_within(got, model, what=""):
    """integers exact, floats within the summation bound of the model's (n, A), NaN exactly where the model has NaN"""
    for k in ("n_samples", "n_below"):
        bad = np.nonzero(np.asarray(got[k]) != model[k])[0]
        assert len(bad) == 0, f"{what} {k}: {len(bad)} paths differ, first {bad[:5]}: got {got[k][bad[:3]]} want {model[k][bad[:3]]}"
    worst = {}
    for k in FLOATS:
        a, b = np.asarray(got[k], np.float64), model[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        lim = bound(model[k + "_n"] if k != "grad" else model["grad_n"][:, None], model[k + "_abs"])
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what} {k}: NaN pattern differs"
        err = np.where(np.isnan(b), 0.0, np.abs(a - b))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[k] = float(np.nanmax(np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0)), initial=0.0))
        bad = np.argwhere(err > lim)
        assert len(bad) == 0, (f"{what} {k}: {len(bad)} entries beyond the bound, first {bad[:3].tolist()}: got {a[tuple(bad[0])]!r} "
                               f"want {b[tuple(bad[0])]!r} bound {lim[tuple(bad[0])]!r}")
    print(f"{what}: worst error / bound  " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def assert_bits(got, want, what=""):
    for k, v in want.items():
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(v)
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), f"{what} {k}: bits differ"


def device_call(m, w, off, step, margin, fill=-7):
    """fiesta_hip_path_cost_dev on torch tensors; every output pre-filled with `fill`"""
    import torch
    from fiesta_amd.esdf_map import PATH_COST_FIELDS
    dev = torch.device("cuda", 0)
    w = np.ascontiguousarray(w, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(off, np.int64)
    wt, ot = torch.from_numpy(w).to(dev), torch.from_numpy(off).to(dev)
    outs = {name: torch.full(((len(off) - 1) if per == "path" else len(w),) + shape, fill,
                             dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
            for name, dt, per, shape in PATH_COST_FIELDS}
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the fills above must have landed)
    m.PathCostDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, step, margin, {k: v.data_ptr() for k, v in outs.items()})
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def hash_map_scene(obstacles=150, seed=4):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, reserve_size=100000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((-20, -20, -10), (40, 30, 20), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    rng = np.random.RandomState(seed)
    S = np.stack([rng.randint(-20, 41, obstacles), rng.randint(-20, 31, obstacles), rng.randint(-10, 21, obstacles)], 1).astype(np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m, rng


@pytest.mark.parametrize("scene", ["scatter64", "partial64", "ragged32", "hash"])
def test_path_cost_equals_the_point_route(hip_lib, scene):
    rng = np.random.RandomState(len(scene))
    if scene == "scatter64":
        m, _ = dense_map(64)
        lo, hi, res = np.zeros(3), np.full(3, 6.4), 0.1
    elif scene == "partial64":
        m, _ = dense_map(64, obstacles=300, seed=2, hidden_blocks=12)
        lo, hi, res = np.zeros(3), np.full(3, 6.4), 0.1
    elif scene == "ragged32":
        m, _ = dense_map(32, res=0.2, origin=(-3.2, -3.2, 0.0), obstacles=120, seed=11)
        lo, res = np.array([-3.2, -3.2, 0.0]), 0.2
        hi = lo + 6.4
    else:   # the observed box of the clearance tests' hash-block map; paths also leave it through unallocated blocks
        m, rng = hash_map_scene()
        lo, hi, res = np.array([-1.5, -1.5, -0.5]), np.array([3.5, 2.5, 1.5]), 0.1
    w, off = make_paths(rng, lo, hi, res)
    nwp = np.diff(off)
    saw_long = False
    for step in (0.25 * res, res, 3.7 * res):
        for margin in MARGINS:
            want = model_of(m, w, off, step, margin)
            got = m.PathCost(w, off, step, margin)
            assert_within(got, want, f"{scene} step {step:g} margin {margin}")
            saw_long |= bool(want["n_samples"].max() >= 100_000)
            valid = (want["n_samples"] > 0) & (nwp >= 2)
            if margin == 1.0:   # against an empty test, on the MODEL's output: most paths are penalised and pulled
                pulled = np.array([want["grad"][off[p]:off[p + 1]].any() for p in range(len(nwp))])
                share = np.count_nonzero(valid & (want["cost"] > 0) & pulled) / np.count_nonzero(valid)
                assert share >= 0.5, (scene, step, share)
            if margin == -2.0:
                assert not got["cost"][want["n_samples"] >= 0].any() and not got["grad"].any()
                assert (got["n_below"][want["n_samples"] >= 0] == 0).all()
    assert saw_long
    assert (want["n_samples"] == 0).any() and (want["n_samples"] == 1).any()     # empty and single-waypoint paths were there
    m.close()


def test_runs_of_one_sample_segments_and_segments_over_many_pieces(hip_lib):
    """the segmented scan at its ends: groups of 64 samples on 64 segments (zig-zag runs of one-sample segments between segments of
    2 ... 5), and segments of 10^4 ... 3 * 10^5 samples that span many pieces (their sums are folded from head / tail records), with a
    one-sample segment right after a long one; host and device variant"""
    m = wall_map()
    step = 0.05
    runs = [(3, 2), (1, 64), (4, 1), (1, 63), (2, 2), (1, 65), (5, 1), (1, 200), (3, 2), (1, 128), (2, 2)] * 2
    long_a = np.array([[0.3, 2.0, 3.0], [6.1, 2.05, 3.1], [6.1, 2.06, 3.1], [0.4, 5.9, 0.3], [0.4, 5.9, 0.3], [5.0, 1.4, 6.0]])
    paths = [zigzag(runs), zigzag([(1, 2999)]), long_a]
    w = np.concatenate(paths)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    for margin in (2.0, 1.7):
        want = model_of(m, w, off, step, margin)
        assert want["n_samples"][1] == 3000 and (want["cost"] > 0).all()
        assert_within(m.PathCost(w, off, step, margin), want, f"one-sample runs, margin {margin}")
        assert_within(device_call(m, w, off, step, margin), want, f"one-sample runs, device variant, margin {margin}")
    # one path alone: up to 2^18 pieces for it, so pieces of 1024 samples; segments of 3 * 10^5 samples
    want = model_of(m, long_a, [0, len(long_a)], 2e-5, 1.9)
    assert want["n_samples"][0] > 900_000
    assert_within(m.PathCost(long_a, [0, len(long_a)], 2e-5, 1.9), want, "segments over hundreds of pieces")
    m.close()


def test_host_route_and_device_route_agree(hip_lib):
    """batches of at most 256 samples: the host variant answers from the brick cache (sums in sample order), the device variant
    runs the kernels: both within the bound of the model"""
    m, _ = dense_map(64, obstacles=250, seed=5)
    small_w = np.array([[1.0, 1.0, 1.0], [1.5, 1.2, 1.1], [2.0, 2.2, 1.3], [3.0, 3.0, 3.0], [3.0, 3.0, 3.0], [2.5, 3.1, 2.0]])
    grew = []
    for off_s, step in (([0, 3, 4, 6], 0.05), ([0, 4, 4, 6], 0.02), ([0, 6], 0.03)):
        off_s = np.array(off_s)
        want = model_of(m, small_w, off_s, step, 0.8)
        assert 0 < want["n_samples"].sum() <= 256 and want["cost"].max() > 0
        before = m.host_cache_fetches
        host = m.PathCost(small_w, off_s, step, 0.8)
        grew.append(m.host_cache_fetches > before)
        assert_within(host, want, "host route")
        dev = device_call(m, small_w, off_s, step, 0.8)
        assert_within(dev, want, "device route, small batch")
        lim = bound(want["grad_n"][:, None], want["grad_abs"])
        assert (np.abs(host["grad"] - dev["grad"]) <= lim).all() and (np.abs(host["cost"] - dev["cost"]) <= bound(want["cost_n"], want["cost_abs"])).all()
    assert grew[0]   # the host route was taken: bricks fetched
    big = np.array([[0.5, 0.5, 0.5], [5.5, 5.5, 5.5]])   # just above: the device route (no brick fetched)
    before = m.host_cache_fetches
    got = m.PathCost(big, [0, 2], 0.02, 0.8)
    assert got["n_samples"][0] > 256 and m.host_cache_fetches == before
    assert_within(got, model_of(m, big, [0, 2], 0.02, 0.8), "just above the host limit")
    m.close()


def expected_alone(m, W, offs, step, margin, flagged):
    """the model of every unflagged path ALONE, assembled into the batch's outputs; flagged paths: NaN / -1 / rows 0"""
    n = len(offs) - 1
    out = {"cost": np.zeros(n), "length": np.zeros(n), "n_below": np.zeros(n, np.int64), "n_samples": np.zeros(n, np.int64),
           "grad": np.zeros((len(W), 3)), "cost_n": np.zeros(n, np.int64), "cost_abs": np.zeros(n), "length_n": np.zeros(n, np.int64),
           "length_abs": np.zeros(n), "grad_n": np.zeros(len(W), np.int64), "grad_abs": np.zeros((len(W), 3))}
    for q in range(n):
        if q in flagged:
            out["cost"][q] = out["length"][q] = np.nan
            out["n_below"][q] = out["n_samples"][q] = -1
            continue
        a, b = int(offs[q]), int(offs[q + 1])
        one = model_of(m, W[a:b], [0, b - a], step, margin)
        for k in ("cost", "length", "n_below", "n_samples", "cost_n", "cost_abs", "length_n", "length_abs"):
            out[k][q] = one[k][0]
        for k in ("grad", "grad_n", "grad_abs"):
            out[k][a:b] = one[k]
    return out


def test_device_variant(hip_lib):
    """PathCostDevice equals PathCost bit for bit (the same kernels); broken device offsets flag exactly the paths the header names,
    give their rows 0, and leave every other path equal to the model of that path alone"""
    m, _ = dense_map(64, obstacles=250, seed=5)
    rng = np.random.RandomState(6)
    w, off = make_paths(rng, np.zeros(3), np.full(3, 6.4), 0.1, n_paths=60)
    for step, margin in ((0.05, 1.0), (0.37, 0.3)):
        host = m.PathCost(w, off, step, margin)
        assert host["n_samples"].sum() > 256
        assert_bits(device_call(m, w, off, step, margin), host, "device vs host variant")
    # only some outputs requested: the call works, the others are not touched
    import torch
    dev = torch.device("cuda", 0)
    wt, ot = torch.from_numpy(w).to(dev), torch.from_numpy(off).to(dev)
    cost = torch.full((len(off) - 1,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    m.PathCostDevice(wt.data_ptr(), len(w), ot.data_ptr(), len(off) - 1, 0.37, 0.3, {"cost": cost.data_ptr()})
    m.synchronize()
    assert np.array_equal(cost.cpu().numpy().view(np.int64), host["cost"].view(np.int64))
    # broken offsets
    W = 0.3 + rng.rand(60, 3) * 5.5
    W[23] = [np.nan, 1.0, 1.0]
    good = np.arange(0, 61, 5).astype(np.int64)                  # 12 paths of 5 waypoints
    cases = []
    swapped = good.copy()
    swapped[2], swapped[3] = 15, 10          # entries 2 and 3 swapped: path 2 reversed, path 3 starts below entry 2; 4: the NaN
    cases.append(("swapped", swapped, {2, 3, 4}))
    garbage = good.copy()
    garbage[3], garbage[8] = 10 ** 9, -7     # out of range: the two paths that share each entry
    cases.append(("out of range", garbage, {2, 3, 4, 7, 8}))
    overlap = good.copy()
    overlap[3] = 17                          # another partition, still valid: path 2 = [10, 17), path 3 = [17, 20)
    overlap[6] = 38                          # in range but too large: path 5 = [25, 38) is valid, 6 is reversed, 7 would overlap 5
    cases.append(("overlapping", overlap, {4, 6, 7}))
    for name, offs, flagged in cases:
        got = device_call(m, W, offs, 0.05, 1.0)
        assert set(np.nonzero(got["n_samples"] < 0)[0].tolist()) == flagged, (name, got["n_samples"])
        want = expected_alone(m, W, offs, 0.05, 1.0, flagged)
        assert_within(got, want, f"device offsets: {name}")
        assert (want["cost"][[q for q in range(12) if q not in flagged]] > 0).any()
    m.close()


def test_same_call_same_bits_and_the_live_field(hip_lib):
    m, S = dense_map(64, obstacles=250, seed=31)
    rng = np.random.RandomState(32)
    w, off = make_paths(rng, np.zeros(3), np.full(3, 6.4), 0.1, n_paths=80)
    first = m.PathCost(w, off, 0.04, 0.6)
    for _ in range(2):
        assert_bits(m.PathCost(w, off, 0.04, 0.6), first, "same call twice")
    d1 = device_call(m, w, off, 0.04, 0.6)
    assert_bits(device_call(m, w, off, 0.04, 0.6), d1, "same device call twice")
    # a path through free space; then an obstacle right beside it: the call reads the live field
    p = np.array([[1.0, 3.2, 3.2], [5.4, 3.2, 3.2]])
    before = m.PathCost(p, [0, 2], 0.01, 0.5)
    near = np.array([[32, 34, 32], [20, 30, 32]], np.int32)
    for _ in range(3):
        m.SetOccupancy(near, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    after = m.PathCost(p, [0, 2], 0.01, 0.5)
    assert after["cost"][0] > before["cost"][0] and after["n_below"][0] >= before["n_below"][0]
    assert_within(after, model_of(m, p, [0, 2], 0.01, 0.5), "after the update")
    m.close()


def test_whole_call_errors(hip_lib):
    from fiesta_amd._lib import PathCostResult
    m, _ = dense_map(32, obstacles=30)
    lib = m._lib
    probe = np.array([[1.0, 1.0, 1.0]] * 9)
    ref = m.GetDistWithGradTrilinear(probe)
    w = np.array([[0.5, 0.5, 0.5], [2.0, 2.0, 2.0], [1.0, 2.0, 0.5]])
    out, grad = np.zeros(16), np.zeros((3, 3))
    res = PathCostResult(out.ctypes.data, grad.ctypes.data, None, None, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    off = np.array([0, 3], np.int64)
    off_start, off_end, off_down = np.array([1, 3], np.int64), np.array([0, 2], np.int64), np.array([0, 2, 1, 3], np.int64)
    inf, nan = float("inf"), float("nan")
    bad_calls = [(p(w), 3, p(off), 1, 0.0, 0.5, C.byref(res)), (p(w), 3, p(off), 1, -0.1, 0.5, C.byref(res)),
                 (p(w), 3, p(off), 1, inf, 0.5, C.byref(res)), (p(w), 3, p(off), 1, nan, 0.5, C.byref(res)),
                 (p(w), 3, p(off), 1, 0.1, nan, C.byref(res)), (p(w), 3, p(off), 1, 0.1, inf, C.byref(res)),
                 (p(w), 3, p(off), 1, 0.1, -inf, C.byref(res)),
                 (p(w), 3, p(off_start), 1, 0.1, 0.5, C.byref(res)), (p(w), 3, p(off_end), 1, 0.1, 0.5, C.byref(res)),
                 (p(w), 3, p(off_down), 3, 0.1, 0.5, C.byref(res)),
                 (None, 3, p(off), 1, 0.1, 0.5, C.byref(res)), (p(w), 3, None, 1, 0.1, 0.5, C.byref(res)),
                 (p(w), 3, p(off), 1, 0.1, 0.5, None)]
    for args in bad_calls:
        assert lib.fiesta_hip_path_cost(m._h, *args) == 1, args            # FIESTA_HIP_ERR_INVALID
        d, g = m.GetDistWithGradTrilinear(probe)
        assert np.array_equal(d, ref[0]) and np.array_equal(g, ref[1])     # the map is still usable
    assert lib.fiesta_hip_path_cost_dev(m._h, None, 3, None, 1, 0.1, 0.5, C.byref(res)) == 1
    assert lib.fiesta_hip_path_cost_dev(m._h, p(w), 3, p(off), 1, 0.1, nan, C.byref(res)) == 1
    assert lib.fiesta_hip_path_cost_dev(m._h, p(w), 3, p(off), 1, 0.0, 0.5, C.byref(res)) == 1
    assert lib.fiesta_hip_path_cost(m._h, p(w), 0, p(np.array([0], np.int64)), 0, 0.1, 0.5, C.byref(res)) == 0   # n_paths = 0
    assert lib.fiesta_hip_path_cost(m._h, p(w), 3, p(off), 1, 0.1, 0.5, C.byref(res)) == 0
    assert out[0] > 0 and grad.any()
    m.close()


def test_cpp_example_descends(hip_lib, tmp_path):
    """examples/path_cost.cpp against the facade: plain gradient descent with the call's waypoint gradients; the cost never rises
    after the first step and ends below half of where it began"""
    import __graft_entry__ as g
    g.build_hip()
    exe = str(tmp_path / "path_cost")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "path_cost.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, check=True)
    out = json.loads(run.stdout.strip().splitlines()[-1])
    costs = np.array(out["costs"])
    print(f"example: cost {costs[0]:.6f} -> {costs[-1]:.6f} in {len(costs) - 1} steps")
    assert len(costs) >= 25 and costs[0] > 0
    assert (np.diff(costs[1:]) <= 0).all(), costs
    assert costs[-1] < 0.5 * costs[0]
    path = np.array(out["final_path"])
    assert np.array_equal(path[0], [-2.6, 1.5, 1.0]) and np.array_equal(path[-1], [-2.6 + 5.5 * 1.0, 1.5 + 0.1 * 1.0, 1.0])   # the ends stayed
