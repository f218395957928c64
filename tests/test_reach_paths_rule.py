"""CPU side of the reach paths (fiesta_hip_reach_paths, include/fiesta_hip.h): the definition.

fiesta_amd.reach_paths_model (descent, line-of-sight anchors, memoised per voxel) is the model the GPU tests compare the kernels
with, so it must be the header's definition: it is checked against a literal restatement -- plain loops over the moves and the
anchors, its own copy of the reference traversal with the general intbound arithmetic, no memo -- on random 12 x 10 x 9 fields that
fiesta_amd.reach_model flooded.  Everything is integer or one f64 expression: comparisons are exact.  Also: the structure of a
path, the chain property that makes the unsubstituted traversal the right visibility test, an arbitrary array, the ctypes mirror,
the whole-call argument rules that the library checks before it touches a device, the kernels' resources and the C++ example.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from fiesta_amd.reach_model import (REACH_PATH_BLOCKED, REACH_PATH_BROKEN, REACH_PATH_OK, REACH_PATH_OUTSIDE, REACH_PATH_UNREACHED,
                                    REACH_PATHS_SHORTCUT, REACH_THROUGH_UNKNOWN, reach_model, reach_moves, reach_paths_model, reach_visible,
                                    reach_walk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (12, 10, 9)
INF = 2 ** 31 - 1


def loop_walk(p, q):
    """src/raycast.cpp:56-158 between two voxel centres, literally: signum, mod and intbound as the reference writes them, no clipping
    box, no 1500-voxel exception, no substitution of the last voxel"""
    def intbound(s, ds):
        if ds < 0:
            s, ds = -s, -ds
        w = math.fmod(math.fmod(s, 1.0) + 1.0, 1.0)
        return (1 - w) / ds if ds != 0 else math.inf
    a, b = [v + 0.5 for v in p], [v + 0.5 for v in q]
    c, e = [math.floor(v) for v in a], [math.floor(v) for v in b]
    d = [float(e[i] - c[i]) for i in range(3)]
    step = [(v > 0) - (v < 0) for v in d]
    tmax = [intbound(a[i], d[i]) for i in range(3)]
    tstep = [step[i] / d[i] if d[i] != 0 else math.nan for i in range(3)]
    reach2 = (b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1]) + (b[2] - a[2]) * (b[2] - a[2])
    out = []
    if step == [0, 0, 0]:
        return out
    while True:
        out.append(tuple(c))
        if (c[0] - a[0]) * (c[0] - a[0]) + (c[1] - a[1]) * (c[1] - a[1]) + (c[2] - a[2]) * (c[2] - a[2]) > reach2 or c == e:
            return out
        if tmax[0] < tmax[1]:
            ax = 0 if tmax[0] < tmax[2] else 2
        else:
            ax = 1 if tmax[1] < tmax[2] else 2
        c[ax] += step[ax]
        tmax[ax] += tstep[ax]


def loop_paths(cost, box_lo, targets, connectivity, flags, max_span, origin, resolution):
    """the header's rule, target by target, with nothing shared between targets"""
    moves = [(dx, dy, dz, 2 + abs(dx) + abs(dy) + abs(dz)) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    shape = cost.shape

    def inside(v):
        return all(0 <= v[c] < shape[c] for c in range(3))

    def visible(p, q):           # box-local voxels here; the map voxels are these plus box_lo
        if sum(abs(p[c] - q[c]) for c in range(3)) > 4095:
            return False
        P, Q = [p[c] + box_lo[c] for c in range(3)], [q[c] + box_lo[c] for c in range(3)]
        for v in loop_walk(P, Q):
            w = tuple(v[c] - box_lo[c] for c in range(3))
            if not inside(w) or cost[w] < 0:
                return False
        return True

    offsets, vox, status, n_moves = [0], [], [], []
    for t in targets:
        v = tuple(int(t[c]) - box_lo[c] for c in range(3))
        st = REACH_PATH_OK
        if not inside(v):
            st = REACH_PATH_OUTSIDE
        elif cost[v] == -1:
            st = REACH_PATH_BLOCKED
        elif cost[v] == INF:
            st = REACH_PATH_UNREACHED
        elif cost[v] < -1:
            st = REACH_PATH_BROKEN
        D = [v]
        while st == REACH_PATH_OK and cost[D[-1]] > 0:
            c, nxt = int(cost[D[-1]]), None
            for dx, dy, dz, w in moves:
                n = (D[-1][0] + dx, D[-1][1] + dy, D[-1][2] + dz)
                if not inside(n):
                    continue
                if cost[n] < -1:
                    st = REACH_PATH_BROKEN
                if nxt is None and cost[n] >= 0 and int(cost[n]) + w == c:
                    nxt = n
            if nxt is None:
                st = REACH_PATH_BROKEN
            D.append(nxt)
        if st != REACH_PATH_OK:
            status.append(st), n_moves.append(-1), offsets.append(offsets[-1])
            continue
        L = len(D) - 1
        K = list(range(L + 1))
        if flags & 1:
            K, i = [0], 0
            while i < L:
                j = i + 1
                while j < L and j + 1 - i <= max_span and visible(D[i], D[j + 1]):
                    j += 1
                K.append(j)
                i = j
        for k in reversed(K):
            vox.append([D[k][c] + box_lo[c] for c in range(3)])
        status.append(st), n_moves.append(L), offsets.append(len(vox))
    vox = np.array(vox, np.int32).reshape(-1, 3)
    pos = np.empty((len(vox), 3))
    for i in range(len(vox)):
        for c in range(3):
            pos[i, c] = (float(vox[i, c]) + 0.5) * resolution + origin[c]
    return {"offsets": np.array(offsets, np.int64), "waypoints_vox": vox, "waypoints_pos": pos, "status": np.array(status, np.int32),
            "n_moves": np.array(n_moves, np.int32)}


def same(a, b, what=""):
    for k in ("offsets", "waypoints_vox", "waypoints_pos", "status", "n_moves"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def random_field(seed, conn):
    """a flooded 12 x 10 x 9 block: scattered obstacles, a wall with a door, an enclosed pocket, an unknown slab"""
    rng = np.random.RandomState(seed)
    obs = np.ones(SHAPE, bool)
    occ = rng.rand(*SHAPE) < (0.05, 0.15, 0.3)[seed % 3]
    occ[6] = True
    occ[6, rng.randint(0, 10), rng.randint(0, 9)] = False           # the door
    occ[8:11, 1:4, 1:4] = True
    occ[9, 2, 2] = False                                             # a pocket: free, never reached
    obs[2, 5:, :] = False
    org = [int(v) for v in rng.randint(-30, 30, 3)]
    seeds = rng.randint(0, (5, 10, 9), (2, 3)) + org
    occ[tuple((seeds - org).T)] = False
    r = reach_model(obs, occ, seeds, connectivity=conn, flags=(REACH_THROUGH_UNKNOWN if seed & 1 else 0), origin_vox=org)
    return rng, r["cost"], r["box_lo"]


ALL = np.stack(np.meshgrid(*[np.arange(-1, s + 1) for s in SHAPE], indexing="ij"), -1).reshape(-1, 3)   # every voxel and a shell outside


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("seed", range(4))
def test_model_is_the_definition_on_random_fields(seed, conn):
    rng, cost, lo = random_field(seed, conn)
    targets = ALL + lo
    origin, res = (-1.3, 0.7, 2.05), (0.1, 0.25, 0.05)[seed % 3]
    counts = set()
    for flags, span in ((0, 4096), (1, 1), (1, 3), (1, 4096)):
        got = reach_paths_model(cost, lo, targets, conn, flags, span, origin, res)
        same(got, loop_paths(cost, lo, targets, conn, flags, span, origin, res), (seed, conn, flags, span))
        counts.add(int(got["offsets"][-1]))
        assert {REACH_PATH_OK, REACH_PATH_OUTSIDE, REACH_PATH_BLOCKED, REACH_PATH_UNREACHED} <= set(got["status"].tolist())
    assert len(counts) >= 2                                          # shortcutting shortens something
    # a model call that shares nothing: one target at a time
    pick = targets[rng.randint(0, len(targets), 40)]
    whole = reach_paths_model(cost, lo, pick, conn, 1, 4096, origin, res)
    for i, t in enumerate(pick):
        one = reach_paths_model(cost, lo, [t], conn, 1, 4096, origin, res)
        assert np.array_equal(one["waypoints_vox"], whole["waypoints_vox"][whole["offsets"][i]:whole["offsets"][i + 1]])


@pytest.mark.parametrize("conn", [6, 26])
def test_max_span_one_is_the_raw_path(conn):
    _, cost, lo = random_field(5, conn)
    raw = reach_paths_model(cost, lo, ALL + lo, conn, 0, 77)           # (max_span is ignored without the flag)
    same(raw, reach_paths_model(cost, lo, ALL + lo, conn, REACH_PATHS_SHORTCUT, 1), conn)
    same(raw, reach_paths_model(cost, lo, ALL + lo, conn, 0, -5), conn)
    for bad in (dict(flags=2), dict(flags=1, max_span=0), dict(connectivity=18)):
        with pytest.raises(ValueError):
            reach_paths_model(cost, lo, ALL + lo, **{"connectivity": conn, **bad})


@pytest.mark.parametrize("conn", [6, 26])
def test_path_structure(conn):
    _, cost, lo = random_field(6, conn)
    targets = ALL + lo
    weights = {(dx, dy, dz): w for dx, dy, dz, w in reach_moves(conn)}
    raw = reach_paths_model(cost, lo, targets, conn, 0, 1, (0.5, -2.0, 1.0), 0.2)
    cut = reach_paths_model(cost, lo, targets, conn, 1, 4096, (0.5, -2.0, 1.0), 0.2)
    assert np.array_equal(raw["status"], cut["status"]) and np.array_equal(raw["n_moves"], cut["n_moves"])
    n_ok = shorter = 0
    for i, t in enumerate(targets):
        w = raw["waypoints_vox"][raw["offsets"][i]:raw["offsets"][i + 1]].astype(np.int64)
        s = cut["waypoints_vox"][cut["offsets"][i]:cut["offsets"][i + 1]].astype(np.int64)
        if raw["status"][i] != REACH_PATH_OK:
            assert len(w) == 0 and len(s) == 0 and raw["n_moves"][i] == -1
            continue
        n_ok += 1
        c = [int(cost[tuple(v - lo)]) for v in w]
        assert len(w) == raw["n_moves"][i] + 1 and c[0] == 0 and np.array_equal(w[-1], t) and c[-1] == int(cost[tuple(t - lo)])
        for k in range(len(w) - 1):                                   # seed -> target: every step a legal move that costs its weight
            assert c[k + 1] - c[k] == weights[tuple(w[k + 1] - w[k])]
        # the shortcut path: a subsequence of the raw one with the same ends, every segment visible from its target-side end
        rows = [tuple(v) for v in w]
        at = [rows.index(tuple(v)) for v in s]
        assert at == sorted(set(at)) and at[0] == 0 and at[-1] == len(w) - 1
        for a, b in zip(s[1:], s[:-1]):
            assert np.abs(a - b).max() == 1 or reach_visible(cost, lo, a, b)
        shorter += len(s) < len(w)
    assert n_ok > 300 and shorter > 100
    assert np.array_equal(raw["waypoints_pos"], (raw["waypoints_vox"].astype(np.float64) + 0.5) * 0.2 + np.array((0.5, -2.0, 1.0)))
    # a target of cost 0: one waypoint, no move
    seed = targets[[int(cost[tuple(t - lo)]) == 0 if np.all((t - lo >= 0) & (t - lo < SHAPE)) else False for t in targets]]
    r = reach_paths_model(cost, lo, seed, conn, 1, 8)
    assert len(seed) >= 1 and np.array_equal(r["waypoints_vox"], seed) and (r["n_moves"] == 0).all()


def test_unsubstituted_traversal_is_a_six_connected_chain():
    """why visible() tests the traversal's own voxels and not the ray query's W: between two centres the emitted sequence followed
    by q is a 6-connected chain (no corner is cut), of at most sum |delta| + 1 voxels; where the traversal stops beside q, W -- the
    sequence with its last voxel replaced by q -- has dropped a voxel of that chain"""
    from fiesta_amd import ray_walk
    rng = np.random.RandomState(11)
    n, beside = 20000, 0
    ext = np.array((6, 40, 201))[rng.randint(0, 3, (n, 3))]
    d = (rng.randint(0, 2 ** 31 - 1, (n, 3)) % ext) * rng.choice((-1, 1), (n, 3))
    d[rng.rand(n, 3) < 0.15] = 0                                      # some axes equal
    p = rng.randint(-500, 500, (n, 3))
    for i in range(n):
        a, b = [int(v) for v in p[i]], [int(v) for v in p[i] + d[i]]
        w = reach_walk(a, b)
        if a == b:
            assert w == []
            continue
        assert w[0] == tuple(a) and len(w) <= int(np.abs(d[i]).sum()) + 1
        chain = w if w[-1] == tuple(b) else w + [tuple(b)]
        steps = np.abs(np.diff(np.array(chain), axis=0)).sum(1)
        assert (steps == 1).all(), (a, b)
        beside += w[-1] != tuple(b)
        if i % 20 == 0:                                               # the model's walk is the reference's, and the ray query's up to its last voxel
            assert w == loop_walk(a, b)
            W = ray_walk([v + 0.5 for v in a], [v + 0.5 for v in b])
            assert len(W) == len(w) and [tuple(v) for v in W[:-1].tolist()] == w[:-1] and tuple(W[-1].tolist()) == tuple(b)
    assert 0.01 * n < beside < 0.15 * n


def test_arbitrary_field_is_broken_and_terminates():
    sevens = np.full((6, 5, 4), 7, np.int32)
    for conn in (6, 26):
        for flags in (0, 1):
            r = reach_paths_model(sevens, (0, 0, 0), [(1, 1, 1), (5, 4, 3), (6, 0, 0)], conn, flags, 9)
            assert r["status"].tolist() == [REACH_PATH_BROKEN, REACH_PATH_BROKEN, REACH_PATH_OUTSIDE]
            assert r["offsets"].tolist() == [0, 0, 0, 0] and r["n_moves"].tolist() == [-1, -1, -1]
    # costs that descend and then lead nowhere; a cost below -1 next to the way; a target below -1
    f = np.full((5, 1, 1), -1, np.int32)
    f[:, 0, 0] = [4, 6, 9, 12, 15]
    assert reach_paths_model(f, (0, 0, 0), [(4, 0, 0)], 6)["status"].tolist() == [REACH_PATH_BROKEN]
    f[:, 0, 0] = [0, 3, 6, 9, 12]
    assert reach_paths_model(f, (0, 0, 0), [(4, 0, 0)], 6)["n_moves"].tolist() == [4]
    g = np.full((5, 2, 1), -1, np.int32)
    g[:, 0, 0] = [0, 3, 6, 9, 12]
    g[1, 1, 0] = -2
    assert reach_paths_model(g, (0, 0, 0), [(4, 0, 0), (0, 0, 0), (1, 1, 0)], 6)["status"].tolist() == [REACH_PATH_BROKEN, REACH_PATH_OK, REACH_PATH_BROKEN]
    # random arrays: every call ends, and a path that is OK descends
    rng = np.random.RandomState(2)
    junk = rng.randint(-3, 12, (7, 6, 5)).astype(np.int32)
    tg = np.argwhere(np.ones(junk.shape, bool))
    r = reach_paths_model(junk, (0, 0, 0), tg, 26, 1, 4096)
    assert (r["status"] == REACH_PATH_BROKEN).any() and ((r["status"] == REACH_PATH_OK) == (r["n_moves"] >= 0)).all()
    same(r, loop_paths(junk, (0, 0, 0), tg, 26, 1, 4096, (0.0, 0.0, 0.0), 1.0))


def test_struct_mirror_follows_the_header():
    from fiesta_amd import _lib
    import importlib
    rm = importlib.import_module("fiesta_amd.reach_model")       # (fiesta_amd.reach_model itself is the function)
    text = open(_lib.HEADER_PATH).read()
    struct, mirror = "fiesta_hip_reach_paths_result", _lib.ReachPathsResult
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*?\]", "", n).strip(" *") for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in mirror._fields_] == ["offsets", "waypoints_vox", "waypoints_pos", "status", "n_moves"]
    assert C.sizeof(mirror) == 5 * C.sizeof(C.c_void_p)
    for name in ("PATHS_SHORTCUT", "PATH_OK", "PATH_OUTSIDE", "PATH_BLOCKED", "PATH_UNREACHED", "PATH_BROKEN"):
        assert re.search(r"#define FIESTA_HIP_REACH_%s (\d+)" % name, text).group(1) == str(getattr(rm, "REACH_" + name)), name


def test_argument_rules_are_checked_before_any_device_use():
    """every whole-call error is refused -- with its own message -- before the handle is looked at: the calls below pass no map at
    all, on a machine that may have no GPU"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)
    neg = (C.c_int32 * 3)(1, 1, -1)
    big_lo, big_hi = (C.c_int32 * 3)(-2 ** 31, 0, 0), (C.c_int32 * 3)(2 ** 31 - 1, 0, 0)
    cube_hi = (C.c_int32 * 3)(1023, 1023, 256)                       # 1024 * 1024 * 257 > 2^28
    cost = (C.c_int32 * 8)(*([0] * 8))
    pts = (C.c_int32 * 3)(1, 1, 1)
    off = (C.c_int64 * 2)(77, 77)
    res = _lib.ReachPathsResult(C.cast(off, C.c_void_p), None, None, None, None)
    no_off = _lib.ReachPathsResult(None, None, None, None, None)
    #        cost  lo   hi   targets n conn flags span capacity result   the message names
    cases = [(cost, lo, hi, pts, 1, 26, 0, 1, 0, None, "result is null"),
             (cost, lo, hi, pts, 1, 26, 0, 1, 0, no_off, "offsets"),
             (cost, lo, hi, pts, 1, 18, 0, 1, 0, res, "connectivity"),
             (cost, lo, hi, pts, 1, 0, 0, 1, 0, res, "connectivity"),
             (cost, lo, hi, pts, 1, 26, 2, 1, 0, res, "flag"),
             (cost, lo, hi, pts, 1, 26, -1, 1, 0, res, "flag"),
             (cost, lo, hi, pts, 1, 26, 1, 0, 0, res, "max_span"),
             (cost, lo, hi, pts, 1, 6, 1, -4, 0, res, "max_span"),
             (cost, lo, hi, pts, -1, 26, 0, 1, 0, res, "negative count"),
             (cost, lo, hi, pts, 1, 26, 0, 1, -1, res, "negative capacity"),
             (cost, lo, hi, None, 1, 26, 0, 1, 0, res, "targets"),
             (None, lo, hi, pts, 1, 26, 0, 1, 0, res, "all be given"),
             (cost, None, hi, pts, 1, 26, 0, 1, 0, res, "all be given"),
             (cost, lo, None, pts, 1, 26, 0, 1, 0, res, "all be given"),
             (cost, None, None, pts, 1, 26, 0, 1, 0, res, "all be given"),
             (cost, lo, neg, pts, 1, 26, 0, 1, 0, res, "empty"),
             (cost, big_lo, big_hi, pts, 1, 26, 0, 1, 0, res, "2^28"),
             (cost, lo, cube_hi, pts, 1, 26, 0, 1, 0, res, "2^28"),
             (cost, lo, hi, pts, 1, 26, 0, 0, 0, res, "null map"),      # nothing wrong but the missing map (max_span ignored without the flag)
             (None, None, None, None, 0, 6, 1, 1, 5, res, "null map")]
    for fn in (lib.fiesta_hip_reach_paths, lib.fiesta_hip_reach_paths_dev):
        for c, a, b, t, n, conn, flags, span, cap, r, word in cases:
            st = fn(None, c, a, b, t, n, conn, flags, span, cap, C.byref(r) if r is not None else None)
            assert st == 1, (word, st)                                   # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    assert list(off) == [77, 77]


def test_reach_path_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_reach_path_" in k}
    # count and write: connectivity 6 / 26 x raw / shortcut; one scan
    for kernel, copies in (("k_reach_path_count", 4), ("k_reach_path_write", 4), ("k_reach_path_scan", 1)):
        assert sum(kernel in k for k in res) == copies, (kernel, sorted(res))
    assert len(res) == 9
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)


def test_example_compiles_with_host_compiler_only(tmp_path):
    import __graft_entry__ as g
    g.build_hip()
    exe = os.path.join(str(tmp_path), "reach_path")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "reach_path.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "ReachPathSet ReachPaths(const std::vector<Eigen::Vector3i> &targets, int32_t connectivity = 26, bool shortcut = false" in src
