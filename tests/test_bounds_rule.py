"""The rule of fiesta_hip_corridor_bounds (include/fiesta_hip.h) without a GPU.

fiesta_amd.corridor_bounds_model is the definition: it is held to fiesta_amd.corridor_bounds -- the host function the call replaces --
bit for bit on seeded synthetic corridors, its `box` output to a literal per-waypoint loop, and each rule the older function does
not have (VOID_BROKEN, truncated corridors, the device variant's offset rules) to a hand-made case.  Then the ctypes mirror against
the header, every whole-call error through the built library (none needs a device), and the resources of the new kernels.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, ORG = 0.25, np.array([-3.0, 1.5, 0.0])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def boxes_pos(bx):
    bx = np.asarray(bx, np.int32).reshape(-1, 6)
    return np.concatenate([bx[:, :3].astype(np.float64) * RES + ORG, (bx[:, 3:].astype(np.float64) + 1.0) * RES + ORG], axis=1)


def walk(rng, m, kind):
    """a voxel walk of m waypoints: 6-connected, 26-connected, or with segments of up to 9 voxels along one to three axes"""
    start = rng.randint(-20, 20, 3)
    if m == 0:
        return np.zeros((0, 3), np.int64)
    if kind == 6:
        steps = np.zeros((m - 1, 3), np.int64)
        steps[np.arange(m - 1), rng.randint(0, 3, m - 1)] = rng.choice([-1, 1], m - 1)
    elif kind == 26:
        steps = rng.randint(-1, 2, (m - 1, 3))
    else:
        steps = rng.randint(-9, 10, (m - 1, 3)) * (rng.rand(m - 1, 3) < 0.5)
    return start + np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(steps, axis=0)])


def random_corridors(seed, n_paths=120):
    """(waypoints_vox, offsets, corridor) with random non-decreasing entries (entry[0] = 0; ties allowed, but entry[1] >= 1: see the
    model's docstring), random boxes around the walk and statuses 0 / 1 / 2"""
    rng = np.random.RandomState(seed)
    paths, bxs, ents, status = [], [], [], []
    for p in range(n_paths):
        m = int(rng.choice([0, 1, 2, 3, 5, 17, 40]))
        v = walk(rng, m, (6, 26, "long")[p % 3])
        chain = int(np.abs(np.diff(v, axis=0)).sum()) if m > 1 else 0
        nb = int(rng.randint(0, 7))
        e = np.sort(rng.randint(1, max(2, chain + 3), max(nb - 1, 0)))
        if nb > 2 and rng.rand() < 0.3:
            e[1] = e[0]                                                  # a tie: the box before it is never anybody's b(i)
        centre = v[rng.randint(0, m, nb)] if m else rng.randint(-20, 20, (nb, 3))
        lo = centre.reshape(nb, 3) - rng.randint(0, 6, (nb, 3))
        hi = lo + rng.randint(0, 9, (nb, 3))
        if m and p % 2:                                                  # every other path: boxes that hold the whole walk and more
            lo, hi = v.min(axis=0) - rng.randint(0, 4, (nb, 3)), v.max(axis=0) + rng.randint(0, 4, (nb, 3))
        paths.append(v), bxs.append(np.concatenate([lo, hi], axis=1)), ents.append(np.concatenate([[0], e])[:nb])
        status.append(int(rng.choice([0, 0, 0, 1, 2])))
    off = np.concatenate([[0], np.cumsum([len(v) for v in paths])]).astype(np.int64)
    bx = np.concatenate(bxs).astype(np.int32).reshape(-1, 6)
    cor = {"offsets": np.concatenate([[0], np.cumsum([len(b) for b in bxs])]).astype(np.int64), "boxes": bx, "boxes_pos": boxes_pos(bx),
           "entry": np.concatenate(ents).astype(np.int32), "status": np.array(status, np.int32)}
    return np.concatenate(paths).astype(np.int32), off, cor


def literal_box(wv, off, cor):
    """per waypoint the global index of the last box of its path with entry <= its chain index, -1 where the path has no box"""
    out = []
    for p in range(len(off) - 1):
        c = 0
        for i in range(off[p], off[p + 1]):
            if i > off[p]:
                c += sum(abs(int(wv[i][k]) - int(wv[i - 1][k])) for k in range(3))
            best = -1
            for j in range(cor["offsets"][p], cor["offsets"][p + 1]):
                if cor["entry"][j] <= c:
                    best = j
            out.append(best)
    return np.array(out, np.int64)


# ---- 1. the model against the function it replaces -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_the_model_equals_corridor_bounds_on_random_corridors(seed):
    import fiesta_amd
    wv, off, cor = random_corridors(seed)
    assert not np.signbit(cor["boxes_pos"][cor["boxes_pos"] == 0]).any()   # no negative zero
    seen = {"empty": 0, "skipped": 0, "first_outside": 0, "inter": 0}
    for inset in (0.0, RES * 2.0 ** -20, 0.07):
        old_b, old_ok = fiesta_amd.corridor_bounds(wv, off, cor, inset=inset)
        got = fiesta_amd.corridor_bounds_model(wv, off, cor, inset)
        assert got["bounds"].dtype == np.float64 and got["ok"].dtype == np.int32 and got["box"].dtype == np.int64
        assert np.array_equal(bits(got["bounds"]), bits(old_b))
        assert np.array_equal(got["ok"] != 0, old_ok) and set(np.unique(got["ok"])) <= {0, 1}
    box = literal_box(wv, off, cor)
    assert np.array_equal(got["box"], box)
    assert np.array_equal(np.isnan(got["bounds"]).all(axis=1), box < 0) and not np.isnan(got["bounds"][box >= 0]).any()
    # what the corridors were made to hold
    plain = cor["boxes_pos"][np.maximum(box, 0)]
    raw = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0)["bounds"]
    changed = (box >= 0) & (bits(raw) != bits(plain)).any(axis=1)
    seen["inter"] = int(changed.sum())
    seen["empty"] = int((raw[changed, :3] > raw[changed, 3:]).any(axis=1).sum())
    for p in range(len(off) - 1):
        b = box[off[p]:off[p + 1]]
        if len(b) > 1 and b[0] >= 0 and cor["status"][p] == 0 and not got["ok"][p]:
            seen["skipped" if (np.diff(b) > 1).any() else "first_outside"] += 1
    print(seed, seen)
    assert seen["inter"] >= 5 and seen["empty"] >= 1 and seen["skipped"] >= 1 and seen["first_outside"] >= 1
    assert set(cor["status"].tolist()) == {0, 1, 2} and got["ok"].sum() >= 3


# ---- 2. each rule on a hand-made case -------------------------------------------------------------------------------------------------
def corridor(boxes_by_path, entries_by_path, status):
    bx = np.array([b for bs in boxes_by_path for b in bs], np.int32).reshape(-1, 6)
    return {"offsets": np.concatenate([[0], np.cumsum([len(b) for b in boxes_by_path])]).astype(np.int64), "boxes": bx, "boxes_pos": boxes_pos(bx),
            "entry": np.array([e for es in entries_by_path for e in es], np.int32), "status": np.array(status, np.int32)}


A, B, Cx, D = [0, 0, 0, 4, 3, 3], [3, 0, 0, 8, 2, 2], [7, 1, 0, 9, 9, 1], [0, 0, 0, 1, 1, 1]


def hand_made():
    """path 0: chain indices 0 2 3 5 7 11 through boxes A (entry 0), B (4), C (8); path 1 skips B; path 2 is BLOCKED after its only
    box; path 3 is empty; path 4 is one waypoint; path 5 starts outside the box its second waypoint changes to; path 6 has no box"""
    p0 = [[1, 1, 1], [3, 1, 1], [4, 1, 1], [6, 1, 1], [8, 1, 1], [8, 5, 1]]
    p1 = [[1, 1, 1], [8, 2, 1], [8, 6, 1]]
    p2 = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0]]
    p4 = [[8, 8, 1]]
    p5 = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    p6 = [[0, 0, 0], [1, 0, 0]]
    wv = np.array(p0 + p1 + p2 + p4 + p5 + p6, np.int32)
    off = np.array([0, 6, 9, 13, 13, 14, 17, 19], np.int64)
    cor = corridor([[A, B, Cx], [A, B, Cx], [D], [], [Cx], [D, [1, 1, 1, 5, 5, 5]], []], [[0, 4, 8], [0, 4, 8], [0], [], [0], [0, 3], []],
                   [0, 0, 2, 0, 0, 0, 2])
    return wv, off, cor


def test_the_rules_on_a_hand_made_corridor():
    import fiesta_amd
    wv, off, cor = hand_made()
    pos = cor["boxes_pos"]
    got = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0)
    assert got["ok"].tolist() == [1, 0, 0, 1, 1, 0, 0]
    assert got["box"].tolist() == [0, 0, 0, 1, 1, 2, 3, 5, 5, 6, 6, 6, 6, 7, 8, 9, 9, -1, -1]
    both = lambda a, b: np.concatenate([np.maximum(pos[a, :3], pos[b, :3]), np.minimum(pos[a, 3:], pos[b, 3:])])  # noqa: E731
    assert np.array_equal(got["bounds"][:6], np.array([pos[0], pos[0], both(0, 1), pos[1], both(1, 2), pos[2]]))
    assert np.array_equal(got["bounds"][6:17], pos[[3, 5, 5, 6, 6, 6, 6, 7, 8, 9, 9]])   # not ok: each waypoint keeps its own box
    assert np.isnan(got["bounds"][17:]).all()
    # the inset comes off the three upper faces of every row, one subtraction
    ins = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.07)
    assert np.array_equal(bits(ins["bounds"][:, :3]), bits(got["bounds"][:, :3])) and np.array_equal(bits(ins["bounds"][:, 3:]), bits(got["bounds"][:, 3:] - 0.07))
    assert np.array_equal(ins["ok"], got["ok"]) and np.array_equal(ins["box"], got["box"])
    # VOID_BROKEN: the rows of the paths that are not ok are NaN, everything else is as before
    void = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.07, void_broken=True)
    broken = np.repeat(got["ok"] == 0, np.diff(off))
    assert np.isnan(void["bounds"][broken]).all() and np.array_equal(bits(void["bounds"][~broken]), bits(ins["bounds"][~broken]))
    assert np.array_equal(void["ok"], got["ok"]) and np.array_equal(void["box"], got["box"])
    for bad in (float("nan"), -1e-9, float("inf")):
        with pytest.raises(ValueError):
            fiesta_amd.corridor_bounds_model(wv, off, cor, bad)
    with pytest.raises(ValueError):
        fiesta_amd.corridor_bounds_model(wv, off[:-1], cor, 0.0)


def test_a_truncated_corridor():
    """n_boxes below the total: the paths whose box range ends above it get ok = 0, NaN rows and box -1 (the device variant), or the
    call is refused (the host variant); the paths before them are untouched"""
    import fiesta_amd
    wv, off, cor = hand_made()
    full = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0, device_offsets=True)
    whole = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0)
    for k in ("ok", "box"):
        assert np.array_equal(full[k], whole[k])
    assert np.array_equal(bits(full["bounds"]), bits(whole["bounds"]))
    cut = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0, n_boxes=7, device_offsets=True)   # boxes 0 .. 6: paths 0, 1, 2 and the empty 3
    rows = np.arange(len(wv)) < off[4]
    assert cut["ok"].tolist() == [1, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(bits(cut["bounds"][rows]), bits(full["bounds"][rows])) and np.array_equal(cut["box"][rows], full["box"][rows])
    assert np.isnan(cut["bounds"][~rows]).all() and (cut["box"][~rows] == -1).all()
    with pytest.raises(ValueError):
        fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0, n_boxes=7)
    with pytest.raises(ValueError):
        fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0, n_boxes=len(cor["entry"]) + 1)
    # a box range that decreases or is negative
    bad = dict(cor, offsets=cor["offsets"].copy())
    bad["offsets"][3] = 5                                                # path 2: [6, 5) decreases; the empty path 3: [5, 7)
    bad["offsets"][5] = -1                                               # path 4: [7, -1), path 5: [-1, 10)
    got = fiesta_amd.corridor_bounds_model(wv, off, bad, 0.0, device_offsets=True)
    assert got["ok"].tolist() == [1, 0, 0, 1, 0, 0, 0]
    assert np.isnan(got["bounds"][off[4]:off[6]]).all() and (got["box"][off[4]:off[6]] == -1).all()
    assert np.isnan(got["bounds"][off[2]:off[3]]).all() and (got["box"][off[2]:off[3]] == -1).all()
    assert got["box"][off[1]:off[2]].tolist() == [3, 5, 5] and np.array_equal(bits(got["bounds"][:off[2]]), bits(full["bounds"][:off[2]]))
    with pytest.raises(ValueError):
        fiesta_amd.corridor_bounds_model(wv, off, bad, 0.0)


def test_device_offsets():
    """the device variant's offset rule (path clearance's): the flagged paths get ok = 0 and read nothing, every row outside the
    valid paths is NaN / -1, the valid paths are computed over the ranges they name"""
    import fiesta_amd
    wv, off, cor = hand_made()
    good = fiesta_amd.corridor_bounds_model(wv, off, cor, 0.0)
    bad = off.copy()
    bad[1], bad[2] = off[2], off[1]       # path 0: [0, 9) -- three more waypoints; path 1: [9, 6) reversed; path 2: [6, 13) starts below 9
    bad[6] = len(wv) + 4                  # path 5 leaves the range, path 6 starts outside it
    got = fiesta_amd.corridor_bounds_model(wv, bad, cor, 0.0, device_offsets=True)
    assert got["ok"].tolist() == [1, 0, 0, 1, 1, 0, 0]
    assert got["box"][:9].tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 2]        # path 0's chain index runs on over the three new waypoints
    assert np.array_equal(bits(got["bounds"][:6]), bits(good["bounds"][:6])) and np.array_equal(bits(got["bounds"][6:9]), bits(cor["boxes_pos"][[2, 2, 2]]))
    assert np.array_equal(got["box"][9:13], [-1] * 4) and np.isnan(got["bounds"][9:13]).all()
    assert np.array_equal(bits(got["bounds"][13]), bits(good["bounds"][13])) and got["box"][13] == 7
    assert np.isnan(got["bounds"][14:]).all() and (got["box"][14:] == -1).all()
    with pytest.raises(ValueError):
        fiesta_amd.corridor_bounds_model(wv, bad, cor, 0.0)


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_ctypes_mirror_matches_the_header():
    import fiesta_amd
    from fiesta_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct fiesta_hip_bounds_result \{(.*?)\} fiesta_hip_bounds_result;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert [d.split(None, 1)[1].lstrip("*").strip() for d in decls] == [f[0] for f in _lib.BoundsResult._fields_] == ["bounds", "ok", "box"]
    assert [d.split(None, 1)[0] for d in decls] == ["double", "int32_t", "int64_t"] and all(d.split(None, 1)[1].startswith("*") for d in decls)
    assert all(f[1] is C.c_void_p for f in _lib.BoundsResult._fields_)
    assert re.search(r"#define FIESTA_HIP_BOUNDS_VOID_BROKEN 1\b", text) and fiesta_amd.BOUNDS_VOID_BROKEN == 1
    assert "fiesta_hip_corridor_bounds" in _lib.declared_symbols() and "fiesta_hip_corridor_bounds_dev" in _lib.declared_symbols()
    assert re.search(r"return 101;", open(os.path.join(ROOT, "fiesta_amd", "csrc", "c_api.hip")).read())   # the version did not move


def test_whole_call_errors_need_no_device():
    """every whole-call error is reported before the map handle is looked at: with a NULL handle a good call fails on the handle, a
    bad one on its own argument"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd._lib import BoundsResult
    lib = fiesta_amd.load()
    wv, off, cor = hand_made()
    out = np.zeros((len(wv), 6))
    res = BoundsResult(out.ctypes.data, None, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = dict(w=p(wv), n_wp=len(wv), off=p(off), n_paths=len(off) - 1, boff=p(cor["offsets"]), boxes=p(cor["boxes"]), pos=p(cor["boxes_pos"]),
                entry=p(cor["entry"]), status=p(cor["status"]), n_boxes=len(cor["entry"]), inset=0.0, flags=0, r=C.byref(res))

    def call(fn, **kw):
        a = dict(good, **kw)
        st = fn(None, a["w"], a["n_wp"], a["off"], a["n_paths"], a["boff"], a["boxes"], a["pos"], a["entry"], a["status"], a["n_boxes"], a["inset"],
                a["flags"], a["r"])
        return st, fiesta_amd._lib.last_error()

    bad_calls = [dict(n_wp=-1), dict(n_paths=-1), dict(n_boxes=-1), dict(w=None), dict(off=None), dict(boff=None), dict(status=None),
                 dict(boxes=None), dict(pos=None), dict(entry=None), dict(r=None), dict(inset=float("nan")), dict(inset=-1e-12),
                 dict(inset=float("inf")), dict(flags=2), dict(flags=-1), dict(n_paths=2 ** 30 + 1)]
    for fn in (lib.fiesta_hip_corridor_bounds, lib.fiesta_hip_corridor_bounds_dev):
        for bad in bad_calls:
            st, msg = call(fn, **bad)
            assert st == 1 and "corridor_bounds" in msg and "handle" not in msg, (bad, st, msg)
        for fine in (dict(), dict(flags=1), dict(inset=1e300), dict(w=None, n_wp=0, off=p(np.zeros(8, np.int64))),
                     dict(n_paths=0, off=None, boff=None, status=None)):
            st, msg = call(fn, **fine)                                   # nothing wrong but the handle
            assert st == 1 and "null map handle" in msg, (fine, msg)
    z = lambda v: p(np.array(v, np.int64))  # noqa: E731
    # the host variant checks both offset arrays; the device variant cannot
    for kw in (dict(off=z([1, 6, 9, 13, 13, 14, 17, 19])), dict(off=z([0, 6, 9, 13, 13, 14, 17, 18])), dict(off=z([0, 9, 6, 13, 13, 14, 17, 19])),
               dict(boff=z([0, 3, 6, 7, 7, 8, 10, 11])), dict(boff=z([0, 3, 2, 7, 7, 8, 10, 10])), dict(boff=z([-1, 3, 6, 7, 7, 8, 10, 10])),
               dict(n_boxes=9)):
        st, msg = call(lib.fiesta_hip_corridor_bounds, **kw)
        assert st == 1 and ("offsets" in msg or "box range" in msg) and "handle" not in msg, (kw, msg)
        st, msg = call(lib.fiesta_hip_corridor_bounds_dev, **kw)
        assert st == 1 and "null map handle" in msg


# ---- 4. the kernels' resources --------------------------------------------------------------------------------------------------------
def test_bounds_kernels_do_not_spill():
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_corridor_bounds" in k or "k_bounds_fill" in k}
    assert any("k_corridor_bounds" in k for k in res) and any("k_bounds_fill" in k for k in res), sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
