"""CPU side of the reach matrix (fiesta_hip_reach_matrix, include/fiesta_hip.h): the definition and the plumbing.

fiesta_amd.reach_matrix_model is one reach_model run per usable source and -1 rows otherwise; here it is held to that sentence on
a scene with walls, a sealed box, an unknown lump, a blocked, an unknown and an outside source and one voxel listed twice.  Also:
the header declares the two calls, the built library exports them and _lib binds them, the ctypes mirrors follow the header, the
argument rules are checked before any device is touched, and the new kernels use no scratch and spill nothing.  Everything is
integer: comparisons are exact.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fiesta_amd.reach_model import REACH_SITE_BLOCKED, REACH_SITE_OK, REACH_SITE_OUTSIDE, reach_matrix_model, reach_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1
SCENE_SHAPE = (40, 24, 40)
SOURCES = [(2, 12, 20), (38, 12, 20), (9, 1, 3), (6, 12, 20), (33, 11, 11), (33, 10, 12), (21, 12, 33), (2, 12, 20), (45, 0, 0), (15, 16, 31),
           (16, 16, 32)]


def scene():
    """(observed, occupied): all observed and free but walls at x = 6, 12, .. 36 with a 3-voxel gap at y < 3 (even walls) or
    y >= 21 (odd walls), a sealed box around [30:36, 9:13, 9:14] and a never-observed lump"""
    obs = np.ones(SCENE_SHAPE, bool)
    occ = np.zeros(SCENE_SHAPE, bool)
    for k, x in enumerate(range(6, SCENE_SHAPE[0], 6)):
        occ[x] = True
        if k % 2 == 0:
            occ[x, :3] = False
        else:
            occ[x, 21:] = False
    occ[30:36, 8:14, 8] = True
    occ[30:36, 8:14, 14] = True
    occ[30:36, 8, 8:15] = True
    occ[30:36, 13, 8:15] = True
    obs[20:24, 10:20, 30:40] = False
    return obs, occ


def expected_status(flags):
    st = [REACH_SITE_OK] * len(SOURCES)
    st[3] = REACH_SITE_BLOCKED
    st[6] = REACH_SITE_OK if flags & 1 else REACH_SITE_BLOCKED
    st[8] = REACH_SITE_OUTSIDE
    return st


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("flags", [0, 1])
def test_model_is_one_flood_per_usable_source(conn, flags):
    obs, occ = scene()
    got = reach_matrix_model(obs, occ, SOURCES, connectivity=conn, flags=flags)
    cost, status = got["cost"], got["source_status"]
    assert cost.shape == (11, 11) and cost.dtype == np.int32
    assert status.tolist() == expected_status(flags)
    assert got["n_sources_used"] == int((status == REACH_SITE_OK).sum())
    for s in range(len(SOURCES)):
        if status[s] == REACH_SITE_OK:
            r = reach_model(obs, occ, [SOURCES[s]], connectivity=conn, flags=flags, targets=SOURCES)
            assert np.array_equal(cost[s], r["target_cost"]), s
            assert got["source_reached"][s] == r["n_reached"] > 0 and cost[s, s] == 0
        else:
            assert (cost[s] == -1).all() and got["source_reached"][s] == 0
    assert np.array_equal(cost, cost.T)                                  # moves are symmetric, traversability belongs to the voxel
    assert np.array_equal(cost[0], cost[7])                              # the same voxel listed twice
    # the sealed box: its two sources reach each other and nothing else
    assert cost[4, 5] == (6 if conn == 6 else 4)
    others = [j for j in range(11) if j not in (4, 5)]
    assert all(cost[4, j] in (INF, -1) for j in others) and all(cost[5, j] in (INF, -1) for j in others)
    assert cost[0, 1] == (450 if conn == 6 else 378)
    # the reach_field way (an unusable seed leaves INT32_MAX on traversable targets) is NOT symmetric: the -1 rows are the point
    field_way = reach_model(obs, occ, [SOURCES[3]], connectivity=conn, flags=flags, targets=SOURCES)["target_cost"]
    assert field_way[0] == INF and cost[0, 3] == -1


def test_model_rectangular_box_and_empty_cases():
    obs, occ = scene()
    cols = [(1, 1, 1), (6, 12, 20), (50, 0, 0), (9, 1, 3)]
    got = reach_matrix_model(obs, occ, SOURCES[:4], targets=cols)
    assert got["cost"].shape == (4, 4) and got["cost"][2].tolist()[1:] == [-1, -1, 0] and (got["cost"][3] == -1).all()
    lo, hi = (3, 2, 5), (37, 21, 36)
    boxed = reach_matrix_model(obs, occ, SOURCES, lo=lo, hi=hi)
    want = [REACH_SITE_OUTSIDE, REACH_SITE_OUTSIDE, REACH_SITE_OUTSIDE, REACH_SITE_BLOCKED, REACH_SITE_OK, REACH_SITE_OK, REACH_SITE_BLOCKED,
            REACH_SITE_OUTSIDE, REACH_SITE_OUTSIDE, REACH_SITE_OK, REACH_SITE_OK]
    assert boxed["source_status"].tolist() == want and boxed["box_lo"] == list(lo) and boxed["box_hi"] == list(hi)
    none = reach_matrix_model(obs, occ, np.zeros((0, 3), np.int32))
    assert none["cost"].shape == (0, 0) and none["n_traversable"] == int((obs & ~occ).sum()) and none["box_hi"] == [39, 23, 39]
    empty = reach_matrix_model(obs, occ, SOURCES, lo=(5, 5, 5), hi=(4, 9, 9))
    assert (empty["cost"] == -1).all() and (empty["source_status"] == REACH_SITE_OUTSIDE).all() and empty["n_traversable"] == 0
    assert empty["box_lo"] == [0, 0, 0] and empty["box_hi"] == [0, 0, 0] and empty["n_sources_used"] == 0


def test_header_library_and_bindings_agree():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    assert fiesta_amd.reach_matrix_model is reach_matrix_model
    names = ("fiesta_hip_reach_matrix", "fiesta_hip_reach_matrix_dev")
    assert all(n in _lib.declared_symbols() for n in names)
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    for n in names:
        assert n in lib._fiesta_signatures and getattr(lib, n) is not None
    text = open(_lib.HEADER_PATH).read()
    for struct, mirror in (("fiesta_hip_reach_matrix_result", _lib.ReachMatrixResult), ("fiesta_hip_reach_matrix_info", _lib.ReachMatrixInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[.*?\]", "", n).strip(" *") for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(_lib.ReachMatrixInfo) == 6 * 4 + 6 * 8 and C.sizeof(_lib.ReachMatrixResult) == 3 * C.sizeof(C.c_void_p)
    for name, value in (("OK", REACH_SITE_OK), ("OUTSIDE", REACH_SITE_OUTSIDE), ("BLOCKED", REACH_SITE_BLOCKED)):
        assert re.search(r"#define FIESTA_HIP_REACH_SITE_%s (\d+)" % name, text).group(1) == str(value)
    assert "retain" in re.search(r"---- reach matrix.*?#define FIESTA_HIP_REACH_SITE_OK", text, re.S).group(0).lower()


def test_argument_rules_are_checked_before_any_device_use():
    """every whole-call error that needs no map is refused, with its own message, before the handle is looked at"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    lib = fiesta_amd.load()
    box = (C.c_int32 * 3)(0, 0, 0)
    pts = (C.c_int32 * 3)(1, 1, 1)
    out = (C.c_int32 * 1)(77)
    res = _lib.ReachMatrixResult(C.cast(out, C.c_void_p), None, None)
    nan = float("nan")
    #        lo   hi   sources n targets n clearance conn flags max_fields result   the message names
    cases = [(box, box, pts, 1, None, 0, 0.0, 26, 0, 0, None, "result"),
             (box, box, pts, 1, None, 0, nan, 26, 0, 0, res, "NaN"),
             (box, None, pts, 1, None, 0, 0.0, 26, 0, 0, res, "lo and hi"),
             (None, box, pts, 1, None, 0, 0.0, 26, 0, 0, res, "lo and hi"),
             (box, box, pts, 1, None, 0, 0.0, 18, 0, 0, res, "connectivity"),
             (box, box, pts, 1, None, 0, 0.0, 26, 2, 0, res, "flag"),
             (box, box, pts, 1, None, 0, 0.0, 26, 0, -1, res, "max_fields"),
             (box, box, pts, -1, None, 0, 0.0, 26, 0, 0, res, "negative"),
             (box, box, pts, 1, pts, -1, 0.0, 26, 0, 0, res, "negative"),
             (box, box, None, 1, None, 0, 0.0, 26, 0, 0, res, "sources"),
             (box, box, pts, 1, None, 1, 0.0, 26, 0, 0, res, "targets"),
             (box, box, pts, 2 ** 15, pts, 2 ** 14, 0.0, 26, 0, 0, res, "2^28"),
             (box, box, pts, 2 ** 15, None, 0, 0.0, 26, 0, 0, res, "2^28"),
             (box, box, pts, 1, pts, 1, 0.0, 26, 1, 4, res, "null map")]     # nothing wrong but the missing map
    for fn in (lib.fiesta_hip_reach_matrix, lib.fiesta_hip_reach_matrix_dev):
        for lo, hi, src, ns, tg, nt, clr, conn, flags, mf, r, word in cases:
            st = fn(None, lo, hi, src, ns, tg, nt, clr, conn, flags, mf, C.byref(r) if r is not None else None, None)
            assert st == 1, (word, st)                                       # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    assert out[0] == 77


def test_reach_matrix_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_rmx_" in k}
    for kernel, copies in (("k_rmx_init", 1), ("k_rmx_seed", 1), ("k_rmx_relax", 2), ("k_rmx_gather", 1), ("k_rmx_count", 1)):
        assert sum(kernel in k for k in res) == copies, (kernel, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
