"""CPU side of the leg paths (fiesta_hip_leg_paths, include/fiesta_hip.h): the definition and the plumbing.

fiesta_amd.leg_paths_model is one reach_model flood per distinct usable source and reach_paths_model on it; here it is held to
literal properties on the scene of tests/test_reach_matrix_rule.py, whose sources include a blocked, an unknown and an outside
one, a voxel listed twice and the sealed pair 4 <-> 5.  Also: the header declares the two calls, the built library exports them
and _lib binds them, the ctypes mirrors follow the header, the argument rules are checked before any map is looked at, and the new
kernels use no scratch and spill nothing.  Everything is integer: comparisons are exact.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fiesta_amd.reach_model import (LEG_BAD_INDEX, LEG_NO_SOURCE, REACH_PATH_BLOCKED, REACH_PATH_OK, REACH_PATH_OUTSIDE, REACH_PATH_UNREACHED,
                                    REACH_SITE_OK, leg_paths_model, reach_matrix_model, reach_moves, reach_visible)
from test_reach_matrix_rule import SOURCES, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1
N = len(SOURCES)
# every (from, to) pair, then indices that are none: -1 and n, as a source and as a target
PAIRS = [(a, b) for a in range(N) for b in range(N)] + [(-1, 0), (N, 0), (0, -1), (0, N), (-1, N), (3, N)]
FROM, TO = [p[0] for p in PAIRS], [p[1] for p in PAIRS]


def leg(r, k):
    return r["waypoints_vox"][r["offsets"][k]:r["offsets"][k + 1]].astype(np.int64)


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("flags", [0, 1])
def test_model_against_literal_properties(conn, flags):
    obs, occ = scene()
    trav = (obs & ~occ) | (~obs if flags else np.zeros_like(obs))
    floods = {}
    kw = dict(connectivity=conn, flags=flags, floods=floods, origin=(0.5, -1.0, 2.0), resolution=0.25)
    raw = leg_paths_model(obs, occ, SOURCES, FROM, to=TO, **kw)
    tight = leg_paths_model(obs, occ, SOURCES, FROM, to=TO, path_flags=1, max_span=4096, **kw)
    short = leg_paths_model(obs, occ, SOURCES, FROM, to=TO, path_flags=1, max_span=8, **kw)
    matrix = reach_matrix_model(obs, occ, SOURCES, connectivity=conn, flags=flags)
    site_ok = matrix["source_status"] == REACH_SITE_OK
    weight = {(dx, dy, dz): w for dx, dy, dz, w in reach_moves(conn)}
    assert raw["box_lo"] == [0, 0, 0] and raw["box_hi"] == [39, 23, 39] and raw["connectivity"] == conn and raw["n_sources"] == N
    assert raw["offsets"].dtype == np.int64 and raw["waypoints_vox"].dtype == np.int32 and raw["waypoints_pos"].dtype == np.float64
    assert all(raw[k].dtype == np.int32 and raw[k].shape == (len(PAIRS),) for k in ("status", "n_moves", "cost"))
    seen = set()
    for k, (a, b) in enumerate(PAIRS):
        st = int(raw["status"][k])
        seen.add(st)
        assert st == tight["status"][k] == short["status"][k] and raw["cost"][k] == tight["cost"][k] == short["cost"][k], k
        if not (0 <= a < N and 0 <= b < N):                              # precedence: a bad index beats an unusable source ((3, N))
            assert st == LEG_BAD_INDEX and raw["cost"][k] == -1
        elif not site_ok[a]:
            assert st == LEG_NO_SOURCE and raw["cost"][k] == -1
        else:
            assert raw["cost"][k] == matrix["cost"][a, b], (a, b)
            c = int(matrix["cost"][a, b])
            assert st == (REACH_PATH_OK if 0 <= c < INF else REACH_PATH_UNREACHED if c == INF else
                          REACH_PATH_OUTSIDE if np.any(np.array(SOURCES[b]) > 39) else REACH_PATH_BLOCKED), (a, b, st, c)
        w = leg(raw, k)
        if st != REACH_PATH_OK:
            assert len(w) == 0 and raw["n_moves"][k] == -1 and len(leg(tight, k)) == 0 and tight["n_moves"][k] == -1
            continue
        # a raw leg: from the source voxel to the target voxel by moves of the connectivity whose weights sum to the cost
        assert tuple(w[0]) == SOURCES[a] and tuple(w[-1]) == SOURCES[b] and len(w) == raw["n_moves"][k] + 1
        steps = np.diff(w, axis=0)
        assert all(tuple(s) in weight for s in steps.tolist()), (a, b)
        assert sum(weight[tuple(s)] for s in steps.tolist()) == raw["cost"][k] == matrix["cost"][a, b]
        assert trav[w[:, 0], w[:, 1], w[:, 2]].all()
        if a == b:
            assert len(w) == 1 and raw["n_moves"][k] == 0 and raw["cost"][k] == 0
        # shortcut legs: a subsequence of the raw waypoints with the same ends, every segment visible on the source's flood
        field = floods[a]
        for r, span in ((tight, 4096), (short, 8)):
            t = leg(r, k)
            assert r["n_moves"][k] == raw["n_moves"][k] and tuple(t[0]) == SOURCES[a] and tuple(t[-1]) == SOURCES[b]
            at = 0
            for v in t.tolist():                                         # (a descent visits no voxel twice: its cost falls)
                at = next(i for i in range(at, len(w)) if w[i].tolist() == v) + 1
            idx = [next(i for i in range(len(w)) if w[i].tolist() == v) for v in t.tolist()]
            assert all(0 < j - i <= span for i, j in zip(idx, idx[1:]))
            for p, q in zip(t[1:].tolist(), t[:-1].tolist()):            # (visible() is tested from the target side)
                if max(abs(p[c] - q[c]) for c in range(3)) > 1 or conn == 6:
                    assert reach_visible(field["cost"], field["box_lo"], p, q), (a, b, p, q)
        assert len(leg(tight, k)) <= len(leg(short, k)) <= len(w)
    # every status that a fixed point can give (BROKEN needs a field that is none: the planes are floods)
    assert seen == {REACH_PATH_OK, REACH_PATH_OUTSIDE, REACH_PATH_BLOCKED, REACH_PATH_UNREACHED, LEG_NO_SOURCE, LEG_BAD_INDEX}
    k45 = PAIRS.index((4, 5))
    assert raw["status"][k45] == REACH_PATH_OK and raw["cost"][k45] == (6 if conn == 6 else 4)     # the sealed pair reach each other
    assert raw["status"][PAIRS.index((0, 4))] == REACH_PATH_UNREACHED and raw["status"][PAIRS.index((5, 1))] == REACH_PATH_UNREACHED
    assert raw["n_moves"].max() > 64 and tight["offsets"][-1] < short["offsets"][-1] < raw["offsets"][-1]
    assert np.array_equal(raw["waypoints_pos"], (raw["waypoints_vox"].astype(np.float64) + 0.5) * 0.25 + np.array((0.5, -1.0, 2.0)))
    # to_vox agrees with to on the sites' voxels (bad target indices have no voxel: those legs are left out)
    keep = [k for k, (a, b) in enumerate(PAIRS) if 0 <= b < N]
    for want, pf in ((raw, 0), (tight, 1)):
        got = leg_paths_model(obs, occ, SOURCES, [FROM[k] for k in keep], to_vox=[SOURCES[TO[k]] for k in keep], path_flags=pf, **kw)
        for name in ("status", "n_moves", "cost"):
            assert np.array_equal(got[name], want[name][keep]), name
        for j, k in enumerate(keep):
            assert np.array_equal(leg(got, j), leg(want, k)), k
    # a voxel that is no site, inside and outside the box
    extra = leg_paths_model(obs, occ, SOURCES, [0, 0, 3], to_vox=[(1, 1, 1), (40, 0, 0), (1, 1, 1)], **kw)
    assert extra["status"].tolist() == [REACH_PATH_OK, REACH_PATH_OUTSIDE, LEG_NO_SOURCE] and extra["cost"][1] == extra["cost"][2] == -1
    assert extra["cost"][0] == floods[0]["cost"][1, 1, 1] > 0 and tuple(leg(extra, 0)[-1]) == (1, 1, 1)


def test_model_argument_rules():
    obs, occ = scene()
    with pytest.raises(ValueError):
        leg_paths_model(obs, occ, SOURCES, [0])
    with pytest.raises(ValueError):
        leg_paths_model(obs, occ, SOURCES, [0], to=[1], to_vox=[(1, 1, 1)])
    with pytest.raises(ValueError):
        leg_paths_model(obs, occ, SOURCES, [0], to=[1], lo=(5, 5, 5), hi=(4, 9, 9))          # an empty box retains nothing
    with pytest.raises(ValueError):
        leg_paths_model(obs, occ, np.zeros((0, 3), np.int32), [0], to=[0])
    none = leg_paths_model(obs, occ, SOURCES, [], to=[])
    assert none["offsets"].tolist() == [0] and none["waypoints_vox"].shape == (0, 3) and none["n_sources"] == N


def test_header_library_and_bindings_agree():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    assert fiesta_amd.leg_paths_model is leg_paths_model
    names = ("fiesta_hip_leg_paths", "fiesta_hip_leg_paths_dev")
    assert all(n in _lib.declared_symbols() for n in names)
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    for n in names:
        assert n in lib._fiesta_signatures and getattr(lib, n) is not None
    text = open(_lib.HEADER_PATH).read()
    for struct, mirror in (("fiesta_hip_leg_paths_result", _lib.LegPathsResult), ("fiesta_hip_leg_paths_info", _lib.LegPathsInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[.*?\]", "", n).strip(" *") for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(_lib.LegPathsInfo) == 8 * 4 + 8 and C.sizeof(_lib.LegPathsResult) == 6 * C.sizeof(C.c_void_p)
    for name, value in (("NO_SOURCE", LEG_NO_SOURCE), ("BAD_INDEX", LEG_BAD_INDEX)):
        assert re.search(r"#define FIESTA_HIP_LEG_%s (\d+)" % name, text).group(1) == str(value)
    assert (LEG_NO_SOURCE, LEG_BAD_INDEX) == (5, 6)
    # the reach matrix's section still says what is retained, the old sentence and the new rule
    section = re.search(r"---- reach matrix.*?#define FIESTA_HIP_REACH_SITE_OK", text, re.S).group(0)
    assert "The field that fiesta_hip_reach_paths RETAINS is left alone" in section and "fiesta_hip_leg_paths" in section
    assert "retain" in section.lower()
    for method in ("LegPaths", "LegPathsDevice", "TourRoute"):
        assert callable(getattr(fiesta_amd.ESDFMap, method))


def test_argument_rules_are_checked_before_any_device_use():
    """every whole-call error that needs no map is refused, with its own message, before the handle is looked at"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    lib = fiesta_amd.load()
    idx = (C.c_int32 * 1)(0)
    vox = (C.c_int32 * 3)(1, 1, 1)
    off = (C.c_int64 * 2)(77, 77)
    res = _lib.LegPathsResult(C.cast(off, C.c_void_p), None, None, None, None, None)
    no_off = _lib.LegPathsResult(None, None, None, None, None, None)
    #        from to    to_vox n flags span capacity result  the message names
    cases = [(idx, idx, None, 1, 0, 1, 0, None, "result"),
             (idx, idx, None, 1, 0, 1, 0, no_off, "offsets"),
             (idx, idx, None, -1, 0, 1, 0, res, "negative count"),
             (idx, idx, None, 1, 0, 1, -1, res, "negative capacity"),
             (idx, idx, None, 1, 2, 1, 0, res, "flag"),
             (idx, idx, None, 1, 1, 0, 0, res, "max_span"),
             (None, idx, None, 1, 0, 1, 0, res, "from"),
             (idx, idx, vox, 1, 0, 1, 0, res, "exactly one"),
             (idx, None, None, 1, 0, 1, 0, res, "exactly one"),
             (idx, None, vox, 1, 1, 1, 0, res, "null map"),              # nothing wrong but the missing map
             (None, None, None, 0, 0, 0, 0, res, "null map")]            # ... and an empty batch
    info = _lib.LegPathsInfo()
    info.n_sources = -5
    for fn in (lib.fiesta_hip_leg_paths, lib.fiesta_hip_leg_paths_dev):
        for fr, to, tv, n, flags, span, cap, r, word in cases:
            st = fn(None, fr, to, tv, n, flags, span, cap, C.byref(r) if r is not None else None, C.byref(info))
            assert st == 1, (word, st)                                   # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    assert list(off) == [77, 77] and info.n_sources == -5


def test_leg_path_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_leg_path_" in k}
    for kernel, copies in (("k_leg_path_count", 2), ("k_leg_path_write", 2)):
        assert sum(kernel in k for k in res) == copies, (kernel, sorted(res))
    for k, v in res.items():
        assert "k_reach_path_" not in k and "k_rmx_" not in k, k         # (other tests count kernels by those substrings)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
