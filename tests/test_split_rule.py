"""The rule of fiesta_hip_split_clusters (include/fiesta_hip.h) without a GPU.

fiesta_amd.split_model is the definition, a literal recursion.  It is held to hand-worked cases (the line, the axis tie, the
max_depth cut, an empty segment, a member listed twice) and, on seeded random clusters, to the properties the rule promises:
the parts of a cluster partition its members, nothing is left oversize at max_depth 63, low comes before high, the split is
idempotent and the identity case equals fiesta_amd.cluster_model.  Then the ctypes mirror against the header, every whole-call
error through the built library (none needs a device), and the resources of the new kernels.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, ORG = 0.25, (-3.0, 1.5, 0.0)
PER_PART = ("parent", "depth", "size", "root", "box_lo", "box_hi", "centroid", "mask_or", "key_min", "key_argmin")


def one_cluster(vox):
    v = np.asarray(vox, np.int32).reshape(-1, 3)
    return v, np.array([0, len(v)], np.int64), np.arange(len(v), dtype=np.int64)


def segments(out):
    return [sorted(out["members"][out["offsets"][p]:out["offsets"][p + 1]].tolist()) for p in range(out["n_parts"])]


def random_clusters(seed):
    """a few blobs, sheets and lines as clusters of one entry list, with a mask and a key; the CSR pair lists every cluster's entries
    in a shuffled order"""
    rng = np.random.RandomState(seed)
    vox, off, mem = [], [0], []
    for k in range(int(rng.randint(3, 7))):
        kind = rng.randint(0, 3)
        m = int(rng.choice([1, 2, 7, 64, 65, 200]))
        base = rng.randint(-500, 500, 3)
        if kind == 0:                                                    # (distinct voxels, as the cluster call lists them)
            c = base + np.stack(np.unravel_index(rng.choice(12 ** 3, m, replace=False), (12, 12, 12)), axis=1)
        elif kind == 1:
            c = base + np.stack(np.unravel_index(rng.choice(40 * 40, m, replace=False), (40, 40, 1)), axis=1)
        else:
            c = base + np.arange(m)[:, None] * np.array([1, 1, 0]) * int(rng.randint(1, 4))
        idx = len(vox) + rng.permutation(m)
        vox.extend(c.tolist()), mem.extend(idx.tolist()), off.append(len(mem))
        if k == 1:
            off.append(len(mem))                                         # an empty segment
    v = np.array(vox, np.int32)
    return (v, np.array(off, np.int64), np.array(mem, np.int64), rng.randint(0, 256, len(v)).astype(np.uint8),
            rng.randint(-3, 50, len(v)).astype(np.int32))


# ---- 1. hand-worked cases -------------------------------------------------------------------------------------------------------------
def test_a_line_of_ten_with_max_size_three():
    import fiesta_amd
    v, off, mem = one_cluster([[x, 0, 0] for x in range(10)])
    out = fiesta_amd.split_model(v, off, mem, max_size=3, resolution=RES, origin=ORG)
    assert segments(out) == [[0, 1, 2], [3, 4], [5, 6, 7], [8, 9]]
    assert out["n_parts"] == 4 and out["n_members"] == 10 and out["n_split_clusters"] == 1 and out["n_oversize"] == 0
    assert out["largest"] == 3 and out["deepest"] == 2 and out["status"] == fiesta_amd.SPLIT_OK
    assert out["parent"].tolist() == [0] * 4 and out["depth"].tolist() == [2] * 4 and out["depth"].dtype == np.uint8
    assert out["size"].tolist() == [3, 2, 3, 2] and out["root"].tolist() == [0, 3, 5, 8]
    assert out["box_lo"][:, 0].tolist() == [0, 3, 5, 8] and out["box_hi"][:, 0].tolist() == [2, 4, 7, 9]
    assert out["label"].tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3] and out["offsets"].tolist() == [0, 3, 5, 8, 10]
    assert out["centroid"][1].tolist() == [(7.0 / 2.0 + 0.5) * RES + ORG[0], 0.5 * RES + ORG[1], 0.5 * RES + ORG[2]]


def test_the_axis_tie_goes_to_the_lowest_axis():
    import fiesta_amd
    v, off, mem = one_cluster([[x, y, 7] for x in range(4) for y in range(4)])
    out = fiesta_amd.split_model(v, off, mem, max_size=8)
    assert out["n_parts"] == 2                                           # x and y tie at extent 4: cut along x
    assert out["box_lo"].tolist() == [[0, 0, 7], [2, 0, 7]] and out["box_hi"].tolist() == [[1, 3, 7], [3, 3, 7]]
    out = fiesta_amd.split_model(v[:, [2, 0, 1]], off, mem, max_size=8)   # the sheet in the y-z plane: y and z tie, cut along y
    assert out["box_lo"].tolist() == [[7, 0, 0], [7, 2, 0]] and out["box_hi"].tolist() == [[7, 1, 3], [7, 3, 3]]
    out = fiesta_amd.split_model(v, off, mem, max_extent=2)               # x first, then each half along y
    assert out["n_parts"] == 4 and out["box_lo"].tolist() == [[0, 0, 7], [0, 2, 7], [2, 0, 7], [2, 2, 7]]


def test_max_depth_cuts_the_recursion_and_counts_what_it_left():
    import fiesta_amd
    v, off, mem = one_cluster([[x, 0, 0] for x in range(16)])
    for depth, parts in ((0, 1), (1, 2), (2, 4), (3, 8)):
        out = fiesta_amd.split_model(v, off, mem, max_size=1, max_depth=depth)
        assert out["n_parts"] == parts and out["n_oversize"] == parts and out["deepest"] == depth and out["largest"] == 16 >> depth
        assert out["n_split_clusters"] == (depth > 0)
    out = fiesta_amd.split_model(v, off, mem, max_size=1, max_depth=4)
    assert out["n_parts"] == 16 and out["n_oversize"] == 0 and out["deepest"] == 4
    with pytest.raises(ValueError):
        fiesta_amd.split_model(v, off, mem, max_size=1, max_depth=64)
    with pytest.raises(ValueError):
        fiesta_amd.split_model(v, off, mem, max_size=-1)


def test_an_empty_segment_yields_no_part():
    import fiesta_amd
    v = np.array([[0, 0, 0], [1, 0, 0], [9, 9, 9]], np.int32)
    out = fiesta_amd.split_model(v, np.array([0, 2, 2, 3, 3], np.int64), np.array([1, 0, 2], np.int64), max_size=1)
    assert out["parent"].tolist() == [0, 0, 2] and segments(out) == [[0], [1], [2]] and out["n_split_clusters"] == 1
    out = fiesta_amd.split_model(v, np.array([0, 0, 0], np.int64), np.zeros(0, np.int64), max_size=1)
    assert out["n_parts"] == 0 and out["offsets"].tolist() == [0] and (out["label"] == -1).all()
    out = fiesta_amd.split_model(v, np.array([1, 3], np.int64), np.array([2, 1, 0], np.int64), max_size=1)   # position 0 belongs to no part
    assert out["offsets"].tolist() == [1, 2, 3] and out["members"].tolist() == [2, 0, 1] and out["label"].tolist() == [0, 1, -1]
    assert out["n_members"] == 3


def test_a_member_listed_twice_counts_twice():
    import fiesta_amd
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], np.int32)
    off, mem = np.array([0, 5, 7], np.int64), np.array([0, 1, 1, 2, 3, 3, 0], np.int64)
    key = np.array([5, -1, 2, 2], np.int32)
    out = fiesta_amd.split_model(v, off, mem, key=key, mask=np.array([1, 2, 4, 8], np.uint8), max_size=3)
    assert segments(out) == [[0, 1, 1], [2, 3], [0, 3]] and out["size"].tolist() == [3, 2, 2]
    assert out["centroid"][0, 0] == 2.0 / 3.0 + 0.5                     # (0 + 1 + 1) / 3
    assert out["label"].tolist() == [2, 0, 1, 2]                         # entries 0 and 3: the largest part index wins
    assert out["key_min"].tolist() == [5, 2, 2] and out["key_argmin"].tolist() == [0, 2, 3] and out["mask_or"].tolist() == [3, 12, 9]
    # members of ONE voxel cannot be cut: the part stays oversize, whatever max_depth
    out = fiesta_amd.split_model(v, np.array([0, 4], np.int64), np.array([2, 1, 1, 1], np.int64), max_size=1)
    assert segments(out) == [[1, 1, 1], [2]] and out["n_oversize"] == 1 and out["deepest"] == 1 and out["largest"] == 3


def test_data_errors():
    import fiesta_amd
    v = np.array([[0, 0, 0], [1, 0, 0], [2 ** 20 - 1, 0, 0]], np.int32)
    ok_off, ok_mem = np.array([0, 2], np.int64), np.array([0, 1], np.int64)
    bad = [(np.array([-1, 2], np.int64), ok_mem), (np.array([0, 2, 1], np.int64), ok_mem), (np.array([0, 3], np.int64), ok_mem),
           (ok_off, np.array([0, 3], np.int64)), (ok_off, np.array([-1, 0], np.int64)), (ok_off, np.array([0, 2], np.int64))]
    for off, mem in bad:
        with pytest.raises(ValueError):
            fiesta_amd.split_model(v, off, mem, max_size=1)
        out = fiesta_amd.split_model(v, off, mem, max_size=1, device=True)
        assert out["status"] == fiesta_amd.SPLIT_INVALID and out["n_parts"] == 0 and (out["label"] == -1).all() and out["n_members"] == 0
    assert fiesta_amd.split_model(v, ok_off, ok_mem, max_size=1)["n_parts"] == 2
    # the effective cluster count cuts the offsets: what lies beyond it is not read
    out = fiesta_amd.split_model(v, np.array([0, 2, 1], np.int64), ok_mem, max_size=1, n_clusters=1)
    assert out["n_parts"] == 2 and out["status"] == fiesta_amd.SPLIT_OK


# ---- 2. the promised properties on random clusters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_properties_on_random_clusters(seed):
    import fiesta_amd
    from fiesta_amd.split_model import split_oversize
    v, off, mem, mask, key = random_clusters(seed)
    for max_size, max_extent in ((5, 0), (0, 6), (40, 9), (1, 0), (0, 1)):
        out = fiesta_amd.split_model(v, off, mem, mask, key, max_size, max_extent, 63, RES, ORG)
        segs = segments(out)
        P = out["n_parts"]
        assert out["deepest"] <= 63 and out["n_oversize"] == 0 and out["status"] == 0 and out["n_members"] == len(mem)
        assert out["members"].shape == mem.shape and out["offsets"][0] == 0 and out["offsets"][-1] == len(mem)
        for k in range(len(off) - 1):                                    # the parts of a cluster partition its members
            mine = [p for p in range(P) if out["parent"][p] == k]
            assert mine == list(range(mine[0], mine[-1] + 1)) if mine else off[k] == off[k + 1]
            assert sorted(i for p in mine for i in segs[p]) == sorted(mem[off[k]:off[k + 1]].tolist())
        assert (np.diff(out["parent"]) >= 0).all()                       # cluster-major
        for p in range(P):
            ext = (out["box_hi"][p].astype(np.int64) - out["box_lo"][p] + 1).tolist()
            assert not split_oversize(out["size"][p], ext, max_size, max_extent) and out["size"][p] == len(segs[p]) > 0
            assert out["root"][p] == min(segs[p]) and np.array_equal(out["box_lo"][p], v[segs[p]].min(axis=0))
        # low before high: two neighbours of one cluster are separated by the plane of their last common cut, the earlier one below it
        for p in range(P - 1):
            if out["parent"][p] == out["parent"][p + 1]:
                assert any(out["box_hi"][p][a] < out["box_lo"][p + 1][a] for a in range(3)), (p, out["box_lo"][p:p + 2], out["box_hi"][p:p + 2])
        assert out["n_split_clusters"] == len({int(out["parent"][p]) for p in range(P) if out["depth"][p] > 0})
        # idempotent: the parts as clusters come back as they are
        again = fiesta_amd.split_model(v, out["offsets"], out["members"], mask, key, max_size, max_extent, 63, RES, ORG)
        assert again["n_parts"] == P and again["deepest"] == 0 and again["n_split_clusters"] == 0 and segments(again) == segs
        assert again["parent"].tolist() == list(range(P))
        for name in PER_PART[2:] + ("offsets", "members", "label"):
            assert np.array_equal(again[name], out[name]), name
        # max_depth below what the recursion used leaves something oversize, and only cuts
        if out["deepest"] > 0:
            cut = fiesta_amd.split_model(v, off, mem, mask, key, max_size, max_extent, int(out["deepest"]) - 1, RES, ORG)
            assert cut["n_oversize"] >= 1 and cut["n_parts"] < P and cut["deepest"] == out["deepest"] - 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_identity_case_equals_the_cluster_model(seed):
    import fiesta_amd
    rng = np.random.RandomState(seed)
    v = rng.randint(-6, 6, (300, 3)).astype(np.int32)
    v[7] = [2 ** 20, 0, 0]                                               # an invalid entry; duplicates come by themselves
    mask, key = rng.randint(0, 256, 300).astype(np.uint8), rng.randint(-2, 30, 300).astype(np.int32)
    cl = fiesta_amd.cluster_model(v, mask, key, connectivity=6, min_size=2, resolution=RES, origin=ORG)
    for depth in (0, 63):
        out = fiesta_amd.split_model(v, cl["offsets"], cl["members"], mask, key, 0, 0, depth, RES, ORG)
        assert out["n_parts"] == cl["n_clusters"] and out["n_members"] == cl["n_members"] and out["largest"] == cl["largest"]
        assert out["parent"].tolist() == list(range(cl["n_clusters"])) and not out["depth"].any() and out["deepest"] == 0
        for name in PER_PART[2:] + ("offsets", "members"):
            assert out[name].dtype == cl[name].dtype and np.array_equal(out[name], cl[name]), name
        assert np.array_equal(out["centroid"].view(np.int64), cl["centroid"].view(np.int64))
        # (the cluster call labels later duplicates too; the split labels what the segments list: the representatives)
        listed = np.zeros(300, bool)
        listed[cl["members"]] = True
        assert np.array_equal(out["label"][listed], cl["label"][listed]) and (out["label"][~listed] == -1).all()


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------------------------
def struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    return [(d.split(None, 1)[0], d.split(None, 1)[1]) for d in decls]


def test_the_ctypes_mirror_matches_the_header():
    import fiesta_amd
    from fiesta_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    res = struct_fields(text, "fiesta_hip_split_result")
    assert [n.lstrip("*").strip() for _, n in res] == [f[0] for f in _lib.SplitResult._fields_] == list(PER_PART) + ["offsets", "members", "label"]
    assert [t for t, _ in res] == ["int32_t", "uint8_t", "int32_t", "int64_t", "int32_t", "int32_t", "double", "uint8_t", "int32_t", "int64_t", "int64_t",
                                   "int64_t", "int32_t"]
    assert all(n.startswith("*") for _, n in res) and all(f[1] is C.c_void_p for f in _lib.SplitResult._fields_)
    info = struct_fields(text, "fiesta_hip_split_info")
    assert [n for _, n in info] == [f[0] for f in _lib.SplitInfo._fields_] == ["n_parts", "n_members", "n_split_clusters", "n_oversize", "largest", "depth",
                                                                              "status"]
    assert all(t == "int64_t" for t, _ in info) and all(f[1] is C.c_int64 for f in _lib.SplitInfo._fields_)
    for name, value in (("MAX_DEPTH", 63), ("OK", 0), ("INVALID", 1)):
        assert re.search(r"#define FIESTA_HIP_SPLIT_%s %d\b" % (name, value), text) and getattr(fiesta_amd, "SPLIT_" + name) == value
    assert "fiesta_hip_split_clusters" in _lib.declared_symbols() and "fiesta_hip_split_clusters_dev" in _lib.declared_symbols()
    assert "need not be connected" in text.lower() and "must not overlap inputs" in text.lower()
    assert re.search(r"return 101;", open(os.path.join(ROOT, "fiesta_amd", "csrc", "c_api.hip")).read())   # the version did not move


def test_whole_call_errors_need_no_device():
    """every whole-call error, and for the host variant every data error, is reported before the map handle is looked at: with a NULL
    handle a good call fails on the handle, a bad one on its own argument"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd._lib import SplitInfo, SplitResult
    lib = fiesta_amd.load()
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2 ** 20 - 1, 0, 0]], np.int32)
    off, mem = np.array([0, 2, 3], np.int64), np.array([0, 1, 2], np.int64)
    size = np.zeros(8, np.int32)
    res = SplitResult(size=size.ctypes.data)
    info = SplitInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = dict(vox=p(v), mask=None, key=None, n=4, off=p(off), mem=p(mem), K=2, M=3, max_size=1, max_extent=0, max_depth=63, cap=8, r=C.byref(res),
                info=C.byref(info))

    def call(dev, **kw):
        a = dict(good, **kw)
        head = (None, a["vox"], a["mask"], a["key"], a["n"], a["off"], a["mem"], a["K"])
        tail = (a["M"], a["max_size"], a["max_extent"], a["max_depth"], a["cap"], a["r"], a["info"])
        st = lib.fiesta_hip_split_clusters_dev(*head, None, *tail) if dev else lib.fiesta_hip_split_clusters(*head, *tail)
        return st, fiesta_amd._lib.last_error()

    bad_calls = [dict(n=-1), dict(n=2 ** 24 + 1), dict(K=-1), dict(K=2 ** 24 + 1), dict(M=-1), dict(M=2 ** 24 + 1), dict(max_size=-1),
                 dict(max_extent=-1), dict(max_depth=-1), dict(max_depth=64), dict(vox=None), dict(off=None), dict(mem=None), dict(info=None),
                 dict(cap=-1)]
    z = lambda a: p(np.array(a, np.int64))  # noqa: E731
    data_errors = [dict(off=z([-1, 2, 3])), dict(off=z([0, 3, 2])), dict(off=z([0, 2, 4])), dict(M=2), dict(mem=z([0, 1, 4])), dict(mem=z([0, -1, 2])),
                   dict(mem=z([0, 1, 3])), dict(n=2)]
    for dev in (False, True):
        for bad in bad_calls:
            st, msg = call(dev, **bad)
            assert st == 1 and "split_clusters" in msg and "handle" not in msg, (bad, st, msg)
        for fine in (dict(), dict(r=None), dict(max_size=0, max_depth=0), dict(vox=None, n=0, K=0, M=0, off=None, mem=None), dict(K=0, off=None),
                     dict(cap=0), dict(off=z([1, 2, 3])), dict(max_extent=2 ** 31 - 1)):
            st, msg = call(dev, **fine)                                  # nothing wrong but the handle
            assert st == 1 and "null map handle" in msg, (fine, msg)
        for bad in data_errors:                                          # the host variant refuses them, the device variant cannot see them
            st, msg = call(dev, **bad)
            assert st == 1 and (("null map handle" in msg) if dev else ("split_clusters" in msg and "handle" not in msg)), (dev, bad, msg)


# ---- 4. the kernels' resources --------------------------------------------------------------------------------------------------------
def test_split_kernels_do_not_spill():
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_split_" in k}
    for name in ("init", "validate", "seed", "partial", "scan", "rescan", "first", "box", "decide", "scatter", "acc_init", "stats", "finish", "info"):
        assert any("k_split_" + name in k for k in res), (name, sorted(res))
    for k, v in res.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
