"""Cluster splitting on the GPU (fiesta_hip_split_clusters[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/split_kernels.hpp).

The expected result is always fiesta_amd.split_model (the header's definition in plain Python; tests/test_split_rule.py checks it
against hand-worked cases and its own promises).  Every comparison is exact: integers equal, centroids equal as f64 BITS, member
segments equal as sorted sets.  The call reads nothing of a map but its resolution and origin, so the list cases run on a small
dense map and on a hash-block map.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RES = 0.1
ORIGIN = (-2.0, -1.6, 0.3)
LIMIT = 2 ** 20 - 1
PER_PART = ("parent", "depth", "size", "root", "box_lo", "box_hi", "centroid", "mask_or", "key_min", "key_argmin")
TOTALS = ("n_parts", "n_members", "n_split_clusters", "n_oversize", "largest", "deepest", "status")
INFO = ("n_parts", "n_members", "n_split_clusters", "n_oversize", "largest", "depth", "status")
ERR_INVALID = 1


@pytest.fixture(scope="module")
def maps(hip_lib):
    import fiesta_amd
    made = {"dense": fiesta_amd.ESDFMap(ORIGIN, RES, (3.15, 3.15, 3.15)), "hash": fiesta_amd.ESDFMap(ORIGIN, RES, reserve_size=20000, mode="hash")}
    yield made
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def dense(maps):
    return maps["dense"]


def model(m, vox, off, mem, mask=None, key=None, **kw):
    from fiesta_amd import split_model
    return split_model(vox, off, mem, mask=mask, key=key, resolution=m.resolution, origin=m.origin, **kw)


def segments(r):
    off = r["offsets"]
    return [sorted(r["members"][off[p]:off[p + 1]].tolist()) for p in range(len(off) - 1)]


def assert_same(got, want, what=""):
    for k in TOTALS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("label", "offsets") + PER_PART:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float64:
            g, w = g.view(np.int64), w.view(np.int64)                              # the bits
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1)) if g.size else []
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} rows, first {bad[:3].tolist()}: got {got[k][bad[:3]].tolist()} " \
                              f"want {want[k][bad[:3]].tolist()}"
    assert len(got["members"]) == len(want["members"]) and segments(got) == segments(want), (what, "members")
    m0 = int(want["offsets"][0])
    assert np.array_equal(got["members"][:m0], want["members"][:m0]), (what, "members below offsets[0]")


def check(m, vox, off, mem, mask=None, key=None, what="", **kw):
    want = model(m, vox, off, mem, mask, key, **kw)
    got = m.SplitClusters(vox, off, mem, mask=mask, key=key, **kw)
    assert_same(got, want, what)
    return want


def sheet(n=72):
    """an n x n x 1 sheet as ONE cluster, its members in a shuffled order; 5 184 members at n = 72: more than one work-group's share
    (2 048) of the member scan"""
    rng = np.random.RandomState(72)
    v = np.ascontiguousarray((np.argwhere(np.ones((n, n, 1), bool)) + np.array([-30, 11, 5])).astype(np.int32))
    mask = (1 << rng.randint(0, 7, len(v))).astype(np.uint8)
    key = rng.randint(-2, 4000, len(v)).astype(np.int32)
    return v, np.array([0, len(v)], np.int64), rng.permutation(len(v)).astype(np.int64), mask, key


SHEET = sheet()


def three_clusters():
    """clusters of 1, 65 and 700 voxels out of a real cluster call over an entry list with duplicates, invalid entries and specks
    that min_size drops; then two members are listed twice"""
    rng = np.random.RandomState(5)
    one = np.array([[-50, -50, -50]])
    line = np.stack([np.arange(65), np.zeros(65, int), np.zeros(65, int)], 1) + (100, 7, -3)
    slab = np.argwhere(np.ones((35, 20, 1), bool)) + (-400, 300, 12)
    specks = np.array([[500, 500, 500], [600, 600, 600]])
    bad = np.array([[LIMIT, 0, 0], [0, -LIMIT - 5, 0]])
    v = np.concatenate([slab, one, bad, line, specks, slab[rng.randint(0, 700, 90)], line[:9]])
    v = np.ascontiguousarray(v[rng.permutation(len(v))].astype(np.int32))
    return v, rng.randint(0, 256, len(v)).astype(np.uint8), rng.randint(-3, 90, len(v)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "hash"])
@pytest.mark.parametrize("params", [dict(max_size=64), dict(max_extent=8), dict(max_size=40, max_extent=11), dict(max_size=64, max_depth=2)],
                         ids=["size", "extent", "both", "depth2"])
def test_the_sheet(maps, kind, params):
    v, off, mem, mask, key = SHEET
    want = check(maps[kind], v, off, mem, mask, key, what=f"sheet {params}", **params)
    assert want["n_split_clusters"] == 1
    if "max_depth" in params:
        assert want["n_parts"] == 4 and want["n_oversize"] == 4 and want["deepest"] == 2
    else:
        assert want["n_parts"] >= 81 and want["n_oversize"] == 0 and want["deepest"] >= 7


def two_sheets(n_members):
    """two clusters of unequal size -- a strip 7 voxels wide with a third of the members, a strip 13 wide with the rest, far apart --
    over a shuffled entry list, each segment's members in a shuffled order"""
    rng = np.random.RandomState(n_members)
    na = n_members // 3
    nb = n_members - na
    a = np.stack([np.arange(na) // 7, np.arange(na) % 7, np.zeros(na, int)], 1) + (-60, 4, 9)
    b = np.stack([np.arange(nb) % 13, np.full(nb, 2), np.arange(nb) // 13], 1) + (200, -30, -11)
    place = rng.permutation(n_members)                                     # entry index of voxel j of a ++ b
    v = np.empty((n_members, 3), np.int32)
    v[place] = np.concatenate([a, b])
    mem = np.concatenate([rng.permutation(place[:na]), rng.permutation(place[na:])]).astype(np.int64)
    mask, key = (1 << rng.randint(0, 7, n_members)).astype(np.uint8), rng.randint(-2, 900, n_members).astype(np.int32)
    return np.ascontiguousarray(v), np.array([0, na, n_members], np.int64), mem, mask, key


@pytest.mark.parametrize("kind", ["dense", "hash"])
@pytest.mark.parametrize("n_members", [2047, 2048, 2049, 4097])
def test_member_counts_around_the_scan_tile(maps, kind, n_members):
    """kSplitTile = 2048 members are one work-group's share of the member scan: one member short of a tile, a whole tile, one member
    into the second tile, one into the third.  The second cluster starts inside the first tile, so that tile holds a head flag in
    its middle and high-side flags of two parts; max_size makes the smaller cluster cut once and the larger at least twice"""
    v, off, mem, mask, key = two_sheets(n_members)
    want = check(maps[kind], v, off, mem, mask, key, what=f"{kind} {n_members} members", max_size=n_members // 5)
    assert want["n_split_clusters"] == 2 and want["deepest"] >= 2 and want["n_oversize"] == 0 and want["n_members"] == n_members
    assert 0 < off[1] < 2048 and sorted(set(want["parent"].tolist())) == [0, 1]


def test_three_clusters_with_duplicates_invalid_entries_and_dropped_specks(maps):
    v, mask, key = three_clusters()
    m = maps["dense"]
    cl = m.ClusterVoxels(v, mask=mask, key=key, connectivity=6, min_size=2)   # drops the specks (and the single voxel: listed by hand below)
    assert sorted(cl["size"].tolist()) == [65, 700] and cl["n_invalid"] == 2 and cl["n_duplicates"] == 99 and cl["n_dropped_clusters"] == 3
    single = int(np.flatnonzero((v == (-50, -50, -50)).all(1))[0])
    mem = np.concatenate([[single], cl["members"]]).astype(np.int64)
    off = np.concatenate([[0], 1 + cl["offsets"]]).astype(np.int64)
    assert np.diff(off).tolist()[0] == 1 and sorted(np.diff(off).tolist()) == [1, 65, 700]
    for kind in ("dense", "hash"):
        for params in (dict(max_size=7), dict(max_extent=3), dict(max_size=100, max_extent=30), dict(max_size=1)):
            want = check(maps[kind], v, off, mem, mask, key, what=f"three clusters {kind} {params}", **params)
            assert want["n_split_clusters"] == 2 and want["n_oversize"] == 0 and want["parent"][0] == 0 and want["size"][0] == 1
    # an empty segment, then a segment that lists one member twice: it counts twice, and entries listed by two parts take the later
    e, f = (int(i) for i in np.sort(mem[1:])[[3, 700]])                  # (the order inside the cluster call's segments is unspecified)
    mem2 = np.concatenate([mem, [e, f, e]]).astype(np.int64)
    off2 = np.concatenate([off, [off[-1], len(mem2)]]).astype(np.int64)
    for params in (dict(max_size=7), dict(max_size=1)):
        want = check(m, v, off2, mem2, mask, key, what=f"twice-listed {params}", **params)
        assert want["parent"].max() == 4 and 3 not in want["parent"]
        for i in (e, f):                                                   # listed by a part of its cluster and by one of segment 4
            lists = [p for p, seg in enumerate(segments(want)) if i in seg]
            assert len(lists) == 2 and want["label"][i] == lists[1] and want["parent"][lists[1]] == 4
        assert want["n_oversize"] == (params["max_size"] == 1)            # the two listings of e share a voxel: never cut


def test_a_diagonal_line(maps):
    """300 voxels along (1, 1, 1) scaled unevenly: deep, unbalanced recursion (the box halves, the members do not)"""
    t = (np.arange(300) * (np.arange(300) + 3) // 2)[:, None]
    v = np.ascontiguousarray((t * np.array([1, 1, 1]) + np.array([-20000, 5, 9])).astype(np.int32))
    off, mem = np.array([0, 300], np.int64), np.random.RandomState(3).permutation(300).astype(np.int64)
    for kind in ("dense", "hash"):
        want = check(maps[kind], v, off, mem, what="diagonal", max_size=2)
        assert want["deepest"] >= 10 and want["n_oversize"] == 0
        cut = check(maps[kind], v, off, mem, what="diagonal, depth 5", max_size=2, max_depth=5)
        assert cut["n_oversize"] >= 1 and cut["deepest"] == 5
    # max_depth 63 never cuts anything: coordinates across the whole valid range
    far = np.array([[-(LIMIT - 1), 0, 0], [LIMIT - 1, 0, 0], [LIMIT - 2, 0, 0], [0, LIMIT - 1, 1], [0, -(LIMIT - 1), 1], [1, 1, 1], [1, 1, 2]], np.int32)
    want = check(maps["dense"], far, np.array([0, 7], np.int64), np.arange(7, dtype=np.int64), what="far", max_size=1)
    assert want["n_parts"] == 7 and want["n_oversize"] == 0 and want["deepest"] <= 63


def test_the_identity_case_equals_the_cluster_call_bit_for_bit(maps):
    v, mask, key = three_clusters()
    for kind in ("dense", "hash"):
        m = maps[kind]
        cl = m.ClusterVoxels(v, mask=mask, key=key, connectivity=26, min_size=1)
        for depth in (0, 63):
            got = m.SplitClusters(v, cl["offsets"], cl["members"], mask=mask, key=key, max_depth=depth)
            assert got["n_parts"] == cl["n_clusters"] and got["n_members"] == cl["n_members"] and got["largest"] == cl["largest"]
            assert got["n_split_clusters"] == 0 and got["n_oversize"] == 0 and got["deepest"] == 0 and got["status"] == 0
            assert got["parent"].tolist() == list(range(cl["n_clusters"])) and not got["depth"].any()
            for k in PER_PART[2:] + ("offsets",):
                assert got[k].dtype == cl[k].dtype and got[k].tobytes() == cl[k].tobytes(), (kind, depth, k)
            assert segments(got) == segments(cl)
            listed = np.zeros(len(v), bool)
            listed[cl["members"]] = True
            assert np.array_equal(got["label"][listed], cl["label"][listed]) and (got["label"][~listed] == -1).all()


def raw_call(m, v, off, mem, cap, fields, mask=None, key=None, pad=3, **kw):
    """the host call with an explicit capacity and only `fields` of the result struct given; `pad` guard rows behind every array"""
    from fiesta_amd._lib import SplitInfo, SplitResult
    from fiesta_amd.esdf_map import SPLIT_FIELDS
    out = {name: np.full((cap + pad,) + shape, 123, dtype) for name, dtype, shape in SPLIT_FIELDS}
    out["offsets"], out["members"], out["label"] = np.full(cap + 1 + pad, 123, np.int64), np.full(len(mem) + pad, 123, np.int64), np.full(len(v) + pad, 123, np.int32)
    res = SplitResult(*[out[name].ctypes.data if name in fields else None for name, _ in SplitResult._fields_])
    info = SplitInfo()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    st = m._lib.fiesta_hip_split_clusters(m._h, p(v), p(mask), p(key), len(v), p(off), p(mem), len(off) - 1, len(mem), kw.get("max_size", 0),
                                          kw.get("max_extent", 0), kw.get("max_depth", 63), cap, C.byref(res), C.byref(info))
    out.update(zip(TOTALS, (int(getattr(info, k)) for k in INFO)))
    return st, out


def test_capacities_and_null_pointers(dense):
    v, off, mem, mask, key = SHEET
    want = model(dense, v, off, mem, mask, key, max_size=64)
    P = want["n_parts"]
    every = PER_PART + ("offsets", "members", "label")
    for cap in (0, 5, P):                                                  # part_capacity 0 sizes the buffers, then exact
        st, got = raw_call(dense, v, off, mem, cap, every, mask, key, max_size=64)
        assert st == 0
        for k in TOTALS:
            assert got[k] == want[k], (cap, k)
        for k in PER_PART:
            assert got[k][:cap].tobytes() == want[k][:cap].tobytes() and (got[k][cap:] == 123).all(), (cap, k)
        assert np.array_equal(got["offsets"][:cap + 1], want["offsets"][:cap + 1]) and (got["offsets"][cap + 1:] == 123).all()
        assert sorted(got["members"][:len(mem)].tolist()) == sorted(mem.tolist()) and (got["members"][len(mem):] == 123).all()
        assert np.array_equal(got["label"][:len(v)], want["label"]) and (got["label"][len(v):] == 123).all()
    for only in every:                                                     # every result pointer NULL but one, in turn
        st, got = raw_call(dense, v, off, mem, P, (only,), mask, key, max_size=64)
        assert st == 0 and got["n_parts"] == P
        for k in every:
            if k != only:
                assert (got[k] == 123).all(), (only, k)
        if only == "members":
            got["offsets"] = want["offsets"]
            assert segments(got)[:P] == segments(want)
        else:
            n = len(want[only])
            assert got[only][:n].tobytes() == want[only].tobytes(), only
    from fiesta_amd._lib import SplitInfo
    info = SplitInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert dense._lib.fiesta_hip_split_clusters(dense._h, p(v), None, None, len(v), p(off), p(mem), 1, len(mem), 64, 0, 63, 0, None, C.byref(info)) == 0
    assert info.n_parts == P and info.largest == want["largest"] and info.depth == want["deepest"]


def device_call(m, v, off, mem, n_clusters_dev=None, cap=None, mask=None, pad=4, **kw):
    """the _dev call on torch buffers with `pad` guard rows of 123 behind every output; returns the host copies"""
    import torch
    from fiesta_amd.esdf_map import SPLIT_FIELDS
    dev = torch.device("cuda", 0)
    cap = len(mem) if cap is None else cap
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    tv, toff, tmem = up(v), up(off), up(mem if len(mem) else np.zeros(1, np.int64))
    tmask = None if mask is None else up(mask)
    tk = None if n_clusters_dev is None else up(np.array([n_clusters_dev], np.int64))
    t = {name: torch.full((cap + pad,) + shape, 123, dtype=getattr(torch, np.dtype(dtype).name), device=dev) for name, dtype, shape in SPLIT_FIELDS}
    t["offsets"] = torch.full((cap + 1 + pad,), 123, dtype=torch.int64, device=dev)
    t["members"] = torch.full((len(mem) + pad,), 123, dtype=torch.int64, device=dev)
    t["label"] = torch.full((len(v) + pad,), 123, dtype=torch.int32, device=dev)
    info = torch.full((7 + pad,), 123, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()       # (the map's stream does not wait for torch's)
    m.SplitClustersDevice(tv.data_ptr(), len(v), toff.data_ptr(), tmem.data_ptr(), len(off) - 1, len(mem), info.data_ptr(),
                          mask_dev_ptr=0 if tmask is None else tmask.data_ptr(), n_clusters_dev_ptr=0 if tk is None else tk.data_ptr(),
                          part_capacity=cap, out={k: x.data_ptr() for k, x in t.items()}, **kw)
    m.synchronize()
    out = {k: x.cpu().numpy() for k, x in t.items()}
    out["info"] = info.cpu().numpy()
    return out


def test_data_errors_in_the_device_variant(dense):
    """status INVALID, n_parts 0, label filled with -1 and nothing else written: every output keeps its 123s, guard words included"""
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [LIMIT, 0, 0]], np.int32)
    good = (np.array([0, 2, 3], np.int64), np.array([0, 1, 2], np.int64))
    z = lambda a: np.array(a, np.int64)   # noqa: E731
    bad = [(z([-1, 2, 3]), good[1]), (z([0, 3, 2]), good[1]), (z([0, 2, 4]), good[1]), (good[0], z([0, 1, 4])), (good[0], z([0, -1, 2])),
           (good[0], z([0, 1, 3])), (z([2, 1, 3]), good[1])]
    for off, mem in bad:
        out = device_call(dense, v, off, mem, max_size=1)
        assert out["info"].tolist() == [0, 0, 0, 0, 0, 0, 1] + [123] * 4, (off, mem, out["info"])
        assert out["label"].tolist() == [-1] * 4 + [123] * 4
        for k in PER_PART + ("offsets", "members"):
            assert (out[k] == 123).all(), (off, mem, k)
        with pytest.raises(Exception):
            dense.SplitClusters(v, off, mem, max_size=1)                   # the host variant refuses the batch
    out = device_call(dense, v, *good, max_size=1)                         # the same buffers, no error
    assert out["info"].tolist() == [3, 3, 1, 0, 1, 1, 0] + [123] * 4 and out["label"].tolist() == [0, 1, 2, -1] + [123] * 4
    assert out["offsets"].tolist() == [0, 1, 2, 3] + [123] * 4 and out["members"].tolist() == [0, 1, 2] + [123] * 4
    # the device cluster count cuts the offsets: the broken tail is never read
    out = device_call(dense, v, z([0, 2, 1]), good[1], n_clusters_dev=1, max_size=1)
    assert out["info"][:7].tolist() == [2, 2, 1, 0, 1, 1, 0] and out["parent"][:2].tolist() == [0, 0] and (out["parent"][2:] == 123).all()
    out = device_call(dense, v, z([0, 2, 1]), good[1], n_clusters_dev=5, max_size=1)
    assert out["info"][:7].tolist() == [0, 0, 0, 0, 0, 0, 1]
    out = device_call(dense, v, *good, n_clusters_dev=0, max_size=1)
    assert out["info"][:7].tolist() == [0] * 7 and out["offsets"][:2].tolist() == [0, 123] and out["label"][:4].tolist() == [-1] * 4


def test_the_device_variant_equals_the_host_variant_on_both_stores(maps):
    v, off, mem, mask, key = SHEET
    want = model(maps["dense"], v, off, mem, mask, None, max_size=40, max_extent=11)
    P = want["n_parts"]
    for kind in ("dense", "hash"):
        for cap in (len(mem), P - 3):
            out = device_call(maps[kind], v, off, mem, cap=cap, mask=mask, max_size=40, max_extent=11)
            assert out["info"][:7].tolist() == [want[k] for k in TOTALS] and (out["info"][7:] == 123).all()
            k = min(P, cap)
            for name in PER_PART:
                assert out[name][:k].tobytes() == want[name][:k].tobytes() and (out[name][cap:] == 123).all(), (kind, cap, name)
            assert np.array_equal(out["offsets"][:k + 1], want["offsets"][:k + 1]) and (out["offsets"][cap + 1:] == 123).all()
            assert np.array_equal(out["label"][:len(v)], want["label"]) and (out["label"][len(v):] == 123).all()
            got = {"offsets": want["offsets"], "members": out["members"][:len(mem)]}
            assert segments(got) == segments(want) and (out["members"][len(mem):] == 123).all()


@pytest.fixture(scope="module")
def scene(hip_lib):
    from test_cpp_reach import example_scene
    m = example_scene()
    yield m
    m.close()


RING_SENSOR = dict(min_range=0.2, max_range=3.0, tan_h=float(np.tan(np.deg2rad(40.0))), tan_v=float(np.tan(np.deg2rad(30.0))), block_mask=3, min_visible=3)
VIEW_KEYS = ("view_class", "n_in_view", "n_visible", "cover_count", "first_view", "best_view", "best_count")
VIEW_TOTALS = ("n_usable", "n_pairs", "pairs_in_view", "pairs_visible")


def host_chain(m, vox, mask, ring, conn, min_size, split):
    """the host calls one by one on the list `vox`: clusters, parts, coverage"""
    cl = m.ClusterVoxels(vox, mask=mask, connectivity=conn, min_size=min_size)
    sp = m.SplitClusters(vox, cl["offsets"], cl["members"], mask=mask, **split)
    cov = m.ViewCoverage(vox, centroid=sp["centroid"], ring=ring, offsets=sp["offsets"], members=sp["members"], min_clearance=0.3, **RING_SENSOR)
    return cl, sp, cov


def test_the_all_device_chain_equals_the_host_calls(scene):
    """GetFrontierVoxelsDevice -> ClusterVoxelsDevice -> SplitClustersDevice -> ViewCoverageDevice with device counters only"""
    import torch
    from fiesta_amd import view_ring
    from fiesta_amd._lib import ClusterResult, SplitResult, ViewResult
    from fiesta_amd.esdf_map import CLUSTER_FIELDS, SPLIT_FIELDS
    m = scene
    dev = torch.device("cuda", 0)
    cap, ring, split = 32000, view_ring([0.8, 1.6], 6, [0.0]), dict(max_size=48, max_extent=9)
    M = len(ring)
    c = {"vox": torch.zeros((cap, 3), dtype=torch.int32, device=dev), "mask": torch.zeros(cap, dtype=torch.uint8, device=dev),
         "label": torch.zeros(cap, dtype=torch.int32, device=dev), "offsets": torch.zeros(cap + 1, dtype=torch.int64, device=dev),
         "members": torch.zeros(cap, dtype=torch.int64, device=dev), "head": torch.zeros(8, dtype=torch.int64, device=dev)}
    for name, dtype, shape in CLUSTER_FIELDS:
        c[name] = torch.zeros((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    s = {"label": torch.zeros(cap, dtype=torch.int32, device=dev), "offsets": torch.zeros(cap + 1, dtype=torch.int64, device=dev),
         "members": torch.zeros(cap, dtype=torch.int64, device=dev), "info": torch.zeros(7, dtype=torch.int64, device=dev)}
    for name, dtype, shape in SPLIT_FIELDS:
        s[name] = torch.zeros((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    vw = {"view_class": torch.zeros(cap * M, dtype=torch.uint8, device=dev), "n_in_view": torch.zeros(cap * M, dtype=torch.int32, device=dev),
          "n_visible": torch.zeros(cap * M, dtype=torch.int32, device=dev), "cover_count": torch.zeros(cap, dtype=torch.int32, device=dev),
          "first_view": torch.zeros(cap, dtype=torch.int32, device=dev), "best_view": torch.zeros(cap, dtype=torch.int64, device=dev),
          "best_count": torch.zeros(cap, dtype=torch.int32, device=dev), "info": torch.zeros(4, dtype=torch.int64, device=dev)}
    ring_dev = torch.from_numpy(ring).to(dev)
    torch.cuda.synchronize()
    head = c["head"].data_ptr()
    m.GetFrontierVoxelsDevice(None, None, 0.0, c["vox"].data_ptr(), c["mask"].data_ptr(), cap, head)
    m.ClusterVoxelsDevice(c["vox"].data_ptr(), cap, head + 8, mask_dev_ptr=c["mask"].data_ptr(), n_dev_ptr=head, connectivity=26, min_size=5,
                          cluster_capacity=cap, member_capacity=cap, out={k: c[k].data_ptr() for k, _ in ClusterResult._fields_})
    m.SplitClustersDevice(c["vox"].data_ptr(), cap, c["offsets"].data_ptr(), c["members"].data_ptr(), cap, cap, s["info"].data_ptr(),
                          mask_dev_ptr=c["mask"].data_ptr(), n_clusters_dev_ptr=head + 8, part_capacity=cap,
                          out={k: s[k].data_ptr() for k, _ in SplitResult._fields_}, **split)
    m.ViewCoverageDevice(c["vox"].data_ptr(), cap, vw["info"].data_ptr(), centroid_dev_ptr=s["centroid"].data_ptr(), ring_dev_ptr=ring_dev.data_ptr(),
                         n_ring=M, offsets_dev_ptr=s["offsets"].data_ptr(), members_dev_ptr=s["members"].data_ptr(), n_groups=cap,
                         n_groups_dev_ptr=s["info"].data_ptr(), n_members=cap, min_clearance=0.3,
                         out={k: vw[k].data_ptr() for k, _ in ViewResult._fields_}, **RING_SENSOR)
    m.synchronize()                                                        # the only wait
    n = int(c["head"][0].item())
    vox, mask = c["vox"][:n].cpu().numpy(), c["mask"][:n].cpu().numpy()
    assert 500 < n < cap
    cl, sp, cov = host_chain(m, vox, mask, ring, 26, 5, split)
    assert sp["n_parts"] > cl["n_clusters"] >= 2 and sp["n_split_clusters"] >= 1 and cov["pairs_visible"] > 0
    info = s["info"].cpu().numpy()
    got = {name: s[name][:sp["n_parts"]].cpu().numpy() for name in PER_PART}
    got.update(zip(TOTALS, info.tolist()))
    got["offsets"], got["members"], got["label"] = s["offsets"][:sp["n_parts"] + 1].cpu().numpy(), s["members"][:sp["n_members"]].cpu().numpy(), s["label"][:n].cpu().numpy()
    assert_same(got, sp, "device chain, parts")
    assert_same(sp, model(m, vox, cl["offsets"], cl["members"], mask, None, **split), "host call against the model")
    P = sp["n_parts"]
    for k, count in (("view_class", P * M), ("n_in_view", P * M), ("n_visible", P * M), ("cover_count", n), ("first_view", n), ("best_view", P), ("best_count", P)):
        assert np.array_equal(vw[k][:count].cpu().numpy(), cov[k]), k
    assert vw["info"].cpu().numpy().tolist() == [cov[k] for k in VIEW_TOTALS]
    # the convenience methods run that chain
    fc = m.FrontierClusters(connectivity=26, min_size=5, **split)
    order = np.lexsort((fc["vox"][:, 2], fc["vox"][:, 1], fc["vox"][:, 0]))
    assert np.array_equal(fc["vox"][order], vox[np.lexsort((vox[:, 2], vox[:, 1], vox[:, 0]))])
    cl2, sp2, _ = host_chain(m, fc["vox"], fc["mask"], ring, 26, 5, split)
    assert_same(fc, sp2, "FrontierClusters(max_size, max_extent)")
    assert fc["n_clusters"] == cl2["n_clusters"] and fc["n_invalid"] == 0 and fc["n_dropped_clusters"] == cl2["n_dropped_clusters"]
    for only in (dict(max_extent=9), dict(max_size=48, max_depth=1)):
        fv = m.FrontierViews(connectivity=26, min_size=5, ring=ring, view_clearance=0.3, **RING_SENSOR, **only)
        cl3, sp3, cov3 = host_chain(m, fv["vox"], fv["mask"], ring, 26, 5, only)
        assert_same(fv, sp3, f"FrontierViews({only})")
        assert fv["n_clusters"] == cl3["n_clusters"] and sp3["n_parts"] > cl3["n_clusters"]
        for k in VIEW_KEYS + VIEW_TOTALS:
            assert np.array_equal(fv[k], cov3[k]), (only, k)
        assert np.array_equal(fv["view_pos"], (sp3["centroid"][:, None, :] + ring[None, :, :3]).reshape(-1, 3))   # the rings stand around the parts


def test_with_the_defaults_both_methods_return_what_they_returned(scene):
    from fiesta_amd import view_ring
    from fiesta_amd.esdf_map import CLUSTER_FIELDS
    m = scene
    ring = view_ring([0.8, 1.6], 6, [0.0])
    a = m.FrontierClusters(connectivity=26, min_size=5)
    b = m.FrontierClusters(connectivity=26, min_size=5, max_size=0, max_extent=0, max_depth=7)
    cluster_keys = {name for name, _, _ in CLUSTER_FIELDS} | {"offsets", "members", "vox", "mask", "label", "n_clusters", "n_members", "n_invalid",
                                                              "n_duplicates", "n_dropped_clusters", "largest"}
    assert set(a) == set(b) == cluster_keys
    for r in (a, b):                                                       # (the frontier call's order is unspecified: each against its own list)
        host = m.ClusterVoxels(r["vox"], mask=r["mask"], connectivity=26, min_size=5)
        for k in cluster_keys - {"vox", "mask", "members"}:
            assert np.array_equal(r[k], host[k]), k
    va = m.FrontierViews(connectivity=26, min_size=5, ring=ring, view_clearance=0.3, **RING_SENSOR)
    vb = m.FrontierViews(connectivity=26, min_size=5, ring=ring, view_clearance=0.3, max_depth=3, **RING_SENSOR)
    view_keys = cluster_keys | set(VIEW_KEYS) | set(VIEW_TOTALS) | {"view_pos", "view_dir", "best_pos", "best_dir"}
    assert set(va) == set(vb) == view_keys
    for r in (va, vb):
        cov = m.ViewCoverage(r["vox"], centroid=r["centroid"], ring=ring, offsets=r["offsets"], members=r["members"], min_clearance=0.3, **RING_SENSOR)
        for k in VIEW_KEYS + VIEW_TOTALS:
            assert np.array_equal(r[k], cov[k]), k


def test_errors_leave_the_map_usable(dense):
    import fiesta_amd
    v, off, mem, mask, key = SHEET
    want = model(dense, v, off, mem, mask, key, max_extent=8)
    for bad in (dict(max_size=-1), dict(max_extent=-2), dict(max_depth=64), dict(max_depth=-1)):
        with pytest.raises(fiesta_amd.FiestaHipError):
            dense.SplitClusters(v, off, mem, **bad)
        st, out = raw_call(dense, v, off, mem, 8, PER_PART + ("offsets", "members", "label"), **bad)
        assert st == ERR_INVALID and all((out[k] == 123).all() for k in PER_PART + ("offsets", "members", "label")), bad
    with pytest.raises(fiesta_amd.FiestaHipError):
        dense.SplitClusters(v, off, np.array([len(v)], np.int64), max_size=1)
    with pytest.raises(fiesta_amd.FiestaHipError):
        dense.SplitClustersDevice(0, 5, 8, 8, 1, 1, 8)
    with pytest.raises(fiesta_amd.FiestaHipError):
        dense.SplitClustersDevice(8, 5, 8, 8, 1, 1, 0)
    assert_same(dense.SplitClusters(v, off, mem, mask=mask, key=key, max_extent=8), want, "after the errors")
