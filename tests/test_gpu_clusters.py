"""Voxel clusters on the GPU (fiesta_hip_cluster_voxels[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/cluster_kernels.hpp).

The expected result is always fiesta_amd.cluster_model (the header's definition in plain Python; tests/test_cluster_rule.py checks it
against a literal flood fill and scipy.ndimage.label).  Every comparison is exact: integers equal, centroids equal as f64 BITS,
member segments equal as sorted sets.  The call reads nothing of a map but its resolution and origin, so the list cases run on a
small dense map and on a hash-block map; the ragged scenes (a real frontier, a real ReachField for the keys) exist for both kinds.
"""
import ctypes as C

import numpy as np
import pytest

from scenarios import P_DEFAULT

pytestmark = pytest.mark.gpu
RES = 0.1
ORIGIN = (-2.0, -1.6, 0.3)
SHAPE = (40, 32, 36)
LIMIT = 2 ** 20 - 1
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
PER_CLUSTER = ("size", "root", "box_lo", "box_hi", "centroid", "mask_or", "key_min", "key_argmin")
TOTALS = ("n_clusters", "n_members", "n_invalid", "n_duplicates", "n_dropped_clusters", "largest")
ERR_INVALID = 1


def scene_boxes(shift=(0, 0, 0)):
    """observed-free boxes: a hall with a wall in it, a separate room, and seeded random crumbs that make small ragged groups"""
    s = np.asarray(shift, np.int32)
    rng = np.random.RandomState(77)
    crumbs = np.stack([rng.randint(22, 39, 260), rng.randint(14, 31, 260), rng.randint(14, 35, 260)], 1)
    boxes = [((2, 2, 2), (20, 18, 20)), ((24, 4, 4), (30, 10, 12)), ((34, 2, 30), (34, 2, 30)), ((35, 3, 31), (35, 3, 31))]
    boxes += [(tuple(c), tuple(c)) for c in crumbs.tolist()]
    wall = np.array([(10, y, z) for y in range(2, 15) for z in range(2, 21)], np.int32)
    return [(s + lo, s + hi) for lo, hi in boxes], s + wall, s + np.array([4, 4, 4], np.int32)


def fill(m, shift=(0, 0, 0)):
    boxes, wall, seed = scene_boxes(shift)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    for lo, hi in boxes:
        m.SetOccupancyBox(lo, hi, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    for _ in range(3):                                  # (an obstacle needs three hits to count as occupied)
        m.SetOccupancy(wall, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return seed


class Scene:
    """a map, its frontier list with masks, and keys from a real ReachField call on it; computed once, left unchanged"""

    def __init__(self, kind):
        import fiesta_amd
        self.kind = kind
        if kind == "dense":
            self.m = fiesta_amd.ESDFMap(ORIGIN, RES, tuple((s - 0.5) * RES for s in SHAPE))
            assert self.m.grid_size == SHAPE
            shift = (0, 0, 0)
        else:
            self.m = fiesta_amd.ESDFMap(ORIGIN, RES, reserve_size=100000, mode="hash")
            shift = (-41, -23, -37)                     # negative coordinates, nothing aligned with the 16 x 16 x 32 tiles
        seed = fill(self.m, shift)
        self.lo, self.hi = np.asarray(shift, np.int32) - 2, np.asarray(shift, np.int32) + np.array(SHAPE, np.int32) + 2
        self.vox, self.mask = self.m.GetFrontierVoxels()
        order = np.lexsort((self.vox[:, 2], self.vox[:, 1], self.vox[:, 0]))      # (the call's order is unspecified: fix one)
        self.vox, self.mask = np.ascontiguousarray(self.vox[order]), np.ascontiguousarray(self.mask[order])
        assert len(self.vox) > 1500
        # the flood's box ends at x = 32: the frontier voxels beyond it read -1, whole small clusters among them
        reach_hi = np.asarray(shift, np.int32) + np.array([32, SHAPE[1] + 2, SHAPE[2] + 2], np.int32)
        r = self.m.ReachField([seed], self.lo, reach_hi, targets=self.vox, min_clearance=0.15, connectivity=26, want_cost=False)
        self.key = r["target_cost"]
        assert (self.key == -1).any() and (self.key == I32_MAX).any() and ((self.key >= 0) & (self.key < I32_MAX)).any()
        self.memo = {}

    def want(self, conn, min_size):
        if (conn, min_size) not in self.memo:
            self.memo[(conn, min_size)] = model(self.m, self.vox, self.mask, self.key, conn, min_size)
        return self.memo[(conn, min_size)]


@pytest.fixture(scope="module")
def scenes(hip_lib):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Scene(kind)
        return made[kind]
    yield get
    for s in made.values():
        s.m.close()


@pytest.fixture(params=["dense", "hash"])
def anymap(request, scenes):
    return scenes(request.param).m


def model(m, vox, mask=None, key=None, conn=26, min_size=1):
    from fiesta_amd import cluster_model
    return cluster_model(vox, mask=mask, key=key, connectivity=conn, min_size=min_size, resolution=m.resolution, origin=m.origin)


def segments(r, k_max=None):
    off = r["offsets"]
    return [sorted(r["members"][off[k]:off[k + 1]].tolist()) for k in range(len(off) - 1 if k_max is None else k_max)]


def assert_same(got, want, what=""):
    for k in TOTALS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("label", "offsets") + PER_CLUSTER:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float64:
            g, w = g.view(np.int64), w.view(np.int64)                              # the bits
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1)) if g.size else []
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} rows, first {bad[:3].tolist()}: got {got[k][bad[:3]].tolist()} " \
                              f"want {want[k][bad[:3]].tolist()}"
    assert len(got["members"]) == len(want["members"]) and segments(got) == segments(want), (what, "members")


def check(m, vox, mask=None, key=None, conn=26, min_size=1, what=""):
    want = model(m, vox, mask, key, conn, min_size)
    got = m.ClusterVoxels(vox, mask=mask, key=key, connectivity=conn, min_size=min_size)
    assert_same(got, want, what)
    return want


def raw_call(m, vox, conn, min_size, ccap, mcap, mask=None, key=None, pad=3):
    """the host call with explicit capacities; every array has `pad` guard rows behind its capacity"""
    from fiesta_amd._lib import ClusterInfo, ClusterResult
    from fiesta_amd.esdf_map import CLUSTER_FIELDS
    v = np.ascontiguousarray(vox, np.int32).reshape(-1, 3)
    n = len(v)
    out = {name: np.full((ccap + pad,) + shape, 123, dtype) for name, dtype, shape in CLUSTER_FIELDS}
    out["label"] = np.full(n + pad, 123, np.int32)
    out["offsets"] = np.full(ccap + 1 + pad, 123, np.int64)
    out["members"] = np.full(mcap + pad, 123, np.int64)
    info = ClusterInfo()
    res = ClusterResult(*[out[name].ctypes.data for name, _ in ClusterResult._fields_])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    st = m._lib.fiesta_hip_cluster_voxels(m._h, p(v), p(mask), p(key), n, conn, min_size, ccap, mcap, C.byref(res), C.byref(info))
    out.update({k: int(getattr(info, k)) for k in TOTALS})
    return st, out


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "hash"])
def test_batch_sizes(scenes, kind):
    """n = 0, 1, 63, 64, 65, 257 entries of the ragged scene: the wave boundaries of the aggregated reduction"""
    s = scenes(kind)
    pick = np.arange(0, len(s.vox), 5)                   # (every fifth frontier voxel: many small groups, a few larger ones)
    for n in (0, 1, 63, 64, 65, 257):
        i = pick[:n]
        for conn in (6, 26):
            want = check(s.m, s.vox[i], s.mask[i], s.key[i], conn, 1, f"{kind} n={n} conn={conn}")
            assert want["n_clusters"] >= min(n, 1)
    want = check(s.m, s.vox[:257], s.mask[:257], s.key[:257], 26, 1, f"{kind} the first 257")
    assert want["largest"] > 64                          # one cluster across several waves


def rods(n, seed):
    """n entries: rods of 1 .. 3 voxels along x in a lattice of pitch (4, 2, 2) -- no two rods touch, not even across a corner --
    shuffled, and as the LAST entry a single voxel far from all of them: a root of its own at index n - 1"""
    rng = np.random.RandomState(seed)
    cells = np.argwhere(np.ones((24, 16, 16), bool)) * np.array([4, 2, 2]) - np.array([50, 17, 9])
    length = rng.randint(1, 4, len(cells))
    vox = np.repeat(cells, length, 0)
    vox[:, 0] += np.arange(len(vox)) - np.repeat(np.cumsum(length) - length, length)
    assert len(vox) >= n - 1
    vox = vox[:n - 1][rng.permutation(n - 1)]
    return np.ascontiguousarray(np.concatenate([vox, [[300, -200, 100]]]).astype(np.int32))


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_numbering_scan_trips(anymap, n):
    """k_cluster_number takes kClusterScanBlock * kClusterScanItems = 4096 entries per trip: one entry short of a trip, a whole
    trip, one entry into the second trip, one into the third.  Thousands of small clusters whose roots lie all over the list, so the
    ids and member offsets of the later trips are the carry plus a prefix; the last entry is a root alone in its trip at 4097 and
    8193.  min_size 2 drops the single voxels: the same scan then numbers fewer roots and counts the dropped ones"""
    vox = rods(n, n)
    rng = np.random.RandomState(n + 1)
    mask, key = rng.randint(0, 64, n).astype(np.uint8), rng.randint(-2, 500, n).astype(np.int32)
    want = check(anymap, vox, mask, key, 26, 1, f"rods n={n}")
    assert want["n_clusters"] > n // 3 and want["largest"] == 3 and want["root"][-1] == n - 1 and want["size"][-1] == 1
    assert (np.diff(want["root"]) > 0).all() and want["offsets"][-1] == n
    kept = check(anymap, vox, mask, key, 6, 2, f"rods n={n}, min_size 2")
    assert 0 < kept["n_clusters"] < want["n_clusters"] and kept["n_dropped_clusters"] == want["n_clusters"] - kept["n_clusters"]
    assert kept["label"][-1] == -1


def snake(nx=28, ny=28, nz=8):
    """a 6-connected serpentine one voxel wide, in path order: rows along x at every second y, joined at alternating ends by one
    voxel; layers at every second z joined the same way.  Rows and layers are two apart, so no two voxels that are not neighbours
    along the path touch -- not even across a corner, save at the turns themselves"""
    path, x_up, y_up = [], True, True
    for z in range(0, nz, 2):
        ys = list(range(0, ny, 2)) if y_up else list(range(0, ny, 2))[::-1]
        for j, y in enumerate(ys):
            xs = range(nx) if x_up else range(nx - 1, -1, -1)
            path += [(x, y, z) for x in xs]
            x_end = nx - 1 if x_up else 0
            x_up = not x_up
            if j + 1 < len(ys):
                path.append((x_end, (y + ys[j + 1]) // 2, z))
        if z + 2 < nz:
            path.append((x_end, ys[-1], z + 1))
        y_up = not y_up
    return np.array(path, np.int32)


def test_snake(anymap):
    m = anymap
    path = snake() + np.array([-9, 3, -2], np.int32)
    assert len(path) >= 1500 and len({tuple(p) for p in path.tolist()}) == len(path)
    step = np.abs(np.diff(path.astype(np.int64), axis=0))
    assert (step.sum(1) == 1).all()                      # 6-connected along the path
    orders = {"path": np.arange(len(path)), "reversed": np.arange(len(path))[::-1],
              "sorted": np.lexsort((path[:, 2], path[:, 1], path[:, 0]))}
    for seed in (1, 2, 3):
        orders[f"shuffle {seed}"] = np.random.RandomState(seed).permutation(len(path))
    first = None
    for name, order in orders.items():
        vox = np.ascontiguousarray(path[order])
        for conn in (6, 26):
            want = model(m, vox, conn=conn)
            assert want["n_clusters"] == 1 and want["size"][0] == len(path), (name, conn)     # the fixture itself, on the model
            got = m.ClusterVoxels(vox, connectivity=conn)
            assert_same(got, want, f"snake {name} {conn}")
            first = want if first is None else first
            assert got["centroid"].view(np.int64).tolist() == first["centroid"].view(np.int64).tolist()


def test_diagonal_contacts(anymap):
    m = anymap
    blob = np.argwhere(np.ones((3, 3, 3), bool)).astype(np.int32)
    # A and B touch only across an edge (x and y differ), C and D only across a corner
    vox = np.concatenate([blob, blob + (3, 3, 0), blob + (20, 0, 0), blob + (23, 3, 3)])
    vox = np.ascontiguousarray(vox[np.random.RandomState(4).permutation(len(vox))] - np.array([11, 2, 1], np.int32))
    for conn, k in ((6, 4), (18, 3), (26, 2)):
        want = check(m, vox, conn=conn, what=f"contacts {conn}")
        assert want["n_clusters"] == k


def test_checkerboard_and_short_capacities(anymap):
    m = anymap
    g = np.argwhere(np.indices((16, 16, 16)).sum(0) % 2 == 0).astype(np.int32) - 5
    assert len(g) == 2048
    for conn, k in ((6, 2048), (18, 1), (26, 1)):
        want = check(m, g, conn=conn, what=f"checkerboard {conn}")
        assert want["n_clusters"] == k
    want = model(m, g, conn=6)
    for ccap, mcap in ((100, 2048), (65, 37), (0, 0), (1, 0)):
        st, got = raw_call(m, g, 6, 1, ccap, mcap)
        assert st == 0
        for k in TOTALS:
            assert got[k] == want[k], (ccap, mcap, k)
        assert np.array_equal(got["label"][:2048], want["label"]) and (got["label"][2048:] == 123).all()
        for k in PER_CLUSTER:
            assert np.array_equal(got[k][:ccap].view(np.uint8), want[k][:ccap].view(np.uint8)), (ccap, k)
            assert (got[k][ccap:] == 123).all(), (ccap, k, "written beyond the capacity")
        assert np.array_equal(got["offsets"][:ccap + 1], want["offsets"][:ccap + 1]) and (got["offsets"][ccap + 1:] == 123).all()
        assert np.array_equal(got["members"][:mcap], want["members"][:mcap])       # (clusters of one voxel: the order is fixed)
        assert (got["members"][mcap:] == 123).all()
    # one cluster, a short member capacity: a subset of the right size
    st, got = raw_call(m, g, 26, 1, 4, 700)
    assert st == 0 and got["n_clusters"] == 1 and got["n_members"] == 2048 and got["offsets"][:2].tolist() == [0, 2048]
    assert len(set(got["members"][:700].tolist())) == 700 and (got["members"][700:] == 123).all()


def test_one_big_blob(anymap):
    m = anymap
    blob = np.argwhere(np.ones((16, 16, 16), bool)).astype(np.int32) + np.array([-8, 100, -300], np.int32)
    rng = np.random.RandomState(8)
    mask = (1 << rng.randint(0, 6, len(blob))).astype(np.uint8)
    key = rng.randint(-1, 50, len(blob)).astype(np.int32)
    for conn in (6, 18, 26):
        want = check(m, blob, mask, key, conn, what=f"blob {conn}")
        assert want["n_clusters"] == 1 and want["size"][0] == 4096 and want["mask_or"][0] == 63 and want["key_min"][0] == 0


def test_more_clusters_than_the_wrapper_guesses(scenes):
    """ESDFMap.ClusterVoxels sizes the per-cluster arrays for 65 536 clusters and calls again with the total when there are more"""
    m = scenes("dense").m
    vox = np.ascontiguousarray((np.argwhere(np.ones((41, 40, 40), bool)) * 2 - 40).astype(np.int32))      # no two adjacent
    want = check(m, vox, conn=6, what="65 600 single voxels")
    assert want["n_clusters"] == len(vox) == 65600 > 1 << 16 and want["largest"] == 1


def test_lattice_coordinates(anymap):
    m = anymap
    a = np.argwhere(np.ones((8, 8, 8), bool)).astype(np.int32) - 4
    lattice = a * 1024                                   # low ten bits all zero
    pairs = np.concatenate([lattice[:100], lattice[:100] + (1 << 10), lattice[:100] + (1 << 19) - 7, a, a + (1 << 18)])
    for vox, name in ((lattice, "lattice"), (pairs, "high-bit pairs")):
        vox = np.ascontiguousarray(vox[np.random.RandomState(5).permutation(len(vox))])
        for conn in (6, 26):
            check(m, vox, conn=conn, what=f"{name} {conn}")
    assert model(m, lattice)["n_clusters"] == 512


def test_duplicates_and_invalid_entries(anymap):
    m = anymap
    rng = np.random.RandomState(21)
    base = rng.randint(-6, 7, (300, 3)).astype(np.int32) + np.array([-3, 0, 5], np.int32)
    bad = np.array([(LIMIT, 0, 0), (0, -LIMIT, 0), (0, 0, LIMIT), (I32_MIN, 1, 1), (1, I32_MIN, 1), (I32_MAX, I32_MAX, I32_MAX),
                    (-LIMIT, -LIMIT, -LIMIT)], np.int32)
    edge = np.array([(LIMIT - 1, 0, 0), (LIMIT - 1, 1, 0), (-(LIMIT - 1), -(LIMIT - 1), -(LIMIT - 1)), (-(LIMIT - 2), -(LIMIT - 1), -(LIMIT - 1))],
                    np.int32)                            # the outermost valid voxels: their neighbours beyond are never in the table
    vox = np.concatenate([base, bad, base[rng.randint(0, 300, 120)], edge])
    vox = vox[rng.permutation(len(vox))]
    vox = np.ascontiguousarray(np.concatenate([vox[40:41], vox, vox[:1]]))           # the first entry has a duplicate later on
    mask = rng.randint(0, 64, len(vox)).astype(np.uint8)
    key = rng.randint(-2, 9, len(vox)).astype(np.int32)
    for conn in (6, 18, 26):
        for min_size in (1, 3):
            want = check(m, vox, mask, key, conn, min_size, f"duplicates {conn} {min_size}")
            assert want["n_invalid"] == 7 and want["n_duplicates"] > 100
    assert model(m, edge, conn=6)["n_clusters"] == 2


@pytest.mark.parametrize("kind", ["dense", "hash"])
def test_min_size_mask_and_key_on_the_ragged_scene(scenes, kind):
    s = scenes(kind)
    n = len(s.vox)
    for conn in (6, 18, 26):
        for min_size in (1, 2, 10, n + 1):
            want = s.want(conn, min_size)
            got = s.m.ClusterVoxels(s.vox, mask=s.mask, key=s.key, connectivity=conn, min_size=min_size)
            assert_same(got, want, f"{kind} scene {conn} {min_size}")
        one, ten = s.want(conn, 1), s.want(conn, 10)
        assert one["n_clusters"] > ten["n_clusters"] > 1 and ten["n_dropped_clusters"] > 0 and s.want(conn, n + 1)["n_clusters"] == 0
        assert (one["key_min"] == I32_MAX).any() and (one["key_min"] < I32_MAX).any() and (one["mask_or"] > 0).all()
        assert (one["key_argmin"] == -1).any()           # a cluster whose every key is -1


def test_permutation_invariance(scenes):
    s = scenes("dense")
    perm = np.random.RandomState(12).permutation(len(s.vox))
    a = s.m.ClusterVoxels(s.vox, mask=s.mask, key=s.key, connectivity=18, min_size=2)
    b = s.m.ClusterVoxels(s.vox[perm], mask=s.mask[perm], key=s.key[perm], connectivity=18, min_size=2)
    assert a["n_clusters"] == b["n_clusters"] > 3
    # the same partition: entries i and perm-position of i carry labels that correspond one to one
    pairs = set(zip(a["label"][perm].tolist(), b["label"].tolist()))
    assert len(pairs) == a["n_clusters"] + (1 if (a["label"] == -1).any() else 0)

    def rows(r):
        return sorted(zip(r["size"].tolist(), map(tuple, r["box_lo"].tolist()), map(tuple, r["box_hi"].tolist()),
                          map(tuple, r["centroid"].view(np.int64).tolist()), r["mask_or"].tolist(), r["key_min"].tolist()))
    assert rows(a) == rows(b)


def device_chain(m, lo, hi, conn, min_size, capacity):
    import torch
    from fiesta_amd.esdf_map import CLUSTER_FIELDS
    dev = torch.device("cuda", 0)
    t = {"vox": torch.full((capacity, 3), -7, dtype=torch.int32, device=dev), "mask": torch.zeros(capacity, dtype=torch.uint8, device=dev),
         "label": torch.full((capacity,), -7, dtype=torch.int32, device=dev), "offsets": torch.zeros(capacity + 1, dtype=torch.int64, device=dev),
         "members": torch.zeros(capacity, dtype=torch.int64, device=dev), "head": torch.full((8,), 99, dtype=torch.int64, device=dev)}
    for name, dtype, shape in CLUSTER_FIELDS:
        t[name] = torch.zeros((capacity,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    torch.cuda.synchronize()       # (the map's stream does not wait for torch's: the fills above must have landed)
    head = t["head"].data_ptr()
    m.GetFrontierVoxelsDevice(lo, hi, 0.0, t["vox"].data_ptr(), t["mask"].data_ptr(), capacity, head)
    outs = {k: t[k].data_ptr() for k in ("label", "offsets", "members") + PER_CLUSTER}
    m.ClusterVoxelsDevice(t["vox"].data_ptr(), capacity, head + 8, mask_dev_ptr=t["mask"].data_ptr(), n_dev_ptr=head, connectivity=conn,
                          min_size=min_size, cluster_capacity=capacity, member_capacity=capacity, out=outs)
    m.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


@pytest.mark.parametrize("kind", ["dense", "hash"])
def test_device_chain(scenes, kind):
    s = scenes(kind)
    n = len(s.vox)
    cap = n + 100
    for conn, min_size in ((26, 1), (6, 3)):
        t = device_chain(s.m, None, None, conn, min_size, cap)
        assert t["head"][0] == n and t["head"][7] == 99
        vox, mask = t["vox"][:n], t["mask"][:n]
        assert sorted(map(tuple, vox.tolist())) == sorted(map(tuple, s.vox.tolist())) and (t["vox"][n:] == -7).all()
        want = model(s.m, vox, mask, None, conn, min_size)                          # the list as the device buffer holds it
        k = want["n_clusters"]
        got = {name: t[name][:k] for name in PER_CLUSTER}
        got.update({name: int(t["head"][1 + i]) for i, name in enumerate(TOTALS)})
        got["label"], got["offsets"], got["members"] = t["label"][:n], t["offsets"][:k + 1], t["members"][:want["n_members"]]
        assert_same(got, want, f"{kind} device chain {conn} {min_size}")
        assert (t["label"][n:] == -7).all(), "label beyond the device count is left untouched"


@pytest.mark.parametrize("kind", ["dense", "hash"])
def test_frontier_clusters_convenience(scenes, kind):
    s = scenes(kind)
    for _ in range(2):                                   # (the second call finds its buffers in place)
        got = s.m.FrontierClusters(connectivity=26, min_size=2)
        assert sorted(map(tuple, got["vox"].tolist())) == sorted(map(tuple, s.vox.tolist()))
        host = s.m.ClusterVoxels(got["vox"], mask=got["mask"], connectivity=26, min_size=2)
        assert_same(got, host, f"{kind} FrontierClusters against the host route")
        assert_same(got, model(s.m, got["vox"], got["mask"], None, 26, 2), f"{kind} FrontierClusters against the model")
    lo, hi = s.lo + 2, s.lo + 2 + np.array([21, 19, 21], np.int32)
    got = s.m.FrontierClusters(lo, hi, connectivity=6, min_size=1)
    bv, bm = s.m.GetFrontierVoxels(lo, hi)
    assert 0 < len(bv) == len(got["vox"]) < len(s.vox)
    assert_same(got, model(s.m, got["vox"], got["mask"], None, 6, 1), f"{kind} FrontierClusters, boxed")


def test_errors_leave_the_map_usable(scenes):
    import fiesta_amd
    s = scenes("dense")
    m, vox = s.m, s.vox[:300]
    want = model(m, vox, conn=26)
    for conn, min_size, ccap, mcap in ((8, 1, 4, 4), (0, 1, 4, 4), (26, 0, 4, 4), (26, -3, 4, 4), (26, 1, -1, 4), (26, 1, 4, -1)):
        st, out = raw_call(m, vox, conn, min_size, max(ccap, 0), max(mcap, 0)) if ccap >= 0 and mcap >= 0 else (None, None)
        if st is None:                                   # a negative capacity: the arrays are sized for 4, the call gets the bad value
            from fiesta_amd._lib import ClusterInfo
            info = ClusterInfo()
            st = m._lib.fiesta_hip_cluster_voxels(m._h, vox.ctypes.data_as(C.c_void_p), None, None, len(vox), conn, min_size, ccap, mcap, None,
                                                  C.byref(info))
        else:
            assert (out["label"] == 123).all(), "nothing is written"
        assert st == ERR_INVALID, (conn, min_size, ccap, mcap)
        assert_same(m.ClusterVoxels(vox), want, "after an error")
    from fiesta_amd._lib import ClusterInfo
    info = ClusterInfo()
    p = vox.ctypes.data_as(C.c_void_p)
    f = m._lib.fiesta_hip_cluster_voxels
    assert f(m._h, p, None, None, -1, 26, 1, 0, 0, None, C.byref(info)) == ERR_INVALID
    assert f(m._h, p, None, None, 2 ** 24 + 1, 26, 1, 0, 0, None, C.byref(info)) == ERR_INVALID
    assert f(m._h, None, None, None, 5, 26, 1, 0, 0, None, C.byref(info)) == ERR_INVALID
    assert f(m._h, p, None, None, 5, 26, 1, 0, 0, None, None) == ERR_INVALID
    assert_same(m.ClusterVoxels(vox), want, "after the errors")
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.ClusterVoxels(vox, connectivity=7)
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.ClusterVoxelsDevice(0, 5, 8)
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.ClusterVoxelsDevice(8, 5, 0)
    # a sizing call: capacities 0, null result
    assert f(m._h, p, None, None, len(vox), 26, 1, 0, 0, None, C.byref(info)) == 0
    assert info.n_clusters == want["n_clusters"] and info.n_members == want["n_members"] and info.largest == want["largest"]
    assert_same(m.ClusterVoxels(vox), want, "after the sizing call")


def test_shard(hip_lib, scenes):
    import fiesta_amd
    from fiesta_amd.sharded import ShardedESDFMap
    s = scenes("dense")
    sh = fiesta_amd.ESDFMap(ORIGIN, RES, (15.5 * RES,) * 3, shard_lo=(16, 0, 0), global_grid=(32, 16, 16))
    want = model(sh, s.vox, s.mask, s.key, 26, 2)
    assert_same(sh.ClusterVoxels(s.vox, mask=s.mask, key=s.key, min_size=2), want, "shard")
    assert_same(want, s.want(26, 2), "a shard shares the map's resolution and origin")
    sh.close()
    group = ShardedESDFMap(ORIGIN, RES, (32, 16, 16), 2)
    assert_same(group.ClusterVoxels(s.vox, mask=s.mask, key=s.key, min_size=2), want, "sharded class")
    assert_same(group.ClusterVoxels(s.vox, mask=s.mask, key=s.key, min_size=2, rank=1), want, "sharded class, rank 1")
    group.close()
