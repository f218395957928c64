"""Skeleton extraction on the GPU (fiesta_hip_get_skeleton_voxels[_dev], include/fiesta_hip.h; kernels:
fiesta_amd/csrc/skeleton_kernels.hpp).

The expected set is always fiesta_amd.skeleton_model (the header's definition in numpy; tests/test_skeleton_rule.py checks it against
a plain loop) fed from what the map itself reports through the calls that existed before: download_field (d2, coc, occ) or
download_hash, and GetDistance of every voxel -- never from the call under test.  Everything is integer: results are compared as
sorted (x, y, z, mask, d2, sep2) rows, tolerance zero, nothing excluded.  Every case asserts that the model's set is not empty.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import planner_probe as pp
from planner_probe import HASH_SHIFT
from scenarios import all_voxels
from test_gpu_frontiers import make_dense, ragged_scene

pytestmark = pytest.mark.gpu
NAMES = ("vox", "mask", "d2", "sep2")
DTYPES = {"vox": np.int32, "mask": np.uint8, "d2": np.int32, "sep2": np.int32}
ERR_INVALID = 1


def rows(r):
    a = np.concatenate([np.asarray(r["vox"], np.int64).reshape(-1, 3)] + [np.asarray(r[k], np.int64).reshape(-1, 1) for k in NAMES[1:]], 1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def assert_same(got, want, what=""):
    g, w = rows(got), rows(want)
    assert g.shape == w.shape, f"{what}: {len(g)} skeleton voxels, the model has {len(w)}"
    bad = np.nonzero((g != w).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first got {g[bad[:3]].tolist()} want {w[bad[:3]].tolist()}"


class DenseModel:
    """skeleton_model on the map's own dump, read once"""

    def __init__(self, m):
        f = m.download_field(("d2", "coc", "occ"))
        s = tuple(m.grid_size)
        self.d2, self.coc, self.occ = f["d2"].reshape(s), f["coc"].reshape(s + (3,)), f["occ"].reshape(s) != 0
        self.dist = m.GetDistance(all_voxels(s)).reshape(s)

    def __call__(self, min_sep2=9, lo=None, hi=None, min_clearance=0.0):
        from fiesta_amd import skeleton_model
        return skeleton_model(self.d2, self.coc, self.occ, min_sep2, self.dist, lo, hi, min_clearance)


class HashModel:
    """skeleton_model on download_hash scattered into an array padded by one voxel, in which absent voxels have no site"""

    def __init__(self, m):
        h = m.download_hash()
        self.org = h["vox"].min(0).astype(np.int64) - 1
        shape = tuple(int(v) for v in (h["vox"].max(0) - self.org + 2))
        i = tuple((h["vox"] - self.org).T)
        self.d2, self.coc = np.full(shape, -1, np.int64), np.zeros(shape + (3,), np.int64)
        self.occ, self.dist = np.zeros(shape, bool), np.full(shape, 10000.0)
        self.d2[i], self.coc[i], self.occ[i] = h["d2"], h["coc"], h["occ"] != 0
        self.dist[i] = m.GetDistance(h["vox"])

    def __call__(self, min_sep2=9, lo=None, hi=None, min_clearance=0.0):
        from fiesta_amd import skeleton_model
        return skeleton_model(self.d2, self.coc, self.occ, min_sep2, self.dist, lo, hi, min_clearance, origin_vox=self.org)


def raw_call(m, lo, hi, min_sep2, clearance, capacity, arrays, n_out=True, result=True):
    """the C call itself on the arrays named in `arrays` (the others NULL); returns (status, n_out)"""
    from fiesta_amd._lib import SkeletonResult
    from fiesta_amd.esdf_map import _p
    n = C.c_int64(-1)
    blo = None if lo is None else np.ascontiguousarray(lo, np.int32)
    bhi = None if hi is None else np.ascontiguousarray(hi, np.int32)
    res = SkeletonResult(*[arrays[k].ctypes.data if arrays.get(k) is not None else None for k in NAMES])
    st = m._lib.fiesta_hip_get_skeleton_voxels(m._h, _p(blo), _p(bhi), int(min_sep2), float(clearance), int(capacity),
                                               C.byref(res) if result else None, C.byref(n) if n_out else None)
    return st, n.value


def fresh_arrays(n, names=NAMES):
    return {k: np.full((n, 3) if k == "vox" else n, 0x5B, DTYPES[k]) for k in names}


# ---- 1. dense, ragged z -----------------------------------------------------------------------------------------------------------
RAGGED = [(nz, "box") for nz in (7, 32, 33, 40, 64, 65)] + [(nz, "faces") for nz in (7, 33, 65)] + \
         [(nz, v) for nz in (33, 40) for v in ("carry_low", "carry_high")]


@pytest.mark.parametrize("nz,variant", RAGGED)
def test_dense_ragged_z(hip_lib, nz, variant):
    obs, occupied = ragged_scene(nz, variant)
    m = make_dense(obs.shape, obs, occupied)
    model = DenseModel(m)
    assert model.occ.sum() == len(occupied)
    sizes = {}
    for min_sep2, c in itertools.product((9, 25), (0.0, 0.25)):
        want = model(min_sep2, min_clearance=c)
        sizes[(min_sep2, c)] = len(want["mask"])
        print(f"nz {nz} {variant}: min_sep2 {min_sep2} clearance {c}: {len(want['mask'])} skeleton voxels")
        assert_same(m.GetSkeletonVoxels(min_sep2=min_sep2, min_clearance=c), want, f"nz {nz} {variant} min_sep2 {min_sep2} clearance {c}")
    assert sizes[(9, 0.0)] > 0 and sizes[(9, 0.0)] >= sizes[(25, 0.0)] and sizes[(9, 0.0)] >= sizes[(9, 0.25)], sizes
    want = model(9)
    assert not {tuple(v) for v in want["vox"].tolist()} & set(occupied)
    total = len(want["mask"])
    w = rows(want)
    for k in range(len(NAMES) + 1):            # each subset of the output pointers NULL
        for names in itertools.combinations(NAMES, k):
            a = fresh_arrays(total + 3, names)
            st, n = raw_call(m, None, None, 9, 0.0, total, a)
            assert st == 0 and n == total, (names, st, n)
            for name in names:
                col = {"vox": slice(0, 3), "mask": 3, "d2": 4, "sep2": 5}[name]
                got = np.asarray(a[name][:total], np.int64).reshape(total, -1)
                assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, w[:, col].reshape(total, -1).tolist())), (names, name)
                assert (a[name][total:] == 0x5B).all(), f"{names}: {name} written past the total"
            if "vox" in names:                 # entry k of every array describes the same voxel
                order = np.lexsort(a["vox"][:total].T[::-1])
                for name in names:
                    assert np.array_equal(a[name][:total][order], want[name]), (names, name)
    m.close()


# ---- 2. the walls' known answer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", [(1, 9), (3, 7), (0, 10)])
def test_two_walls_plane(hip_lib, walls):
    shape = (12, 10, 40)
    V = all_voxels(shape)
    m = make_dense(shape, np.ones(shape, bool), V[(V[:, 0] == walls[0]) | (V[:, 0] == walls[1])])
    model = DenseModel(m)
    for min_sep2 in (2, 9, 16):
        want = model(min_sep2)
        assert len(want["mask"]) == 400 and (want["vox"][:, 0] == 5).all(), "the model: exactly the plane x = 5"
        got = m.GetSkeletonVoxels(min_sep2=min_sep2)
        assert got["n"] == 400 and (got["vox"][:, 0] == 5).all()
        assert_same(got, want, f"walls {walls} min_sep2 {min_sep2}")
        assert (got["d2"] == (5 - walls[0]) ** 2).all() and (got["sep2"] >= (walls[1] - walls[0]) ** 2).all()
    m.close()


# ---- 3. boxes ---------------------------------------------------------------------------------------------------------------------
def two_blob_scene(shape=(12, 10, 40)):
    """fully observed; obstacles spread over z so that the skeleton crosses the bitmap word boundary z = 31 | 32"""
    rng = np.random.RandomState(11)
    V = all_voxels(shape)
    return make_dense(shape, np.ones(shape, bool), V[rng.choice(len(V), 14, replace=False)])


@pytest.fixture(scope="module")
def boxed(hip_lib):
    m = two_blob_scene()
    yield m, DenseModel(m)
    m.close()


def test_box_semantics(boxed):
    m, model = boxed
    nx, ny, nz = m.grid_size
    whole = model()
    assert len(whole["mask"]) > 100
    assert_same(m.GetSkeletonVoxels((-5, -5, -5), (100, 100, 100)), whole, "a box around everything")
    assert_same(m.GetSkeletonVoxels((0, 0, 0), (nx - 1, ny - 1, nz - 1)), whole, "the array's own box")
    one = tuple(int(v) for v in whole["vox"][len(whole["vox"]) // 2])
    on = {tuple(r) for r in whole["vox"].tolist()}
    off = next(tuple(int(c) for c in v) for v in all_voxels((nx, ny, nz)) if tuple(v) not in on)
    boxes = [((-3, -3, -3), (5, 5, 20)),            # partly outside the map
             ((4, 2, 30), (9, 8, 33)),              # across the word boundary z = 31 | 32
             ((4, 2, 33), (9, 8, 38)), ((2, 2, 5), (9, 8, 5)),     # inside one word; one z-plane
             ((0, 0, 7), (nx - 1, ny - 1, 29)), ((0, 0, 13), (nx - 1, ny - 1, 37)),   # z bounds that are no multiples of 32
             (one, one), (off, off),                # single voxels: on the skeleton, off it
             ((nx - 1, ny - 1, nz - 1), (nx + 7, ny + 7, nz + 7)),
             ((100, 100, 100), (200, 200, 200)), ((-9, -9, -9), (-1, 50, 50)), ((0, 0, nz), (nx, ny, nz + 5)),   # wholly outside
             ((5, 5, 5), (4, 9, 9)), ((5, 5, 5), (9, 4, 9)), ((5, 5, 5), (9, 9, 4)),                            # lo > hi
             ((-2**31, -2**31, -2**31), (2**31 - 1, 2**31 - 1, 2**31 - 1))]
    counts = []
    for lo, hi in boxes:
        want = model(9, lo, hi)
        got = m.GetSkeletonVoxels(lo, hi, 9)
        assert got["n"] == len(want["mask"])
        assert_same(got, want, f"box {lo} {hi}")
        assert_same(m.GetSkeletonVoxels(lo, hi, 9, 0.25), model(9, lo, hi, 0.25), f"box {lo} {hi} clearance 0.25")
        counts.append(len(want["mask"]))
    print("box counts", counts)
    assert min(counts[:6]) > 0 and counts[6] == 1 and counts[7] == 0
    assert counts[9:15] == [0] * 6 and counts[15] == len(whole["mask"])
    # the box does not clip the neighbour test: a one-plane box keeps the bits that point out of it
    plane = rows(model(9, (0, 0, 20), (nx - 1, ny - 1, 20)))
    assert (plane[:, 3] & 0b110000).any()


# ---- 4. capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity(boxed):
    m, model = boxed
    want = rows(model())
    total = len(want)
    member = {tuple(r[:3]): tuple(r[3:]) for r in want.tolist()}
    for cap in (0, 1, total - 1, total, total + 5):
        a = fresh_arrays(cap + 8)
        st, n = raw_call(m, None, None, 9, 0.0, cap, a)
        assert st == 0 and n == total, (cap, st, n)
        k = min(total, cap)
        got = rows({x: a[x][:k] for x in NAMES})
        assert len({tuple(r[:3]) for r in got.tolist()}) == k, f"capacity {cap}: repeated entries"
        assert all(member.get(tuple(r[:3])) == tuple(r[3:]) for r in got.tolist()), f"capacity {cap}: not one of the model's rows"
        for x in NAMES:
            assert (a[x][k:] == 0x5B).all(), f"capacity {cap}: {x} written past min(total, capacity)"
    assert raw_call(m, None, None, 9, 0.0, 0, {}) == (0, total)                   # capacity 0 sizes the buffers
    assert raw_call(m, None, None, 9, 0.0, total, {}) == (0, total)
    # the same set whatever the launch shape: two halves add up
    halves = [m.GetSkeletonVoxels((0, 0, 0), (5, 9, 39)), m.GetSkeletonVoxels((6, 0, 0), (11, 9, 39))]
    assert_same({x: np.concatenate([h[x] for h in halves]) for x in NAMES}, model(), "two halves")


# ---- 5. engines -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["cells", "envelope", "rounds", "levels", "masked"])
def test_engines(hip_lib, engine):
    from test_gpu_planner_map_states import dense_for
    m = dense_for(engine, full=engine in ("cells", "envelope"))    # (these two serve fully observed maps only)
    model = DenseModel(m)
    for min_sep2, c in ((9, 0.0), (25, 0.3)):
        want = model(min_sep2, min_clearance=c)
        print(f"{engine}: min_sep2 {min_sep2} clearance {c}: {len(want['mask'])} skeleton voxels")
        assert len(want["mask"]) > 100
        assert_same(m.GetSkeletonVoxels(min_sep2=min_sep2, min_clearance=c), want, f"{engine} min_sep2 {min_sep2} clearance {c}")
    lo, hi = pp.Layout.scene().frontier_box
    want = model(9, lo, hi)
    assert 0 < len(want["mask"]) < len(model()["mask"])
    assert_same(m.GetSkeletonVoxels(lo, hi, 9), want, f"{engine} boxed")
    m.close()


# ---- 6. stale field ---------------------------------------------------------------------------------------------------------------
def test_field_not_yet_updated(hip_lib):
    m = two_blob_scene()
    before = DenseModel(m)
    old = rows(before())
    new_occ = old[:: max(len(old) // 6, 1), :3].astype(np.int32)      # a few skeleton voxels become obstacles
    for _ in range(3):
        m.SetOccupancy(new_occ, 1, want_ret=False)
        m.UpdateOccupancy(True)
    stale = DenseModel(m)
    assert stale.occ[tuple(new_occ.T)].all() and np.array_equal(stale.d2, before.d2) and np.array_equal(stale.coc, before.coc)
    want = stale()
    got = m.GetSkeletonVoxels(min_sep2=9)
    assert_same(got, want, "before UpdateESDF")
    g = rows(got)
    # newly occupied voxels drop out; everything else is the old answer, ids included
    keep = np.array([tuple(r[:3]) not in {tuple(v) for v in new_occ.tolist()} for r in old.tolist()])
    assert len(g) == int(keep.sum()) < len(old) and np.array_equal(g, old[keep])
    m.UpdateESDF()
    fresh = DenseModel(m)
    assert not np.array_equal(fresh.d2, before.d2)
    assert len(fresh()["mask"]) > 0
    assert_same(m.GetSkeletonVoxels(min_sep2=9), fresh(), "after UpdateESDF")
    m.close()


# ---- 7. hash-block map ------------------------------------------------------------------------------------------------------------
LONE_BOX = ((66, 18, 2), (76, 28, 20))          # map voxels: inside tile (4, 1, 0), none of whose six neighbour tiles has a page
LONE_OBSTACLES = ((68, 23, 10), (74, 23, 10))


def test_hash_block_map(hip_lib):
    m = pp.hash_scene()
    m.SetOccupancyBox(LONE_BOX[0], LONE_BOX[1], 0)
    m.UpdateOccupancy(True)
    pp.occupy(m, np.array(LONE_OBSTACLES, np.int32))
    m.UpdateESDF()
    model = HashModel(m)
    tiles = {(int(v[0]) >> 4, int(v[1]) >> 4, int(v[2]) >> 5) for v in m.download_hash()["vox"][::8192]}
    assert (4, 1, 0) in tiles and not tiles & {(3, 1, 0), (5, 1, 0), (4, 0, 0), (4, 2, 0), (4, 1, -1), (4, 1, 1)}
    whole = model()
    w = rows(whole)
    lone = w[(w[:, 0] >= LONE_BOX[0][0]) & (w[:, 0] <= LONE_BOX[1][0])]
    print(f"hash: {len(w)} skeleton voxels, {len(lone)} on the lone page")
    assert len(w) > 500 and (lone[:, 0] == 71).sum() > 20                     # half way between the two obstacles
    one = tuple(int(v) for v in lone[lone[:, 0] == 71][5, :3])
    assert (w[:, 0] < 0).any() and (w[:, 2] < 0).any()                        # negative coordinates
    for axis, size in ((0, 16), (1, 16), (2, 32)):                            # ridges across tile faces in all three axes
        lo_side = (w[:, axis] % size == size - 1) & (w[:, 3] & (2 << (2 * axis)) != 0)
        hi_side = (w[:, axis] % size == 0) & (w[:, 3] & (1 << (2 * axis)) != 0)
        assert (lo_side | hi_side).any(), f"no ridge across a tile face of axis {axis}"

    s = HASH_SHIFT.astype(np.int64)
    boxes = [(s + (5, 4, 10), s + (40, 30, 50)), (LONE_BOX[0], LONE_BOX[1]), (one, one), (s + (15, 0, 0), s + (16, 40, 71)),
             ((-100, -100, -100), (100, 100, 100)), ((500, 0, 0), (600, 9, 9)), ((5, 5, 5), (4, 9, 9)),
             ((-2**31, -2**31, -2**31), (2**31 - 1, 2**31 - 1, 2**31 - 1))]
    want_box = [model(9, lo, hi) for lo, hi in boxes]
    want_c = {(min_sep2, c): model(min_sep2, min_clearance=c) for min_sep2, c in ((25, 0.0), (9, 0.25), (16, 0.3))}
    assert all(len(w_["mask"]) > 0 for w_ in want_c.values())
    assert [len(w_["mask"]) for w_ in want_box[2:3] + want_box[5:7]] == [1, 0, 0] and all(len(w_["mask"]) > 0 for w_ in want_box[:5])

    def compare(what):                       # (the models are read once: both passes ask for the same answers)
        assert_same(m.GetSkeletonVoxels(min_sep2=9), whole, f"hash {what}")
        for (min_sep2, c), want in want_c.items():
            assert_same(m.GetSkeletonVoxels(min_sep2=min_sep2, min_clearance=c), want, f"hash {what} min_sep2 {min_sep2} clearance {c}")
        for (lo, hi), want in zip(boxes, want_box):
            assert_same(m.GetSkeletonVoxels(lo, hi, 9), want, f"hash {what} box {lo} {hi}")

    compare("resident")
    pages = m.grid_total_size_
    m.hash_recentre(HASH_SHIFT + np.array([24 + 512, 20, 36], np.int32))       # parks the lower half in x
    org = m.hash_window()[0]
    assert HASH_SHIFT[0] + 3 < org[0] <= HASH_SHIFT[0] + 44 and m.grid_total_size_ == pages
    compare("half parked")
    m.close()


# ---- 8. the device chain ----------------------------------------------------------------------------------------------------------
def test_device_chain_into_clusters(hip_lib):
    import torch
    from fiesta_amd import cluster_model
    from fiesta_amd._lib import ClusterInfo
    from fiesta_amd.esdf_map import CLUSTER_FIELDS
    from test_cpp_skeleton import example_scene
    m = example_scene()                        # two rooms and a doorway: walls in the plane x = 20, the doorway y = 18 .. 21
    model = DenseModel(m)
    want = model()
    total = len(want["mask"])
    assert total > 500
    cap = total + 50
    dev = torch.device("cuda", 0)
    t = {"vox": torch.full((cap, 3), -7, dtype=torch.int32, device=dev), "mask": torch.full((cap,), 0x5B, dtype=torch.uint8, device=dev),
         "d2": torch.full((cap,), -7, dtype=torch.int32, device=dev), "sep2": torch.full((cap,), -7, dtype=torch.int32, device=dev),
         "label": torch.full((cap,), -7, dtype=torch.int32, device=dev), "offsets": torch.zeros(cap + 1, dtype=torch.int64, device=dev),
         "members": torch.zeros(cap, dtype=torch.int64, device=dev), "head": torch.full((8,), 99, dtype=torch.int64, device=dev)}
    per_cluster = tuple(name for name, _, _ in CLUSTER_FIELDS)
    for name, dtype, shape in CLUSTER_FIELDS:
        t[name] = torch.zeros((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    torch.cuda.synchronize()                   # (the map's stream does not wait for torch's: the fills above must have landed)
    head = t["head"].data_ptr()
    m.GetSkeletonVoxelsDevice(None, None, 9, 0.0, cap, head, vox_dev_ptr=t["vox"].data_ptr(), mask_dev_ptr=t["mask"].data_ptr(),
                              d2_dev_ptr=t["d2"].data_ptr(), sep2_dev_ptr=t["sep2"].data_ptr())
    m.ClusterVoxelsDevice(t["vox"].data_ptr(), cap, head + 8, mask_dev_ptr=t["mask"].data_ptr(), key_dev_ptr=t["d2"].data_ptr(), n_dev_ptr=head,
                          connectivity=26, min_size=5, cluster_capacity=cap, member_capacity=cap,
                          out={k: t[k].data_ptr() for k in ("label", "offsets", "members") + per_cluster})
    m.synchronize()
    t = {k: v.cpu().numpy() for k, v in t.items()}
    assert t["head"][0] == total and t["head"][7] == 99
    sk = {x: t[x][:total] for x in NAMES}
    assert_same(sk, want, "device variant")
    assert_same(sk, m.GetSkeletonVoxels(min_sep2=9), "device against host variant")
    for x in NAMES:
        assert (t[x][total:] == (0x5B if x == "mask" else -7)).all(), f"{x} written past the total"
    cl = cluster_model(sk["vox"], mask=sk["mask"], key=sk["d2"], connectivity=26, min_size=5, resolution=m.resolution, origin=m.origin)
    k = cl["n_clusters"]
    assert k >= 1
    for i, (name, _) in enumerate(ClusterInfo._fields_):
        assert int(t["head"][1 + i]) == cl[name], name
    for name in per_cluster:
        a, b = t[name][:k], cl[name]
        assert (a.view(np.int64).tolist() == b.view(np.int64).tolist()) if name == "centroid" else np.array_equal(a, b), name
    assert np.array_equal(t["label"][:total], cl["label"]) and np.array_equal(t["offsets"][:k + 1], cl["offsets"])
    for c in range(k):
        seg = slice(int(cl["offsets"][c]), int(cl["offsets"][c + 1]))
        assert sorted(t["members"][seg].tolist()) == sorted(cl["members"][seg].tolist())
    # the narrowest member of the piece that runs through the doorway stands in it, two voxels from either door post
    big = int(np.argmax(t["size"][:k]))
    v = sk["vox"][int(t["key_argmin"][big])]
    assert int(t["key_min"][big]) == 4 and v[0] == 20 and v[1] in (19, 20), (t["key_min"][big], v)
    # a capacity below the total: the count is the total, the rows written are the model's
    small = {x: torch.full((40, 3) if x == "vox" else (40,), 0, dtype=getattr(torch, np.dtype(DTYPES[x]).name), device=dev) for x in NAMES}
    count = torch.full((1,), 123456789, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for _ in range(2):                         # (the call zeroes its counter)
        m.GetSkeletonVoxelsDevice(None, None, 9, 0.0, 32, count.data_ptr(), *[small[x].data_ptr() for x in NAMES])
        m.synchronize()
        assert int(count.item()) == total
    member = {tuple(r[:3]): tuple(r[3:]) for r in rows(want).tolist()}
    got = rows({x: small[x].cpu().numpy()[:32] for x in NAMES})
    assert len({tuple(r[:3]) for r in got.tolist()}) == 32 and all(member.get(tuple(r[:3])) == tuple(r[3:]) for r in got.tolist())
    assert all((small[x].cpu().numpy()[32:] == 0).all() for x in NAMES)
    count.fill_(5)
    torch.cuda.synchronize()
    m.GetSkeletonVoxelsDevice((5, 5, 5), (4, 9, 9), 9, 0.0, 32, count.data_ptr())          # an empty box still zeroes the counter
    m.synchronize()
    assert int(count.item()) == 0
    m.close()


# ---- 9. whole-call errors ---------------------------------------------------------------------------------------------------------
def test_errors_leave_the_map_usable(boxed):
    import fiesta_amd
    m, model = boxed
    a = {x: np.zeros((4, 3) if x == "vox" else 4, DTYPES[x]) for x in NAMES}
    bad = [raw_call(m, None, None, 0, 0.0, 4, a), raw_call(m, None, None, -5, 0.0, 4, a), raw_call(m, None, None, 9, np.nan, 4, a),
           raw_call(m, (0, 0, 0), None, 9, 0.0, 4, a), raw_call(m, None, (5, 5, 5), 9, 0.0, 4, a), raw_call(m, None, None, 9, 0.0, -1, a),
           raw_call(m, None, None, 9, 0.0, 4, a, n_out=False), raw_call(m, None, None, 9, 0.0, 4, a, result=False)]
    for st, n in bad:
        assert st == ERR_INVALID and n == -1          # nothing written
    assert not any(v.any() for v in a.values())
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.GetSkeletonVoxels(min_sep2=0)
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.GetSkeletonVoxels(min_clearance=float("nan"))
    with pytest.raises(ValueError):
        m.GetSkeletonVoxels(lo=(0, 0, 0))
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.GetSkeletonVoxelsDevice((0, 0, 0), None, 9, 0.0, 0, 8)
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.GetSkeletonVoxelsDevice(None, None, 9, 0.0, 0, 0)
    assert_same(m.GetSkeletonVoxels(), model(), "after the errors")


# ---- 10. determinism --------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_rows(boxed):
    m, model = boxed
    a, b = m.GetSkeletonVoxels(min_sep2=9, min_clearance=0.15), m.GetSkeletonVoxels(min_sep2=9, min_clearance=0.15)
    assert len(a["mask"]) > 0 and np.array_equal(rows(a), rows(b))
    assert_same(a, model(9, min_clearance=0.15), "clearance 0.15")
    got = m.GetSkeletonVoxels(min_sep2=9, want=("vox", "sep2"))
    assert set(got) == {"vox", "sep2", "n"} and got["n"] == len(model()["mask"])
