"""Frontier extraction on the GPU (fiesta_hip_get_frontier_voxels[_dev], include/fiesta_hip.h; kernels:
fiesta_amd/csrc/frontier_kernels.hpp).

The expected set is always fiesta_amd.frontier_model (the header's definition in numpy; tests/test_frontier_rule.py checks it against a
plain loop) fed from what the map itself reports through the calls that existed before: download_field (d2 >= 0, occ) or
download_hash, and GetDistance of every voxel -- never from the call under test.  Everything is integer: results are compared as
sorted (x, y, z, mask) rows, tolerance zero.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from scenarios import P_DEFAULT, all_voxels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.1


def rows(vox, mask):
    a = np.concatenate([np.asarray(vox, np.int64).reshape(-1, 3), np.asarray(mask, np.int64).reshape(-1, 1)], 1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def assert_same(got, want, what=""):
    g, w = rows(*got), rows(*want)
    assert g.shape == w.shape, f"{what}: {len(g)} frontier voxels, the model has {len(w)}"
    bad = np.nonzero((g != w).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first got {g[bad[:3]].tolist()} want {w[bad[:3]].tolist()}"


def make_dense(shape, observed, occupied=(), res=RES):
    """a dense map of `shape` voxels in which exactly the voxels of the boolean array `observed` (and the occupied ones) were seen"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), res, tuple((s - 0.5) * res for s in shape))   # (ceil(size / res) voxels)
    assert m.grid_size == tuple(shape)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancy(np.argwhere(observed).astype(np.int32), 0, want_ret=False)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    if len(occupied):
        S = np.asarray(occupied, np.int32).reshape(-1, 3)
        for _ in range(3):
            m.SetOccupancy(S, 1, want_ret=False)
            m.UpdateOccupancy(True)
        m.UpdateESDF()
    return m


class DenseModel:
    """frontier_model on the map's own dump, read once"""

    def __init__(self, m):
        f = m.download_field(("d2", "occ"))
        self.obs = (f["d2"] >= 0).reshape(m.grid_size)
        self.occ = f["occ"].reshape(m.grid_size) != 0
        self.dist = m.GetDistance(all_voxels(m.grid_size)).reshape(m.grid_size)

    def __call__(self, lo=None, hi=None, min_clearance=0.0):
        from fiesta_amd import frontier_model
        return frontier_model(self.obs, self.occ, self.dist, lo, hi, min_clearance)


class HashModel:
    """frontier_model on download_hash scattered into an array padded by one voxel, whose outside counts as unknown"""

    def __init__(self, m):
        h = m.download_hash()
        self.org = h["vox"].min(0).astype(np.int64) - 1
        shape = tuple(int(v) for v in (h["vox"].max(0) - self.org + 2))
        i = tuple((h["vox"] - self.org).T)
        self.obs, self.occ, self.dist = np.zeros(shape, bool), np.zeros(shape, bool), np.full(shape, 10000.0)
        self.obs[i] = h["d2"] >= 0
        self.occ[i] = h["occ"] != 0
        self.dist[i] = m.GetDistance(h["vox"])

    def __call__(self, lo=None, hi=None, min_clearance=0.0):
        from fiesta_amd import frontier_model
        return frontier_model(self.obs, self.occ, self.dist, lo, hi, min_clearance, origin_vox=self.org, bounded=False)


def ragged_scene(nz, variant):
    """12 x 10 x nz voxels: a free box that stops 2 voxels short of every face with a 3 x 3 x 3 unknown pocket, occupied voxels (on
    the box's boundary, next to the pocket, inside), lone observed voxels at two grid corners and at z = nz - 1"""
    nx, ny = 12, 10
    obs = np.zeros((nx, ny, nz), bool)
    zc = max(nz // 2, 3)
    if variant == "faces":        # observed up to the map's faces: the outer face is no frontier, only the pocket is left
        obs[:] = True
    elif variant == "carry_low":  # the observed / unknown boundary exactly between z = 31 and z = 32, unknown above
        obs[2:nx - 2, 2:ny - 2, 2:32] = True
        zc = 29
    elif variant == "carry_high":  # ... unknown below
        obs[2:nx - 2, 2:ny - 2, 32:nz] = True
        zc = 33
    else:
        obs[2:nx - 2, 2:ny - 2, 2:nz - 2] = True
    obs[5:8, 4:7, zc - 1:zc + 2] = False
    obs[0, 0, 0] = obs[nx - 1, ny - 1, nz - 1] = obs[6, 0, nz - 1] = obs[nx - 1, 0, 0] = True
    zi = int(np.argwhere(obs[3, 3])[0][0])
    occupied = {(2, 2, zi), (nx - 3, 5, min(zi + 1, nz - 1)), (4, 5, min(zc, nz - 1)), (3, 6, min(zi + 2, nz - 1)), (6, 5, min(zc + 2, nz - 1))}
    return obs, sorted(occupied)


@pytest.mark.parametrize("nz,variant", [(7, "box"), (32, "box"), (33, "box"), (40, "box"), (7, "faces"), (33, "faces"), (40, "faces"),
                                        (33, "carry_low"), (40, "carry_low"), (33, "carry_high"), (40, "carry_high")])
def test_dense_ragged_z(hip_lib, nz, variant):
    obs, occupied = ragged_scene(nz, variant)
    m = make_dense(obs.shape, obs, occupied)
    model = DenseModel(m)
    assert np.array_equal(model.obs, obs | model.occ) and model.occ.sum() == len(occupied)
    want = model()
    w = rows(*want)
    nx, ny = obs.shape[:2]
    inner = w[(w[:, 0] >= 2) & (w[:, 0] <= nx - 3) & (w[:, 1] >= 2) & (w[:, 1] <= ny - 3)]   # (without the lone voxels)
    if variant == "faces":
        assert len(w) == 6 * 9 - 2 and not ((w[:, :3] == 0).all(1)).any()    # the pocket's 54 face neighbours but two occupied ones
    else:
        lone = {tuple(r[:3]): r[3] for r in w.tolist()}
        assert lone[(0, 0, 0)] == 0b101010 and lone[(nx - 1, ny - 1, nz - 1)] == 0b010101 and lone[(6, 0, nz - 1)] == 0b011011
    assert not {tuple(r[:3]) for r in w.tolist()} & set(occupied)
    if variant == "carry_low":
        assert ((inner[:, 2] == 31) & (inner[:, 3] == 32)).any() and not (inner[:, 2] == 32).any()
    if variant == "carry_high":
        assert ((inner[:, 2] == 32) & (inner[:, 3] == 16)).any() and not (inner[:, 2] == 31).any()
    assert_same(m.GetFrontierVoxels(), want, f"nz {nz} {variant}")
    assert_same(m.GetFrontierVoxels(min_clearance=0.25), model(min_clearance=0.25), f"nz {nz} {variant} clearance 0.25")
    vox, mask = m.GetFrontierVoxels(want_mask=False)
    assert mask is None and np.array_equal(rows(vox, np.zeros(len(vox)))[:, :3], w[:, :3])
    m.close()


@pytest.fixture(scope="module")
def boxed(hip_lib):
    obs, occupied = ragged_scene(40, "box")
    m = make_dense(obs.shape, obs, occupied)
    yield m, DenseModel(m)
    m.close()


def test_box_semantics(boxed):
    m, model = boxed
    nx, ny, nz = m.grid_size
    whole = model()
    assert len(whole[1]) > 100
    assert_same(m.GetFrontierVoxels((-5, -5, -5), (100, 100, 100)), whole, "a box around everything")
    assert_same(m.GetFrontierVoxels((0, 0, 0), (nx - 1, ny - 1, nz - 1)), whole, "the array's own box")
    # a box that cuts through the frontier keeps the voxels whose unknown neighbour lies outside it
    lo, hi = (3, 3, 3), (nx - 3, ny - 3, nz - 3)
    got = m.GetFrontierVoxels(lo, hi)
    assert_same(got, model(lo, hi), "cutting box")
    g = rows(*got)
    assert ((g[:, 0] == nx - 3) & (g[:, 3] & 2 != 0)).any() and ((g[:, 2] == nz - 3) & (g[:, 3] & 32 != 0)).any()
    assert 0 < len(g) < len(whole[1])
    boxes = [((-3, -3, -3), (5, 5, 20)),            # partly outside the map
             ((4, 2, 30), (9, 8, 33)),              # across the word boundary z = 31 | 32
             ((4, 2, 33), (9, 8, 38)), ((4, 2, 5), (9, 8, 5)),     # inside one word; one z-plane
             ((2, 2, 2), (2, 2, 2)), ((6, 5, 10), (6, 5, 10)), ((0, 0, 0), (0, 0, 0)),   # single voxels: frontier, interior, corner
             ((nx - 1, ny - 1, nz - 1), (nx + 7, ny + 7, nz + 7)),
             ((100, 100, 100), (200, 200, 200)), ((-9, -9, -9), (-1, 50, 50)), ((0, 0, nz), (nx, ny, nz + 5)),   # wholly outside
             ((5, 5, 5), (4, 9, 9)), ((5, 5, 5), (9, 4, 9)), ((5, 5, 5), (9, 9, 4)),                            # lo > hi
             ((-2**31, -2**31, -2**31), (2**31 - 1, 2**31 - 1, 2**31 - 1))]
    counts = []
    for lo, hi in boxes:
        want = model(lo, hi)
        assert_same(m.GetFrontierVoxels(lo, hi), want, f"box {lo} {hi}")
        assert_same(m.GetFrontierVoxels(lo, hi, 0.25), model(lo, hi, 0.25), f"box {lo} {hi} clearance 0.25")
        counts.append(len(want[1]))
    assert counts[4] == 0 and counts[5] == 0 and counts[6] == 1 and counts[7] == 1   # (2, 2, 2) is occupied in this scene
    assert counts[8:14] == [0] * 6 and counts[14] == len(whole[1]) and min(counts[:4]) > 0


def test_clearance(boxed):
    m, model = boxed
    whole = model()
    sizes = []
    for c in (0.05, 0.25, 1.0, 9999.0, 10001.0):
        want = model(min_clearance=c)
        assert_same(m.GetFrontierVoxels(min_clearance=c), want, f"clearance {c}")
        sizes.append(len(want[1]))
    assert len(whole[1]) >= sizes[0] > sizes[1] > 0 and sizes[4] == 0, sizes
    for c in (0.0, -0.0, -1.0, -np.inf):
        assert_same(m.GetFrontierVoxels(min_clearance=c), whole, f"clearance {c}: no filter")
    assert_same(m.GetFrontierVoxels(min_clearance=np.inf), model(min_clearance=np.inf), "clearance inf")


def test_clearance_of_no_obstacle_and_of_a_field_not_yet_updated(hip_lib):
    obs, _ = ragged_scene(33, "box")
    m = make_dense(obs.shape, obs)                        # no obstacle anywhere: every observed voxel reads +10000
    model = DenseModel(m)
    assert (model.dist[model.obs] == 10000.0).all()
    whole = model()
    assert len(whole[1]) > 100
    assert_same(m.GetFrontierVoxels(min_clearance=9999.0), whole, "+10000 passes 9999")
    assert len(m.GetFrontierVoxels(min_clearance=10001.0)[0]) == 0
    # the field is read as it stands: after UpdateOccupancy and before UpdateESDF the filter sees the old distances
    for _ in range(3):
        m.SetOccupancy(np.array([[4, 4, 4]], np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)
    stale = DenseModel(m)
    assert stale.occ[4, 4, 4] and stale.dist[4, 4, 5] == 10000.0
    assert_same(m.GetFrontierVoxels(min_clearance=0.25), stale(min_clearance=0.25), "before UpdateESDF")
    m.UpdateESDF()
    fresh = DenseModel(m)
    assert fresh.dist[4, 4, 5] == RES
    assert_same(m.GetFrontierVoxels(min_clearance=0.25), fresh(min_clearance=0.25), "after UpdateESDF")
    assert len(fresh(min_clearance=0.25)[1]) < len(stale(min_clearance=0.25)[1])
    m.close()


@pytest.fixture(scope="module")
def chequered(hip_lib):
    """40^3, every second voxel observed: 16 frontier voxels per word, 1024 per wave, 3200 words (13 work-groups)"""
    V = all_voxels(40)
    obs = (V.sum(1) % 2 == 0).reshape(40, 40, 40)
    m = make_dense(obs.shape, obs, [(10, 10, 10), (20, 21, 21)])
    model = DenseModel(m)
    yield m, model
    m.close()


def raw_call(m, lo, hi, clearance, vox, mask, capacity, n_out=True):
    """the C call itself; returns (status, n_out)"""
    from fiesta_amd.esdf_map import _p
    n = C.c_int64(-1)
    blo = None if lo is None else np.ascontiguousarray(lo, np.int32)
    bhi = None if hi is None else np.ascontiguousarray(hi, np.int32)
    st = m._lib.fiesta_hip_get_frontier_voxels(m._h, _p(blo), _p(bhi), float(clearance), _p(vox), _p(mask), capacity, C.byref(n) if n_out else None)
    return st, n.value


def test_capacity_and_compaction(chequered):
    m, model = chequered
    want = rows(*model())
    total = len(want)
    assert total > 30000 and (want[:, 3] == 63).sum() > 20000
    member = {(int(r[0]) * 64 + int(r[1])) * 64 + int(r[2]): int(r[3]) for r in want}
    for cap in (0, 1, total - 1, total, total + 5):
        vox = np.full((cap + 8, 3), -77, np.int32)
        mask = np.full(cap + 8, 0xAB, np.uint8)
        st, n = raw_call(m, None, None, 0.0, vox, mask, cap)
        assert st == 0 and n == total, (cap, st, n)
        k = min(total, cap)
        keys = (vox[:k, 0].astype(np.int64) * 64 + vox[:k, 1]) * 64 + vox[:k, 2]
        assert len(np.unique(keys)) == k, f"capacity {cap}: repeated entries"
        assert all(member.get(int(key), -1) == int(u) for key, u in zip(keys, mask[:k])), f"capacity {cap}: not in the expected set"
        assert (vox[k:] == -77).all() and (mask[k:] == 0xAB).all(), f"capacity {cap}: written past min(total, capacity)"
    # only vox, only mask, neither
    vox = np.full((total, 3), -77, np.int32)
    st, n = raw_call(m, None, None, 0.0, vox, None, total)
    assert st == 0 and n == total and np.array_equal(rows(vox, np.zeros(total))[:, :3], want[:, :3])
    mask = np.full(total, 0xAB, np.uint8)
    st, n = raw_call(m, None, None, 0.0, None, mask, total)
    assert st == 0 and n == total and np.array_equal(np.sort(mask), np.sort(want[:, 3]).astype(np.uint8))
    assert raw_call(m, None, None, 0.0, None, None, total) == (0, total)
    assert raw_call(m, None, None, 0.0, None, None, 0) == (0, total)
    # the same set whatever the launch shape: boxes of one column, one plane, half the map add up
    halves = [m.GetFrontierVoxels((0, 0, 0), (19, 39, 39)), m.GetFrontierVoxels((20, 0, 0), (39, 39, 39))]
    assert_same((np.concatenate([h[0] for h in halves]), np.concatenate([h[1] for h in halves])), model(), "two halves")
    assert_same(m.GetFrontierVoxels(min_clearance=0.15), model(min_clearance=0.15), "chequered, clearance 0.15")


def device_call(m, lo, hi, clearance, capacity, fill=-7):
    import torch
    dev = torch.device("cuda", 0)
    vox = torch.full((capacity + 4, 3), fill, dtype=torch.int32, device=dev)
    mask = torch.full((capacity + 4,), 0xAB, dtype=torch.uint8, device=dev)
    count = torch.full((1,), 123456789, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's: the fills above must have landed)
    m.GetFrontierVoxelsDevice(lo, hi, clearance, vox.data_ptr(), mask.data_ptr(), capacity, count.data_ptr())
    m.synchronize()
    first = int(count.item())
    m.GetFrontierVoxelsDevice(lo, hi, clearance, vox.data_ptr(), mask.data_ptr(), capacity, count.data_ptr())
    m.synchronize()
    assert int(count.item()) == first, "the call zeroes its counter"
    return first, vox.cpu().numpy(), mask.cpu().numpy()


def test_device_variant(chequered, boxed):
    for (m, model), clearance in ((chequered, 0.0), (boxed, 0.0), (boxed, 0.25)):
        want = model(min_clearance=clearance)
        total = len(want[1])
        n, vox, mask = device_call(m, None, None, clearance, total)
        assert n == total
        assert_same((vox[:total], mask[:total]), want, "device variant")
        assert_same((vox[:total], mask[:total]), m.GetFrontierVoxels(min_clearance=clearance), "device against host variant")
        assert (vox[total:] == -7).all() and (mask[total:] == 0xAB).all()
        n, vox, mask = device_call(m, None, None, clearance, total - 9)
        assert n == total and (vox[total - 9:] == -7).all() and (mask[total - 9:] == 0xAB).all()
    m, model = boxed
    lo, hi = (3, 3, 30), (9, 8, 35)
    want = model(lo, hi)
    n, vox, mask = device_call(m, lo, hi, 0.0, 500)
    assert n == len(want[1]) > 0
    assert_same((vox[:n], mask[:n]), want, "device variant, boxed")
    n, vox, mask = device_call(m, (5, 5, 5), (4, 9, 9), 0.0, 16)      # an empty box still zeroes the counter
    assert n == 0 and (vox == -7).all()
    # null outputs: the count alone
    import torch
    count = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    m.GetFrontierVoxelsDevice(None, None, 0.0, 0, 0, 0, count.data_ptr())
    m.synchronize()
    assert int(count.item()) == len(model()[1])


def hash_scene(shift):
    """free boxes laid against tile faces (tiles are 16 x 16 x 32 voxels): one that fills tile (0, 0, 0) up to its high faces in x, y
    and z -- the tile beyond +x has a page (one lone observed voxel far inside it) but is unknown at the face, the tiles beyond +y and
    +z have no page --, one that straddles the negative coordinates and tile faces at -1 | 0, one that crosses x = 15 | 16 and
    lies in the tiles above z = 31 | 32; occupied voxels on a tile face and at negative coordinates"""
    import fiesta_amd
    s = np.asarray(shift, np.int32)
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=100000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    for lo, hi in (((3, 3, 3), (15, 15, 31)), ((30, 8, 8), (30, 8, 8)), ((-6, -5, -4), (2, 2, 2)), ((10, 20, 40), (22, 28, 50)),
                   ((16, 3, 20), (18, 6, 31)), ((4, 16, 30), (6, 17, 33))):
        m.SetOccupancyBox(s + lo, s + hi, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    S = s + np.array([(15, 8, 8), (-1, 0, 0), (8, 15, 31), (12, 24, 45), (0, 0, 0)], np.int32)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m, s


@pytest.mark.parametrize("shift", [(0, 0, 0), (-48, 32, -64), (-41, -23, -37)])
def test_hash_block_map(hip_lib, shift):
    m, s = hash_scene(shift)
    model = HashModel(m)
    want = model()
    w = rows(*want)
    assert len(w) > 500
    at = {tuple(r[:3] - s): r[3] for r in w.tolist()}
    # the faces of the first box: towards a tile with a page that is unknown there, towards tiles without a page (+y, +z)
    assert at[(15, 9, 9)] == 2 and at[(8, 15, 9)] == 8 and at[(8, 9, 31)] == 32 and at[(15, 15, 20)] == 2 + 8
    assert (15, 4, 25) not in at and at[(18, 4, 25)] & 2       # observed across x = 15 | 16: no frontier there, one farther on
    assert (5, 15, 30) not in at and (5, 16, 31) not in at and at[(5, 17, 33)] & 32      # ... across y = 15 | 16 and z = 31 | 32
    assert at[(-6, -5, -4)] == 1 + 4 + 16 and (15, 8, 8) not in at and (-1, 0, 0) not in at
    assert_same(m.GetFrontierVoxels(), want, f"hash {shift}")
    for c in (0.25, 1.0, 9999.0, 10001.0):
        assert_same(m.GetFrontierVoxels(min_clearance=c), model(min_clearance=c), f"hash {shift} clearance {c}")
    assert 0 < len(model(min_clearance=0.25)[1]) < len(w)
    for lo, hi in (((3, 3, 3), (15, 15, 31)), ((-100, -100, -100), (100, 100, 100)), ((15, 0, 0), (16, 40, 60)), ((0, 0, 31), (30, 30, 32)),
                   ((-6, -5, -4), (-6, -5, -4)), ((-3, -3, -3), (0, 0, 0)), ((200, 0, 0), (300, 9, 9)), ((5, 5, 5), (4, 9, 9)),
                   ((-2**31, -2**31, -2**31), (2**31 - 1, 2**31 - 1, 2**31 - 1))):
        lo, hi = s + np.array(lo, np.int64), s + np.array(hi, np.int64)
        lo, hi = np.clip(lo, -2**31, 2**31 - 1), np.clip(hi, -2**31, 2**31 - 1)
        assert_same(m.GetFrontierVoxels(lo, hi), model(lo, hi), f"hash {shift} box {lo} {hi}")
        assert_same(m.GetFrontierVoxels(lo, hi, 0.25), model(lo, hi, 0.25), f"hash {shift} box {lo} {hi} clearance 0.25")
    n, vox, mask = device_call(m, None, None, 0.25, len(w))
    assert_same((vox[:n], mask[:n]), model(min_clearance=0.25), f"hash {shift} device variant")
    # far away: every page is parked and still answers, the null box is still the whole map
    pages_before = m.grid_total_size_
    m.hash_recentre(s + np.array([3000, -3000, 3000]))
    assert m.grid_total_size_ == pages_before
    assert_same(m.GetFrontierVoxels(), want, f"hash {shift} parked")
    assert_same(m.GetFrontierVoxels(min_clearance=0.25), model(min_clearance=0.25), f"hash {shift} parked, clearance 0.25")
    lo, hi = s + np.array((3, 3, 3)), s + np.array((15, 15, 31))
    assert_same(m.GetFrontierVoxels(lo, hi), model(lo, hi), f"hash {shift} parked, boxed")
    m.close()


def test_shard_answers_for_its_own_array(hip_lib):
    """a shard (owned box + ghost layers): the observed set is the field's, also in ghost cells that the halo exchange filled"""
    import fiesta_amd
    from fiesta_amd import frontier_model
    gg = (32, 16, 16)
    shards = [fiesta_amd.ESDFMap((0, 0, 0), RES, (15.5 * RES,) * 3, shard_lo=lo, global_grid=gg) for lo in ((0, 0, 0), (16, 0, 0))]
    for sh in shards:
        sh.SetParameters(*P_DEFAULT)
        sh.SetOriginalRange()
    a, b = shards
    a.SetOccupancyBox((3, 3, 3), (15, 12, 12), 0)        # up to the face between the shards
    b.SetOccupancyBox((16, 5, 5), (20, 10, 14), 0)       # beyond it: A sees these through its ghost layer only
    for sh in shards:
        sh.UpdateOccupancy(True)
        sh.UpdateESDF()
    ia, ib = a.shard_info(), b.shard_info()
    oa, ob, da = np.array(ia["local_origin"]), np.array(ib["local_origin"]), np.array(ia["local_dims"])
    glo, ghi = np.array([16, 0, 0]), oa + da - 1         # A's ghost layer beyond +x, global coordinates
    assert ghi[0] >= 16
    changed = a.halo_apply(glo - oa, ghi - oa, b.halo_pack(glo - ob, ghi - ob))
    assert changed > 0
    f = a.download_field(("d2", "occ"))
    dims = tuple(int(v) for v in da)
    obs, occ = (f["d2"] >= 0).reshape(dims), f["occ"].reshape(dims) != 0
    assert obs[16 - oa[0], 7, 7] and not obs[16 - oa[0], 3, 3]
    dist = a.GetDistance(all_voxels(dims) + oa.astype(np.int32)).reshape(dims)
    for c in (0.0, 0.25):
        want = frontier_model(obs, occ, dist, min_clearance=c, origin_vox=oa)
        assert_same(a.GetFrontierVoxels(min_clearance=c), want, f"shard clearance {c}")
    at = {tuple(r[:3]): r[3] for r in rows(*frontier_model(obs, occ, origin_vox=oa)).tolist()}
    assert (15, 7, 7) not in at and at[(15, 4, 4)] & 2
    for sh in shards:
        sh.close()


def test_empty_hash_map(hip_lib):
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=1000, mode="hash")
    vox, mask = m.GetFrontierVoxels()
    assert vox.shape == (0, 3) and mask.shape == (0,)
    m.close()


def test_errors_leave_the_map_usable(boxed):
    import fiesta_amd
    from fiesta_amd._lib import check
    m, model = boxed
    vox, mask = np.zeros((4, 3), np.int32), np.zeros(4, np.uint8)
    bad = [raw_call(m, None, None, np.nan, vox, mask, 4), raw_call(m, (0, 0, 0), None, 0.0, vox, mask, 4),
           raw_call(m, None, (5, 5, 5), 0.0, vox, mask, 4), raw_call(m, None, None, 0.0, vox, mask, -1),
           raw_call(m, None, None, 0.0, vox, mask, 4, n_out=False)]
    for st, n in bad:
        assert st == 1 and n == -1                    # FIESTA_HIP_ERR_INVALID, nothing written
        with pytest.raises(fiesta_amd.FiestaHipError):
            check(st)
    assert not vox.any() and not mask.any()
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.GetFrontierVoxels(min_clearance=float("nan"))
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.GetFrontierVoxelsDevice((0, 0, 0), None, 0.0, 0, 0, 0, 8)
    with pytest.raises(fiesta_amd.FiestaHipError):
        m.GetFrontierVoxelsDevice(None, None, 0.0, 0, 0, 0, 0)
    assert_same(m.GetFrontierVoxels(), model(), "after the errors")


def example_scene():
    """the scene of examples/frontiers.cpp through the Python class"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap((-4.0, -4.0, 0.0), 0.2, (8.0, 8.0, 4.0))
    assert m.grid_size == (40, 40, 20)
    m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80)
    m.SetOriginalRange()
    V = all_voxels((40, 40, 20)).astype(np.int64)
    d = V - (5, 20, 10)
    cone = (V[:, 0] >= 6) & (V[:, 0] <= 30) & (d[:, 1] ** 2 + d[:, 2] ** 2 <= d[:, 0] ** 2) & ((d ** 2).sum(1) <= 28 * 28)
    hit = (V[:, 0] == 30) | ((V[:, 0] == 18) & (V[:, 1] >= 19) & (V[:, 1] <= 21))
    for cycle in range(3):
        if cycle == 0:
            m.SetOccupancy(V[cone & ~hit].astype(np.int32), 0, want_ret=False)
        m.SetOccupancy(V[cone & hit].astype(np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


def test_cpp_example_counts(hip_lib, tmp_path):
    """examples/frontiers.cpp against the facade: its three counts are the Python call's (and the model's) on the same scene"""
    import __graft_entry__ as g
    g.build_hip()
    exe = str(tmp_path / "frontiers")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frontiers.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, check=True)
    out = json.loads(run.stdout.strip().splitlines()[-1])
    print("example:", out)
    m = example_scene()
    model = DenseModel(m)
    vox, mask = m.GetFrontierVoxels()
    assert_same((vox, mask), model(), "example scene")
    faces = int(np.unpackbits(mask).sum())
    assert out["frontier"] == len(vox) > 500 and out["faces"] == faces
    assert out["clear"] == len(m.GetFrontierVoxels(min_clearance=0.3)[0]) == len(model(min_clearance=0.3)[1])
    assert out["boxed"] == len(m.GetFrontierVoxels((6, 0, 0), (17, 39, 19))[0]) == len(model((6, 0, 0), (17, 39, 19))[1])
    assert 0 < out["clear"] < out["frontier"] and 0 < out["boxed"] < out["frontier"]
    m.close()
