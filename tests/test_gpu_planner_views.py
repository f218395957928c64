"""What a store prepares before a planner call reads it (DenseMap / HashMap::planner_view, fiesta_amd/csrc/planner.hip).

A hash-block map answers a planner call through the page table as it stood when the call fetched its view: a page added by the
last update must be in it before the call's first kernel is enqueued, also when that call is a _dev variant and the first call
after the update.  Sequence: a few obstacles in one tile, UpdateESDF, one query (a page table now exists), a few obstacles 64
voxels further along x in a tile that has no page yet, UpdateESDF -- then the _dev call straight away, the host call after it.
"hash-parked" also moves the window away, so that every lookup goes through the page table; the dense map runs the same sequence
through its own view.  Device and host variant are compared bit for bit.
"""
import numpy as np
import pytest

from scenarios import P_DEFAULT

pytestmark = pytest.mark.gpu
RES = 0.1
DIMS = (96, 16, 32)
FIRST = np.array([(8, 8, 8), (8, 9, 8), (9, 8, 8)], np.int32)
SECOND = FIRST + np.array((64, 0, 0), np.int32)       # x = 72, 73: the tile x = 64 .. 79
RAY_FIELDS = ("n_visited", "hit_index", "hit_class", "hit_vox", "hit_dist", "counts")
OCC = 1


def observe(m, x0, S):
    """the tile's voxels observed free, then S observed occupied"""
    m.SetOccupancyBox((x0, 0, 0), (x0 + 15, DIMS[1] - 1, DIMS[2] - 1), 0)
    m.UpdateOccupancy(True)
    for _ in range(3):
        m.SetOccupancy(S, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()


def build(store):
    import fiesta_amd
    if store == "dense":
        m = fiesta_amd.ESDFMap((0, 0, 0), RES, tuple((s - 0.5) * RES for s in DIMS))
        assert m.grid_size == DIMS
    else:
        m = fiesta_amd.ESDFMap((0, 0, 0), RES, reserve_size=100000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    observe(m, 0, FIRST)
    pages = m.grid_total_size_
    assert m.GetDistance(np.array([[10, 8, 8]], np.int32))[0] == RES      # (a query: the hash store builds its page table)
    observe(m, 64, SECOND)
    if store != "dense":
        assert m.grid_total_size_ > pages                                # the second tile got a page of its own
    if store == "hash-parked":
        m.hash_recentre((3000, -3000, 3000))
        assert m.grid_total_size_ > pages
    return m


@pytest.mark.parametrize("store", ["dense", "hash", "hash-parked"])
def test_dev_ray_query_right_after_an_update_that_added_a_page(hip_lib, store):
    import torch
    m = build(store)
    # a dozen rays along +x through the second tile, y = 7 .. 10, z = 7 .. 9: those at (y, z) = (8, 8) and (9, 8) meet an obstacle
    yz = np.array([(y, z) for y in range(7, 11) for z in range(7, 10)], np.float64)
    start = np.column_stack([np.full(len(yz), 66.5), yz + 0.5]) * RES
    end = np.column_stack([np.full(len(yz), 78.5), yz + 0.5]) * RES
    dev, n = torch.device("cuda", 0), len(yz)
    shapes = {"n_visited": ((n,), torch.int32), "hit_index": ((n,), torch.int32), "hit_class": ((n,), torch.uint8),
              "hit_vox": ((n, 3), torch.int32), "hit_dist": ((n,), torch.float64), "counts": ((n, 4), torch.int32)}
    out = {k: torch.full(shape, 77, dtype=dtype, device=dev) for k, (shape, dtype) in shapes.items()}
    s, e = torch.from_numpy(start).to(dev), torch.from_numpy(end).to(dev)
    torch.cuda.synchronize()   # (the map's stream does not wait for torch's)
    m.RayQueryDevice(s.data_ptr(), e.data_ptr(), n, OCC, {k: t.data_ptr() for k, t in out.items()})
    m.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    for i, (y, z) in enumerate(yz.astype(int)):
        want = {(8, 8): [72, 8, 8], (9, 8): [72, 9, 8]}.get((y, z))
        if want is not None:
            assert got["hit_class"][i] == OCC and got["hit_vox"][i].tolist() == want, (store, y, z, got["hit_vox"][i])
    assert (got["hit_class"] == OCC).sum() == 2 and (got["hit_index"] < 0).sum() == n - 2, (store, got["hit_index"])
    assert got["counts"][:, 2].sum() == 0, (store, got["counts"])       # no voxel of the second tile reads as unknown
    host = m.RayQuery(start, end, OCC)
    for k in RAY_FIELDS:
        g, h = got[k], host[k]
        assert g.dtype == h.dtype and g.shape == h.shape, (store, k)
        if k == "hit_dist":
            assert np.array_equal(np.isnan(g), np.isnan(h)), (store, k)
            g, h = g[~np.isnan(g)].view(np.uint64), h[~np.isnan(h)].view(np.uint64)
        assert np.array_equal(g, h), (store, k, g, h)
    m.close()


@pytest.mark.parametrize("store", ["dense", "hash", "hash-parked"])
def test_dev_reach_field_right_after_an_update_that_added_a_page(hip_lib, store):
    import torch
    m = build(store)
    lo, hi = (0, 0, 0), tuple(d - 1 for d in DIMS)                         # 96 x 16 x 32 voxels: both tiles and the unknown space between
    dev = torch.device("cuda", 0)
    seeds = torch.tensor([[66, 8, 8]], dtype=torch.int32, device=dev)
    cost = torch.full(DIMS, 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    info = m.ReachFieldDevice(seeds.data_ptr(), 1, lo, hi, cost_dev_ptr=cost.data_ptr())
    got = cost.cpu().numpy()
    assert info["n_seeds_used"] == 1 and info["n_traversable"] == 2 * (16 * 16 * 32 - 3), (store, info)
    assert info["n_reached"] == 16 * 16 * 32 - 3, (store, info)          # the second tile's free voxels; the first lies behind unknown space
    assert got[66, 8, 8] == 0 and got[70, 8, 8] == 12 and got[72, 8, 8] == -1 and got[8, 8, 8] == -1, (store, got[66:74, 8, 8])
    assert got[10, 8, 8] == np.iinfo(np.int32).max and got[40, 8, 8] == -1
    host = m.ReachField(np.array([[66, 8, 8]], np.int32), lo, hi)
    assert np.array_equal(got, host["cost"]), (store, np.argwhere(got != host["cost"])[:5])
    for k in ("box_lo", "box_hi", "n_traversable", "n_seeds_used", "n_reached", "max_cost"):
        assert host[k] == info[k], (store, k, host[k], info[k])
    m.close()
