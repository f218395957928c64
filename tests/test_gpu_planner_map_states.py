"""The planner calls' view of the map after every kind of state change (DenseMap / HashMap::planner_view, the host brick cache).

What a planner call reads is redundant state: the dense store's observed / occupied bitmaps, the hash-block store's map-wide page
table, the bricks of the scalar queries and of the path calls' host route.  Every test has one shape:

    build a scene;  d0 = probe(m)        # tests/planner_probe.py; also warms the caches: bricks, page table, reach scratch
    a transition
    d1 = probe(m)                        # every planner call against its model on the map's own field, tolerance zero
    assert d1 differs from d0 in what the transition is about (or equals it, where that is the point)

The first probe is what lets a stale brick, page table or bitmap exist at all; the last assertion keeps a case from testing nothing.
Cases that name an UpdateESDF engine say from the returned statistics which engine served the step and, as
tests/test_gpu_updated_unit.py does, skip with the reason of path_notes -- after every comparison -- where it could not be the one
asked for."""
import numpy as np
import pytest

import planner_probe as pp
from planner_probe import HASH_SHIFT, RES, SHAPE, assert_differs, assert_equal, probe
from scenarios import D2_INF, P_DEFAULT, render_depth, yaw_pose
from test_gpu_cells import free
from test_gpu_updated_unit import check_engine, make_scene, pick

pytestmark = pytest.mark.gpu


def dense_for(engine, full=False):
    """the scene on a map pinned to `engine`: partly observed, or (full) make_scene's fully observed map with the scene's obstacles"""
    if not full:
        return pp.dense_scene(engine)
    m = make_scene(engine, SHAPE)
    pp.occupy(m, pp.OBSTACLES)
    m.UpdateESDF()
    return m


# ---- dense store -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["rounds", "levels", "masked", "auto"])
def test_dense_first_observations(hip_lib, engine):
    """a slab observed for the first time, 20 inserts, 20 deletes: k_fuse sets observed bits while the engine rewrites the field"""
    m = dense_for(engine)
    d0 = probe(m, "dense", what="before")
    pp.first_observations(m)
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (20, 20)
    d1 = probe(m, "dense", what=f"after first observations, {engine}")
    assert_differs(d0, d1, ("frontier", "n_traversable", "scalar"), "first observations")
    m.close()
    check_engine(st, engine, "first observations")


@pytest.mark.parametrize("engine", ["rounds", "levels", "envelope", "cells", "masked", "auto"])
def test_dense_delta_without_new_observations(hip_lib, engine):
    """the same delta, nothing observed for the first time: no engine may move a voxel between observed and never observed"""
    full = engine in ("envelope", "cells")          # (these two serve fully observed maps only)
    m = dense_for(engine, full)
    d0 = probe(m, "dense", what="before")
    pp.delta(m)
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (20, 20)
    d1 = probe(m, "dense", what=f"after a delta, {engine}")
    assert_differs(d0, d1, ("ray_class", "scalar"), "delta")
    if full:
        assert len(d0["frontier"]) == 0 and len(d1["frontier"]) == 0, "a fully observed map has no frontier"
    else:
        assert len(d0["frontier"]) > 1000 and np.array_equal(d0["frontier"][:, :3], d1["frontier"][:, :3])    # (no new observation)
    m.close()
    check_engine(st, engine, "delta without new observations")


INCREMENTAL_SHAPE = (64, 48, 72)     # 8 x 6 x 9 cells of 8^3 voxels: the smallest map on which ONE changed voxel may be served incrementally
                                     # (serve_by_transform: 180 cells per changed voxel must be at most half the map's; the scene has 6 x 5 x 9)


def test_dense_incremental_cell_transform(hip_lib):
    """one voxel inserted, then deleted, each served by the incremental cell transform: only dirty cells are rewritten"""
    reserved = {tuple(v) for v in np.concatenate([pp.OBSTACLES, pp.INSERTS]).tolist()}
    inside = lambda v: np.all(v < np.array(SHAPE), axis=1)   # noqa: E731
    more, = pick(INCREMENTAL_SHAPE, (400,), 43, lambda v: ~inside(v) | pp._free_for_obstacles(v) | (inside(v) & (v[:, 2] > pp.OBS_HI[2])))
    more = np.array([v for v in more.tolist() if tuple(v) not in reserved], np.int32)
    m = make_scene("cells", INCREMENTAL_SHAPE)
    pp.occupy(m, np.concatenate([pp.OBSTACLES, more]))
    st = m.UpdateESDF()
    assert st["cells"] == 1, st
    d0 = probe(m, "dense", what="before")
    one = np.array([pp.NEXT_TO_SCALAR], np.int32)
    pp.occupy(m, one)
    st = m.UpdateESDF()
    assert st["inserted"] == 1 and st["cells"] == 1 and st["nn_incremental"] == 1, st
    d1 = probe(m, "dense", what="after an incremental insert")
    assert d1["scalar"][0] == RES and d0["scalar"][0] > RES, (d0["scalar"][0], d1["scalar"][0])
    free(m, one)
    st = m.UpdateESDF()
    assert st["deleted"] == 1 and st["cells"] == 1 and st["nn_incremental"] == 1, st
    d2 = probe(m, "dense", what="after an incremental delete")
    assert d2["scalar"][0] == d0["scalar"][0] != d1["scalar"][0]
    assert_equal(d0, d2, "insert and delete of one voxel")
    m.close()


def test_dense_snapshot_restore(hip_lib):
    """restore brings the bitmaps back with the field: the digest equals the first one again, the comparisons pass on the restored map"""
    m = pp.dense_scene()
    d0 = probe(m, "dense", what="before")
    m.snapshot_save(0)
    pp.first_observations(m)
    m.UpdateESDF()
    d1 = probe(m, "dense", what="after the step")            # (bitmaps, bricks and scratch now hold the other state)
    assert_differs(d0, d1, pp.DIGEST_KEYS, "the step between save and restore")
    m.snapshot_restore(0)
    d2 = probe(m, "dense", what="restored")
    assert_equal(d0, d2, "restored")
    pp.delta(m)
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (20, 20)
    d3 = probe(m, "dense", what="a step after the restore")
    assert_differs(d2, d3, ("ray_class", "scalar"), "a step after the restore")
    m.close()


def other_dense_scene():
    """the scene's geometry, observed differently: another box, the scene's INSERTS as its obstacles"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, tuple((d - 0.5) * RES for d in SHAPE))
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((10, 8, 6), (40, 30, 60), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    pp.occupy(m, pp.INSERTS)
    m.UpdateESDF()
    return m


def test_dense_checkpoint_into_a_warm_map(hip_lib, tmp_path):
    """load into a map of the same geometry whose bitmaps, bricks and reach scratch are warm with other content"""
    a = pp.dense_scene()
    da = probe(a, "dense", what="the saved map")
    path = str(tmp_path / "scene.ckpt")
    a.save(path)
    a.close()
    b = other_dense_scene()
    d0 = probe(b, "dense", what="the other map")
    assert_differs(da, d0, pp.DIGEST_KEYS, "two different maps")
    b.load(path)
    d1 = probe(b, "dense", what="loaded")
    assert_differs(d0, d1, pp.DIGEST_KEYS, "load")
    assert_equal(da, d1, "loaded")
    pp.delta(b)
    b.UpdateESDF()
    assert_differs(d1, probe(b, "dense", what="a step after the load"), ("ray_class", "scalar"), "a step after the load")
    b.close()


def test_dense_local_map_reset(hip_lib):
    """UpdateOccupancy(False) under an update range resets what is observed outside the previous range (fuse_one), without any
    insert; then the original range again and one more step"""
    m = pp.dense_scene()
    d0 = probe(m, "dense", what="before")
    m.SetUpdateRange((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    m.SetUpdateRange((2.0, 1.5, 1.5), (4.0, 3.3, 3.8))          # the previous range is now the corner box
    m.SetOccupancyBox((22, 17, 17), (38, 31, 36), 0)           # holds SCALAR_VOX[6] = (24, 20, 33)
    before = m.download_field(("d2",))["d2"]
    m.UpdateOccupancy(False)
    after = m.download_field(("d2",))["d2"]
    reset = (before >= 0) & (before != D2_INF) & (after == D2_INF)
    assert int(reset.sum()) > 0, "no voxel was reset: the case is vacuous"
    m.UpdateESDF()
    d1 = probe(m, "dense", what="under the update range")
    assert_differs(d0, d1, ("scalar",), "local-map reset")
    m.SetOriginalRange()
    pp.delta(m)
    m.UpdateESDF()
    d2 = probe(m, "dense", what="the original range again")
    assert_differs(d1, d2, ("scalar",), "the step after the reset")
    m.close()


def test_dense_depth_frame(hip_lib):
    """one depth frame through RaycastDepth (the smallest image of tests/test_gpu_raycast_parity.py) into the partly observed scene"""
    m = pp.dense_scene()
    d0 = probe(m, "dense", what="before")
    intr = dict(fx=48.0, fy=48.0, cx=40.0, cy=30.0)
    T = yaw_pose(10.0, (2.05, 2.05, 3.65))
    depth = render_depth(T, rows=60, cols=80, intr=intr, room=((0.45, 0.45, 0.45), (4.35, 3.55, 5.25)))
    m.RaycastDepth(depth, intr["fx"], intr["fy"], intr["cx"], intr["cy"], T, T[:3, 3], 0.5, 5.0, (0.0, 0.0, 0.0), tuple(np.array(SHAPE) * RES), dedup=1)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    d1 = probe(m, "dense", what="after a depth frame")
    assert_differs(d0, d1, ("frontier", "n_traversable"), "depth frame")
    m.close()


def test_dense_update_occupancy_without_update_esdf(hip_lib):
    """occupancy and first observations change while the distances are stale: calls and models read the same stale field"""
    m = pp.dense_scene()
    d0 = probe(m, "dense", what="before")
    pp.first_observations(m)
    d1 = probe(m, "dense", what="before UpdateESDF")
    assert_differs(d0, d1, ("ray_class",), "UpdateOccupancy alone")
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (20, 20)
    assert_differs(d1, probe(m, "dense", what="after UpdateESDF"), ("scalar",), "UpdateESDF")
    m.close()


def test_dense_seed_and_relax(hip_lib):
    """esdf_seed and relax_pending until nothing is pending, the shard protocol's two halves of UpdateESDF"""
    m = pp.dense_scene()
    d0 = probe(m, "dense", what="before")
    pp.delta(m)
    st = m.esdf_seed()
    assert (st["inserted"], st["deleted"]) == (20, 20)
    for _ in range(64):
        pending, _ = m.relax_pending()
        if pending == 0:
            break
    else:
        pytest.fail("relax_pending never ran dry")
    d1 = probe(m, "dense", what="after seed and relax")
    assert_differs(d0, d1, ("ray_class", "scalar"), "seed and relax")
    m.close()


# ---- dense shard ---------------------------------------------------------------------------------------------------------------------
def test_shard_after_a_halo_exchange(hip_lib):
    """the two shards of tests/test_gpu_frontiers.py::test_shard_answers_for_its_own_array; shard B changes next to the face, the
    exchange rewrites A's ghost layer wholesale: planner_view(true) rebuilds A's observed bitmap from the field"""
    import fiesta_amd
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
    oa, ob = np.array(ia["local_origin"]), np.array(ib["local_origin"])
    da, db = np.array(ia["local_dims"]), np.array(ib["local_dims"])
    a_ghost = (np.array([16, 0, 0]), oa + da - 1)        # A's ghost layer beyond +x, global coordinates
    b_ghost = (ob, np.array([15, gg[1] - 1, gg[2] - 1])) # B's, below its owned box
    assert a_ghost[1][0] >= 16 and b_ghost[0][0] <= 15

    def sweep():
        changed = a.halo_apply(a_ghost[0] - oa, a_ghost[1] - oa, b.halo_pack(a_ghost[0] - ob, a_ghost[1] - ob))
        return changed + b.halo_apply(b_ghost[0] - ob, b_ghost[1] - ob, a.halo_pack(b_ghost[0] - oa, b_ghost[1] - oa))

    assert sweep() > 0
    d0 = probe(a, "shard", what="before")
    ghost = lambda d: d["frontier"][d["frontier"][:, 0] >= 15]   # noqa: E731  (rows at the face and in the ghost layer)
    # B: more free space beside the face and an obstacle on it; the occupancy transitions and the ghost cells travel as in sharded.py
    b.SetOccupancyBox((16, 3, 3), (21, 4, 14), 0)        # (beside the box B observed before: no voxel gets a second miss)
    b.SetOccupancyBox((16, 11, 3), (21, 12, 14), 0)
    for cycle in range(4):
        if cycle:
            b.SetOccupancy(np.array([[16, 7, 7]], np.int32), 1, want_ret=False)
        for sh in shards:
            sh.UpdateOccupancy(True)
        ent = np.concatenate([sh.export_transitions() for sh in shards])
        if len(ent):
            for sh in shards:
                sh.apply_transitions(ent)
    st = [sh.esdf_seed() for sh in shards]
    assert sum(s["inserted"] for s in st) == 1
    sweep()
    for _ in range(32):
        for sh in shards:
            sh.relax_pending()
        if sweep() == 0:
            break
    else:
        pytest.fail("the ghost exchange did not converge")
    d1 = probe(a, "shard", what="after the exchange")
    assert_differs(d0, d1, ("frontier", "ray_class"), "halo exchange")
    assert not np.array_equal(ghost(d0), ghost(d1)), "the frontier at the face did not change"
    assert d1["scalar"][0] < 10000.0                     # (17, 7, 7), a ghost cell: it names the obstacle B owns
    for sh in shards:
        sh.close()


# ---- hash-block store ------------------------------------------------------------------------------------------------------------------
NEW_BOX = ((45, 10, 10), (58, 24, 30))      # scene coordinates: x = 52 .. 58 lies in tiles that have no page in the scene


def hash_layout(reach_at_new_box=False):
    L = pp.Layout.scene(HASH_SHIFT)
    if reach_at_new_box:                    # the reach box across the scene's +x face and NEW_BOX
        L.reach_seed, L.reach_box = HASH_SHIFT + (40, 14, 14), (HASH_SHIFT + (30, 6, 6), HASH_SHIFT + (60, 30, 37))
    return L


def test_hash_pages_added(hip_lib):
    """free space and obstacles observed in a tile that has no page yet: the page table a planner call fetched before is too short"""
    m = pp.hash_scene()
    L = hash_layout(True)
    d0 = probe(m, "hash", L, "before")
    pages = m.grid_total_size_
    m.SetOccupancyBox(HASH_SHIFT + NEW_BOX[0], HASH_SHIFT + NEW_BOX[1], 0)
    m.UpdateOccupancy(True)
    pp.occupy(m, HASH_SHIFT + np.array([(54, 15, 15), (47, 20, 25)], np.int32))
    st = m.UpdateESDF()
    assert st["inserted"] == 2 and m.grid_total_size_ > pages
    d1 = probe(m, "hash", L, "after new pages")
    assert_differs(d0, d1, ("frontier", "n_traversable"), "pages added")
    assert (d1["frontier"][:, 0] >= HASH_SHIFT[0] + 52).any()       # frontier voxels on the new pages
    m.close()


def nearest_obstacle(v):
    d = ((pp.OBSTACLES.astype(np.int64) - np.array(v)) ** 2).sum(1)
    assert (d == d.min()).sum() == 1
    return pp.OBSTACLES[int(np.argmin(d))][None]


def test_hash_parked_and_back(hip_lib):
    """the window far away: every page is parked and answers through the page table alone; back again, a delete, UpdateESDF"""
    m = pp.hash_scene()
    L = hash_layout()
    d0 = probe(m, "hash", L, "before")
    pages = m.grid_total_size_
    m.hash_recentre(HASH_SHIFT + np.array([3000, -3000, 3000], np.int32))
    assert m.grid_total_size_ == pages
    assert_equal(d0, probe(m, "hash", L, "parked"), "parked")
    m.hash_recentre(HASH_SHIFT + np.array(SHAPE, np.int32) // 2)
    free(m, nearest_obstacle(pp.SCALAR_VOX[0]) + HASH_SHIFT)
    st = m.UpdateESDF()
    assert st["deleted"] == 1
    d1 = probe(m, "hash", L, "back, after a delete")
    assert_differs(d0, d1, ("scalar",), "delete after the window came back")
    assert d1["scalar"][0] > d0["scalar"][0]
    m.close()


def test_hash_window_parks_half_the_scene(hip_lib):
    """a window move that parks the lower half in x while the upper half stays resident: the probe's boxes span both"""
    m = pp.hash_scene()
    L = hash_layout()
    d0 = probe(m, "hash", L, "before")
    m.hash_recentre(HASH_SHIFT + np.array([24 + 512, 20, 36], np.int32))
    org = m.hash_window()[0]
    assert HASH_SHIFT[0] + 3 < org[0] <= HASH_SHIFT[0] + 44, org       # the window's low face cuts the scene
    assert org[1] < HASH_SHIFT[1] and org[2] < HASH_SHIFT[2]
    assert_equal(d0, probe(m, "hash", L, "half parked"), "half parked")
    m.close()


def test_hash_checkpoint_into_a_map_with_as_many_other_pages(hip_lib, tmp_path):
    """load into a hash-block map that holds the same number of pages for other tiles and whose page table is built: only the reset
    of the table's page count makes the next planner call rebuild it"""
    a = pp.hash_scene()
    L = hash_layout()
    da = probe(a, "hash", L, "the saved map")
    path = str(tmp_path / "scene.ckpt")
    a.save(path)
    pages = a.grid_total_size_
    a.close()
    b = pp.hash_scene(HASH_SHIFT + np.array((80, 64, 96), np.int32))     # whole tiles away: the same pages around other tiles
    assert b.grid_total_size_ == pages
    d0 = probe(b, "hash", L, "the other map")                            # (the layout of the saved scene: all unknown here)
    assert_differs(da, d0, pp.DIGEST_KEYS, "two different maps")
    b.load(path)
    assert b.grid_total_size_ == pages
    d1 = probe(b, "hash", L, "loaded")
    assert_differs(d0, d1, pp.DIGEST_KEYS, "load")
    assert_equal(da, d1, "loaded")
    b.close()


def test_hash_update_occupancy_without_update_esdf(hip_lib):
    m = pp.hash_scene()
    L = hash_layout()
    d0 = probe(m, "hash", L, "before")
    pp.first_observations(m, HASH_SHIFT)
    d1 = probe(m, "hash", L, "before UpdateESDF")
    assert_differs(d0, d1, ("ray_class",), "UpdateOccupancy alone")
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (20, 20)
    assert_differs(d1, probe(m, "hash", L, "after UpdateESDF"), ("scalar",), "UpdateESDF")
    m.close()
