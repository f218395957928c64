"""GPU: the INCREMENTAL cell transform (nn_kernels.hpp: k_nn_mark / k_nn_lists_dirty / k_nn_fill_dirty) -- on a fully observed map
whose last UpdateESDF was a cell transform, a small delta redoes only the cells whose search window holds a changed voxel
(the reference's own cost follows the delta's Voronoi cells, src/ESDFMap.cpp:273-337).  Exactness is the transform's: squared
distances equal to the reference's on every voxel, whatever mix of incremental and full updates produced the field."""
import numpy as np
import pytest
from scipy import ndimage

from scenarios import P_DEFAULT, Both, all_voxels, assert_exact, compare_dense

pytestmark = pytest.mark.gpu


def _both(oracle_libs, kind, n, engine="cells"):
    import fiesta_amd
    res = 0.1
    gpu = fiesta_amd.ESDFMap((0, 0, 0), res, ((n - 0.5) * res,) * 3, update_engine=engine)
    cpu = oracle_libs.OracleMap((0, 0, 0), res, ((n - 0.5) * res,) * 3, kind=kind)
    b = Both(gpu, cpu)
    b.params()
    b.observe(all_voxels(n), 0)
    b.fuse()
    b.esdf()
    return b


def test_incremental_and_full_updates_interleaved_match_the_reference(hip_lib, oracle_libs, best_oracle_kind):
    n = 160
    b = _both(oracle_libs, best_oracle_kind, n)
    rng = np.random.RandomState(7)
    V = all_voxels(n)
    live = V[rng.choice(len(V), 400, replace=False)]
    b.make_occupied(live)
    sg, _ = b.esdf()
    assert sg["cells"] == 1 and sg["nn_incremental"] == 0, sg
    assert_exact(compare_dense(b.gpu, b.cpu))
    seen_inc = seen_full = 0
    for step in range(10):
        k = [2, 5, 1, 40, 3, 7, 1, 200, 4, 2][step]   # small deltas run incrementally, the large ones dirty too much and run in full
        new = V[rng.choice(len(V), k, replace=False)]
        old, live = live[:k], np.concatenate([live[k:], new])
        b.mixed(new, old)
        sg, _ = b.esdf()
        assert sg["cells"] == 1 and sg["nn_failed"] == 0, sg
        seen_inc += int(sg["nn_incremental"])
        seen_full += int(not sg["nn_incremental"])
        if sg["nn_incremental"]:
            assert 0 < sg["nn_dirty_cells"] < (n // 8) ** 3, sg
        assert_exact(compare_dense(b.gpu, b.cpu))
    assert seen_inc >= 6 and seen_full >= 1, (seen_inc, seen_full)
    b.gpu.close()
    b.cpu.close()


def test_incremental_delete_of_the_only_obstacle_in_reach_falls_back(hip_lib, oracle_libs, best_oracle_kind):
    """Deleting obstacles until some cell finds nothing within its widest window: the incremental attempt fails (a cell without a
    list), the same call is served in full -- by the envelope passes, since the cell transform cannot serve such a scene either."""
    n = 128
    b = _both(oracle_libs, best_oracle_kind, n)
    rng = np.random.RandomState(3)
    V = all_voxels(n)
    S = V[rng.choice(len(V), 500, replace=False)]
    b.make_occupied(S)
    sg, _ = b.esdf()
    assert sg["cells"] == 1, sg
    far = S[(S[:, 0] > 40)]          # free one side of the map completely
    for s in range(0, len(far), 60):
        b.make_free(far[s:s + 60])
        sg, _ = b.esdf()
        assert sg["bulk"] == 1, sg
        assert_exact(compare_dense(b.gpu, b.cpu))
    b.gpu.close()
    b.cpu.close()


def test_other_engines_invalidate_the_lists(hip_lib, oracle_libs, best_oracle_kind):
    n = 128
    b = _both(oracle_libs, best_oracle_kind, n, engine="auto")
    rng = np.random.RandomState(9)
    V = all_voxels(n)
    S = V[rng.choice(len(V), 800, replace=False)]
    b.make_occupied(S)
    sg, _ = b.esdf()
    assert sg["cells"] == 1, sg
    b.gpu.set_update_engine("rounds")
    b.mixed(V[rng.choice(len(V), 3, replace=False)], S[:3])
    sg, _ = b.esdf()
    assert sg["bulk"] == 0, sg
    b.gpu.set_update_engine("cells")
    b.mixed(V[rng.choice(len(V), 3, replace=False)], S[3:6])
    sg, _ = b.esdf()
    assert sg["cells"] == 1 and sg["nn_incremental"] == 0, sg   # (the rounds changed the field behind the lists' back)
    assert_exact(compare_dense(b.gpu, b.cpu))
    b.mixed(V[rng.choice(len(V), 3, replace=False)], S[6:9])
    b.gpu.snapshot_save(0)
    sg, _ = b.esdf()
    assert sg["cells"] == 1 and sg["nn_incremental"] == 1, sg
    assert_exact(compare_dense(b.gpu, b.cpu))
    b.gpu.snapshot_restore(0)
    sg = b.gpu.UpdateESDF()
    assert sg["cells"] == 1 and sg["nn_incremental"] == 0, sg   # (a restored map: whatever the lists describe, it is not this field)
    assert_exact(compare_dense(b.gpu, b.cpu))
    b.gpu.close()
    b.cpu.close()


@pytest.mark.parametrize("shape,seed", [((161, 45, 83), 1), ((72, 200, 40), 2), ((130, 66, 97), 3)])
def test_incremental_updates_on_ragged_maps_are_exact(hip_lib, shape, seed):
    """grids that are no multiple of the cell edge: a run of small deltas, each served incrementally where the lists allow, every
    field the exact transform of what is occupied (scipy)"""
    from test_gpu_cells import check_exact, free, make_map, occupy
    rng = np.random.RandomState(seed)
    m = make_map(shape, "cells")
    V = all_voxels(shape)
    live = V[rng.choice(len(V), len(V) // 2500, replace=False)]
    occupy(m, live)
    st = m.UpdateESDF()
    assert st["cells"] == 1, st
    check_exact(m, shape)
    inc = 0
    for step in range(6):
        k = 1   # (one insert + one delete: these maps have ~10^3 cells, a voxel dirties ~10^2 of them)
        new = V[rng.choice(len(V), k, replace=False)]
        occupy(m, new)
        free(m, live[:k])
        live = np.concatenate([live[k:], new])
        st = m.UpdateESDF()
        assert st["bulk"] == 1, st
        inc += int(st["nn_incremental"])
        check_exact(m, shape)
    assert inc >= 3, inc
    m.close()


def test_incremental_update_with_many_dirty_cells_is_exact(hip_lib):
    """a map large enough for a three-digit delta to stay incremental: tens of thousands of dirty cells, k_nn_mark's work-groups
    flush their LDS queues more than once (one atomic on the list's cursor per flush)"""
    from test_gpu_cells import check_exact, free, make_map, occupy
    shape = (320, 320, 320)
    rng = np.random.RandomState(11)
    m = make_map(shape, "cells")
    n = shape[0] * shape[1] * shape[2]
    pick = lambda k: np.stack(np.unravel_index(rng.choice(n, k, replace=False), shape), 1).astype(np.int32)  # noqa: E731
    live = pick(n // 2700)
    occupy(m, live)
    st = m.UpdateESDF()
    assert st["cells"] == 1, st
    for step in range(2):
        k = 60
        new = pick(k)
        occupy(m, new)
        free(m, live[:k])
        live = np.concatenate([live[k:], new])
        st = m.UpdateESDF()
        assert st["bulk"] == 1 and st["nn_incremental"] == 1, st
        assert st["nn_dirty_cells"] > 5000, st
        check_exact(m, shape)
    m.close()


# ---- cells without a list whose winners lie beyond every window --------------------------------------------------------------------
# A cell that finds no site within its widest window (nn_core.hpp: kWhySparse) is served against every site (k_nn_close), and its
# record says kKmax = 7 cells of reach -- but its winners lie farther.  A change out there does not dirty it (k_nn_mark), so the
# lists of such a transform must not serve an incremental update: the next update runs the full transform.  The scene is
# test_gpu_cells.py's: no obstacle with every coordinate below 70, so the cell (0, 0, 0) and its neighbours have no list.
RES = 0.1
BOX = 70


def _corner_sites():
    S = np.random.RandomState(31).randint(0, 128, (700, 3)).astype(np.int32)
    return S[~np.all(S < BOX, axis=1)]


def _corner_map(engine="cells"):
    """128^3, every voxel observed free, the corner scene inserted and transformed (engine None: the library's default)"""
    from test_gpu_cells import make_map, occupy
    shape = (128, 128, 128)
    m = make_map(shape, engine)
    occupy(m, _corner_sites())
    st = m.UpdateESDF()
    assert st["bulk"] == 1 and st["cells"] == 1 and st["nn_incremental"] == 0 and st["nn_failed"] == 0, st
    assert st["nn_brute_cells"] > 0, st
    return m, shape


def _occupancy(m, shape):
    return m.download_field(("occ",))["occ"].reshape(shape)


def _winner(occ, v):
    """the occupied voxel nearest to v (scipy's exact feature transform)"""
    idx = ndimage.distance_transform_edt(occ == 0, return_distances=False, return_indices=True)
    return np.array([int(idx[k][tuple(v)]) for k in range(3)], np.int32)


def _apply(m, ins=(), dele=()):
    """one delta: inserts hit three times, deletes missed six times (test_gpu_cells.py: occupy / free), one UpdateOccupancy each"""
    ins, dele = np.asarray(ins, np.int32).reshape(-1, 3), np.asarray(dele, np.int32).reshape(-1, 3)
    for c in range(6):
        if c < 3 and len(ins):
            m.SetOccupancy(ins, 1, want_ret=False)
        if len(dele):
            m.SetOccupancy(dele, 0, want_ret=False)
        m.UpdateOccupancy(True)
    return m.UpdateESDF()


def _full_after_brute(st):
    """the update that follows a transform with cells served against every site: the cell transform, in full"""
    assert st["bulk"] == 1 and st["cells"] == 1 and st["nn_failed"] == 0, st
    assert st["nn_incremental"] == 0, ("the lists of a transform with cells served against every site were trusted", st)


def _corner_distances(m, shape):
    """GetDistance at voxels of the corner cell against the exact distance: what a planner reads"""
    occ = _occupancy(m, shape)
    d = ndimage.distance_transform_edt(occ == 0)
    V = np.array([(x, y, z) for x in (0, 3, 7) for y in (0, 5) for z in (0, 6)] + [(12, 9, 2), (20, 30, 40)], np.int32)
    got = np.asarray(m.GetDistance(V), np.float64)
    want = d[tuple(V.T)] * RES
    assert np.allclose(got, want, rtol=1e-6, atol=0), np.stack([got, want], 1)


def test_deleting_the_far_winner_of_a_cell_without_a_list(hip_lib):
    """the winner of voxel (0, 0, 0) lies 8 cells away or more; freeing it in a one-voxel update must move every voxel that held
    it to the next nearest obstacle -- the corner cell is not within 7 cells of the change"""
    from test_gpu_cells import check_exact
    m, shape = _corner_map()
    check_exact(m, shape)
    w = _winner(_occupancy(m, shape), (0, 0, 0))
    assert (w // 8).max() > 7, w   # (beyond the widest reach a record keeps: kKmax = 7 cells)
    st = _apply(m, dele=[w])
    assert st["deleted"] == 1 and st["inserted"] == 0, st
    check_exact(m, shape)             # (first: a library that trusts the corner cell's reach fails here, with the count of stale voxels)
    _corner_distances(m, shape)
    _full_after_brute(st)
    m.close()


def test_inserting_a_nearer_far_site_of_a_cell_without_a_list(hip_lib):
    """(66, 0, 0) lies in cell (8, 0, 0) -- beyond the corner cell's recorded reach -- and is nearer to voxel (0, 0, 0) than its
    current winner (the scene has no obstacle with every coordinate below 70)"""
    from test_gpu_cells import check_exact
    m, shape = _corner_map()
    occ = _occupancy(m, shape)
    p = np.array([66, 0, 0], np.int32)
    w = _winner(occ, (0, 0, 0))
    assert occ[tuple(p)] == 0 and (p // 8).max() >= 8 and int((p ** 2).sum()) < int((w.astype(np.int64) ** 2).sum()), (p, w)
    st = _apply(m, ins=[p])
    assert st["inserted"] == 1 and st["deleted"] == 0, st
    check_exact(m, shape)
    _corner_distances(m, shape)
    _full_after_brute(st)
    m.close()


def test_far_winner_updates_mixed_and_in_a_run(hip_lib):
    """both in one update (free the corner's winner, insert (66, 0, 0)), then ten updates that alternate a far-winner change
    (free the winner of a random voxel of the empty corner / insert a site in it) with a small random delta elsewhere"""
    from test_gpu_cells import check_exact
    m, shape = _corner_map()
    rng = np.random.RandomState(17)
    occ = _occupancy(m, shape)
    w = _winner(occ, (0, 0, 0))
    st = _apply(m, ins=[(66, 0, 0)], dele=[w])
    assert st["inserted"] == 1 and st["deleted"] == 1, st
    check_exact(m, shape)
    _full_after_brute(st)
    prev_brute = st["nn_brute_cells"]
    for step in range(10):
        occ = _occupancy(m, shape)
        if step % 2 == 0:
            if step % 4 == 0:
                v = rng.randint(0, BOX, 3)
                st = _apply(m, dele=[_winner(occ, v)])
            else:
                free_in_box = np.argwhere(occ[:BOX, :BOX, :BOX] == 0)
                st = _apply(m, ins=free_in_box[rng.randint(len(free_in_box))][None])
        else:
            outside = np.argwhere(occ[BOX:, :, :] == 1) + (BOX, 0, 0)
            free_out = rng.randint(0, 128, (2, 3))
            free_out[:, 0] = rng.randint(BOX, 128, 2)
            free_out = free_out[occ[tuple(free_out.T)] == 0]
            st = _apply(m, ins=free_out, dele=outside[rng.choice(len(outside), 2, replace=False)])
        check_exact(m, shape)
        assert st["bulk"] == 1 and st["cells"] == 1 and st["nn_failed"] == 0, (step, st)
        if prev_brute > 0:
            _full_after_brute(st)
        prev_brute = st["nn_brute_cells"]
    m.close()


def test_far_winner_delete_on_the_default_engine(hip_lib):
    """a map made without update_engine: the library's own choice serves the one-voxel update by the cell transform, which
    must not be the incremental one"""
    from test_gpu_cells import check_exact
    m, shape = _corner_map(engine=None)
    w = _winner(_occupancy(m, shape), (0, 0, 0))
    st = _apply(m, dele=[w])
    check_exact(m, shape)
    _corner_distances(m, shape)
    assert st["cells"] == 1, st
    _full_after_brute(st)
    m.close()


# ---- a seeded sequence over scene families --------------------------------------------------------------------------------------
# (shape, empty box lo / hi, solid block lo or None).  plain: no empty region (incremental serves nearly every update); the
# boxes: far winners for the cells inside -- the corner one leaves cells without any site in reach (kWhySparse); a ragged grid
# with an empty slab; a solid block next to the empty corner: cells with too many survivors (kWhyDense) beside sparse ones
# (45 cells without a list at first: the 64 a 128^3 map serves one by one hold them).
# The kinds of delta take turns: inserts into the empty region come late, as they give the sparse cells a site in reach.
KINDS = ["far-winner", "random", "far-winner", "drain", "far-winner", "random", "far-winner", "drain", "insert-empty", "far-winner",
         "random", "far-winner"]
FAMILIES = {
    "plain": ((128, 128, 128), None, None, None),
    "corner-box": ((128, 128, 128), (0, 0, 0), (62, 62, 62), None),
    "face-box": ((128, 128, 128), (0, 24, 24), (64, 104, 104), None),
    "centre-box": ((128, 128, 128), (24, 24, 24), (104, 104, 104), None),
    "ragged-slab": ((130, 97, 121), (30, 0, 0), (100, 97, 121), None),
    "block-and-corner": ((128, 128, 128), (0, 0, 0), (62, 62, 62), (90, 90, 90)),
}
SPARSE_ONLY = ("corner-box", "face-box", "centre-box", "ragged-slab")  # (every cell served one by one is a sparse one)


def _family_scene(fam):
    shape, lo, hi, blk = FAMILIES[fam]
    rng = np.random.RandomState(sorted(FAMILIES).index(fam) + 101)
    occ = np.zeros(shape, np.uint8)
    S = (rng.rand(int(700 * np.prod(shape) / 128 ** 3), 3) * shape).astype(np.int64)
    occ[tuple(S.T)] = 1
    box = None
    if lo is not None:
        box = np.zeros(shape, bool)
        box[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        occ[box] = 0
    block = None
    if blk is not None:
        block = np.zeros(shape, bool)
        block[blk[0]:blk[0] + 7, blk[1]:blk[1] + 7, blk[2]:blk[2] + 7] = True
        occ[block] = 1
    return shape, occ, box, block


def _draw_delta(rng, occ, box, block, kmax, kind):
    """1 ... kmax voxels (inserts, deletes, kind): free the winners of random voxels of the empty region / insert inside it /
    random inserts and deletes / drain the solid block (a kind the scene has no region for: random)"""
    if (kind in ("far-winner", "insert-empty") and box is None) or (kind == "drain" and (block is None or not (occ[block] == 1).any())):
        kind = "random"
    k = rng.randint(1, kmax + 1)
    ins, dele = np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    if kind == "far-winner":
        sites = np.argwhere(occ == 1)
        inbox = np.argwhere(box)
        V = inbox[rng.choice(len(inbox), k, replace=False)]
        dele = np.unique(sites[((sites[None, :, :] - V[:, None, :]) ** 2).sum(-1).argmin(1)], axis=0)
    elif kind == "insert-empty":
        cand = np.argwhere(box & (occ == 0))
        ins = cand[rng.choice(len(cand), k, replace=False)]
    elif kind == "drain":
        cand = np.argwhere(block & (occ == 1))
        dele = cand[rng.choice(len(cand), min(k, len(cand)), replace=False)]
    else:
        sites, shape = np.argwhere(occ == 1), np.array(occ.shape)
        dele = sites[rng.choice(len(sites), k // 2, replace=False)]
        ins = (rng.rand(k - k // 2, 3) * shape).astype(np.int64)
        ins = np.unique(ins[occ[tuple(ins.T)] == 0], axis=0)
    return ins, dele, kind


def test_seeded_sequences_over_scene_families(hip_lib):
    """about a dozen small updates per family, each within the incremental transform's limit ((ins + del) x 180 <= cells / 2),
    drawn from the deltas that test the recorded reach; the exact transform after every one.  At least a third of all updates
    run incrementally; in the families whose cells without a list are all sparse ones, an update that follows a transform
    with such cells never does"""
    from test_gpu_cells import check_exact, make_map, occupy
    total = inc = 0
    for fam in FAMILIES:
        shape, occ, box, block = _family_scene(fam)
        rng = np.random.RandomState(sorted(FAMILIES).index(fam) + 7)
        kmax = min(11, int(np.prod([(s + 7) // 8 for s in shape])) // 2 // 180)
        m = make_map(shape, "cells")
        occupy(m, np.argwhere(occ == 1))
        st = m.UpdateESDF()
        assert st["bulk"] == 1 and st["cells"] == 1 and st["nn_incremental"] == 0 and st["nn_failed"] == 0, (fam, st)
        check_exact(m, shape)
        prev_brute = st["nn_brute_cells"]
        for step in range(12):
            occ = _occupancy(m, shape)
            ins, dele, kind = _draw_delta(rng, occ, box, block, kmax, KINDS[step])
            st = _apply(m, ins, dele)
            assert (st["inserted"], st["deleted"]) == (len(ins), len(dele)), (fam, step, kind, st)
            check_exact(m, shape)
            # (the cell transform serves the update -- unless far-winner deletes left more cells without a list than it serves one
            #  by one, 64 here: then it reports them and the envelope passes serve the update)
            assert st["bulk"] == 1 and (st["cells"] == 1) == (st["nn_failed"] == 0), (fam, step, kind, st)
            if fam in SPARSE_ONLY and prev_brute > 0:
                assert st["nn_incremental"] == 0, (fam, step, kind, st)
            total += 1
            inc += int(st["nn_incremental"])
            prev_brute = st["nn_brute_cells"]
        m.close()
    assert 3 * inc >= total, (inc, total)


def test_tracked_distance_bound_through_incremental_updates(hip_lib):
    """a map that tracks the largest stored distance (one ray-cast frame switches it on): far-winner changes on the corner scene,
    incremental updates that grow distances (the bound of the cells they redo is max-merged into the map's), then a small
    delete on the frontier rounds, whose delete scan is bounded by it -- every field exact"""
    from test_gpu_cells import check_exact, make_map, occupy
    shape = (128, 128, 128)
    m = make_map(shape, "cells")
    T = np.eye(4)
    T[:3, 3] = (6.4, 6.4, 6.4)
    m.RaycastFrame(np.array([[0.3, 0.0, 0.0]], np.float32), T, (6.4, 6.4, 6.4), 0.05, 5.0, (-100.0,) * 3, (100.0,) * 3)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, _corner_sites())
    st = m.UpdateESDF()
    assert st["cells"] == 1 and st["nn_brute_cells"] > 0, st
    check_exact(m, shape)
    st = _apply(m, dele=[_winner(_occupancy(m, shape), (0, 0, 0))])   # far winner: in full
    check_exact(m, shape)
    _full_after_brute(st)
    A, B = (40, 40, 40), (24, 20, 28)
    st = _apply(m, ins=[A, B])            # sites in the corner: its cells get lists again
    check_exact(m, shape)
    _full_after_brute(st)
    rng = np.random.RandomState(2)
    inc = 0
    for step in range(4):
        occ = _occupancy(m, shape)
        if step == 1:
            st = _apply(m, dele=[B])      # the corner's distances grow (their winner is A now)
        else:
            sites = np.argwhere(occ == 1)
            sites = sites[~np.all(sites < BOX, axis=1)]
            st = _apply(m, dele=sites[rng.choice(len(sites), 2, replace=False)])
        check_exact(m, shape)
        assert st["cells"] == 1 and st["nn_failed"] == 0, (step, st)
        inc += int(st["nn_incremental"])
    assert inc >= 1, inc
    m.set_update_engine("rounds")
    occ = _occupancy(m, shape)
    sites = np.argwhere(occ == 1)
    st = _apply(m, dele=np.concatenate([[A], sites[~np.all(sites < BOX, axis=1)][:2]]))
    assert st["bulk"] == 0, st
    check_exact(m, shape)
    m.close()
