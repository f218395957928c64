"""fiesta_hip_snapshot_count_updated -- the "updated voxel", numerator of every throughput figure -- against its definition in
numpy (tests/updated_model.py, checked on its own by tests/test_updated_model.py), on both stores.  Every case is

    before = download;  snapshot_save;  a step that ends with UpdateESDF;  after = download
    assert snapshot_count_updated == model(before, after)

with equality, no tolerance, and a second assertion that the case is not vacuous (what it is about did happen).  Dense cases run
once per UpdateESDF engine and say from the returned statistics which engine served the step; where the engine asked for could not
serve it and fiesta_hip_stats.path_notes says why, the count is still checked and the pair is then reported as skipped."""
import numpy as np
import pytest

from scenarios import D2_INF, P_DEFAULT
from test_gpu_cells import free, make_map, occupy
from updated_model import dense_count, dense_updated, hash_updated

pytestmark = pytest.mark.gpu

SHAPE = (61, 45, 83)        # no multiple of 8, 32 or 64
ZCUT = 55                   # the partially observed scene: planes z >= ZCUT (a third of the map) are never observed
TAIL_SHAPE = (129, 128, 128)
ONE_PASS = 8192 * 256       # voxels one trip of k_count_updated's grid-stride loop covers (grid_for(n, 256, 8192))
ENGINES = ("rounds", "levels", "envelope", "cells", "auto")
# what fiesta_hip_stats.path_notes may give as the reason why a pinned engine did not serve an update
GATE = {"partly_observed", "partial_window", "window_history", "first_wave_pending"}
EXPLAINS = {"rounds": set(), "levels": {"levels_gave_up"}, "envelope": GATE, "cells": GATE | {"cells_failed"},
            "masked": {"late_observation", "partial_window", "window_history", "first_wave_pending", "masked_gave_up"}, "auto": set()}


def served_by(st):
    if st["masked"]:
        return "masked"
    if st["bulk"]:
        return "cells" if st["cells"] else "envelope"
    return "levels" if st["levels"] else "rounds"


def check_engine(st, engine, case):
    """the engine asked for is the one that ran -- or path_notes explains why not (then: a skip, after everything else was asserted)"""
    got = served_by(st)
    print(f"{case} [{engine}]: served by {got}, notes {st['why']}")
    if engine == "auto" or got == engine:
        return
    why = sorted(set(st["why"]) & EXPLAINS[engine])
    assert why, f"{case}: asked for {engine}, served by {got}, and path_notes {st['why']} do not explain it"
    pytest.skip(f"{case}: {engine} is not eligible here ({', '.join(why)}); served by {got}, count checked")


def pick(shape, counts, seed, keep=None):
    """disjoint random voxel sets of the given sizes, all from the voxels where keep(v) holds"""
    v = np.stack(np.unravel_index(np.random.RandomState(seed).permutation(int(np.prod(shape))), shape), 1).astype(np.int32)
    if keep is not None:
        v = v[keep(v)]
    assert len(v) >= sum(counts)
    at = np.concatenate([[0], np.cumsum(counts)])
    return [np.ascontiguousarray(v[a:b]) for a, b in zip(at[:-1], at[1:])]


def make_scene(engine, shape=SHAPE):
    """the fully observed free map of `shape`; engine "masked": the partially observed one (z >= ZCUT never observed)"""
    if engine != "masked":
        return make_map(shape, engine)
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, tuple((s - 0.5) * 0.1 for s in shape), update_engine=engine)
    assert tuple(m.grid_size) == tuple(shape)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((0, 0, 0), (shape[0] - 1, shape[1] - 1, ZCUT - 1), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


def delta(m, ins, gone, cycles=6):
    """`ins` observed occupied and `gone` observed free until both have changed state (3 hits / at most 4 misses)"""
    for _ in range(cycles):
        if len(ins):
            m.SetOccupancy(ins, 1, want_ret=False)
        if len(gone):
            m.SetOccupancy(gone, 0, want_ret=False)
        m.UpdateOccupancy(True)


def count_and_model(m, before, shape=None, **kw):
    after = m.download_field(("d2", "coc", "occ"))
    got = m.snapshot_count_updated(0)
    upd, gone = dense_updated(before, after, shape or m.grid_size, **kw)
    want = int(upd.sum())
    print(f"  updated: device {got}, model {want} ({int(gone.sum())} by 'old obstacle gone' alone) of {len(upd)} voxels")
    assert got == want
    return got, after, upd, gone


def begin(m):
    before = m.download_field(("d2", "coc", "occ"))
    m.snapshot_save(0)
    return before


# ---- dense store --------------------------------------------------------------------------------------------------------------
DELTAS = {"insert": (40, 0), "delete": (0, 40), "mixed": (40, 40)}


@pytest.mark.parametrize("kind", list(DELTAS))
@pytest.mark.parametrize("engine", ENGINES + ("masked",))
def test_dense_delta(hip_lib, engine, kind):
    """40 inserts / 40 deletes / both on a 300-obstacle scatter (engine masked: on the partially observed map, inside its observed part)"""
    keep = (lambda v: v[:, 2] < ZCUT) if engine == "masked" else None
    S, new = pick(SHAPE, (300, 40), 11, keep)
    m = make_scene(engine)
    occupy(m, S)
    m.UpdateESDF()
    before = begin(m)
    ni, nd = DELTAS[kind]
    delta(m, new[:ni], S[:nd])
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (ni, nd)
    got, after, upd, _ = count_and_model(m, before)
    n = int(np.prod(SHAPE))
    assert 0 < got < n
    lin = lambda v: (v[:, 0].astype(np.int64) * SHAPE[1] + v[:, 1]) * SHAPE[2] + v[:, 2]   # noqa: E731
    assert upd[lin(new[:ni])].all() and upd[lin(S[:nd])].all()      # the changed obstacles themselves: d2 0 <-> finite
    m.close()
    check_engine(st, engine, f"{kind} delta")


@pytest.mark.parametrize("engine", ENGINES + ("masked",))
def test_dense_empty_step(hip_lib, engine):
    """observations that change no occupancy: the log-odds move, nothing is queued, nothing is updated"""
    keep = (lambda v: v[:, 2] < ZCUT) if engine == "masked" else None
    S, F = pick(SHAPE, (300, 500), 12, keep)
    m = make_scene(engine)
    occupy(m, S)
    m.UpdateESDF()
    lo_before = m.download_field(("logodds",))["logodds"]
    before = begin(m)
    m.SetOccupancy(S, 1, want_ret=False)
    m.SetOccupancy(F, 0, want_ret=False)
    assert m.CheckUpdate()
    m.UpdateOccupancy(True)
    assert (m.last_insert, m.last_delete) == (0, 0)
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (0, 0)
    got, after, _, _ = count_and_model(m, before)
    assert got == 0
    assert np.array_equal(after["occ"], before["occ"])
    assert int((m.download_field(("logodds",))["logodds"] != lo_before).sum()) >= 500   # (the step did fuse something)
    m.close()


A, B, PLANE_VOX = (30, 22, 36), (30, 22, 46), (30, 22, 41)      # two obstacles mirrored about the plane z = 41


@pytest.mark.parametrize("engine", ENGINES)
def test_dense_tie_winner_deleted(hip_lib, engine):
    """The voxels of the mirror plane are 5 voxels from both obstacles of a pair that stands alone (every other obstacle is more
    than 16 voxels from the pair's centre): the one they name is deleted, the other one gives them the same d2 -- updated only
    because the old closest obstacle is gone."""
    far = lambda v: ((v - np.array(PLANE_VOX)) ** 2).sum(1) > 16 ** 2   # noqa: E731
    S, = pick(SHAPE, (300,), 13, far)
    m = make_scene(engine)
    occupy(m, np.concatenate([S, np.array([A, B], np.int32)]))
    m.UpdateESDF()
    before = begin(m)
    at = (PLANE_VOX[0] * SHAPE[1] + PLANE_VOX[1]) * SHAPE[2] + PLANE_VOX[2]
    winner = tuple(int(c) for c in before["coc"][at])
    assert before["d2"][at] == 25 and winner in (A, B)
    free(m, np.array([winner], np.int32))
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (0, 1)
    got, after, upd, gone = count_and_model(m, before)
    assert after["d2"][at] == 25 and gone[at] and upd[at]
    assert int(gone.sum()) >= 1 and got > int((before["d2"] != after["d2"]).sum())
    m.close()
    check_engine(st, engine, "tie winner deleted")


@pytest.mark.parametrize("engine", ENGINES)
def test_dense_tie_repick(hip_lib, engine):
    """A lattice of obstacles with spacing 8: every voxel of a mid-plane has two or more closest obstacles.  One insert in a corner;
    a voxel elsewhere that names another of its equidistant obstacles afterwards is not updated (no engine has to re-pick)."""
    L = np.stack(np.meshgrid(*[np.arange(4, s, 8) for s in SHAPE], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    m = make_scene(engine)
    occupy(m, L)
    m.UpdateESDF()
    before = begin(m)
    occupy(m, np.array([[1, 1, 1]], np.int32))
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (1, 0)
    got, after, upd, gone = count_and_model(m, before)
    inspected = np.arange(len(upd)) >= 20 * SHAPE[1] * SHAPE[2]          # x >= 20: far from the insert
    repicked = (before["d2"] == after["d2"]) & np.any(before["coc"] != after["coc"], axis=1)
    print(f"  tie re-pick [{engine}]: {int(repicked.sum())} voxels name another equidistant obstacle, {int((repicked & inspected).sum())} of them at x >= 20")
    assert 0 < got < 200 and not upd[inspected].any() and not gone.any()
    m.close()
    check_engine(st, engine, "tie re-pick")


@pytest.mark.parametrize("engine", ENGINES)
def test_dense_first_observation(hip_lib, engine):
    """a third of the map is observed for the first time while obstacles stand: -1 -> D2_INF, or finite where a wave arrives
    (no masked transform here: by the time UpdateESDF runs, every voxel is observed)"""
    import fiesta_amd
    S, new = pick(SHAPE, (300, 5), 14, lambda v: v[:, 2] < ZCUT)
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, tuple((s - 0.5) * 0.1 for s in SHAPE), update_engine=engine)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((0, 0, 0), (SHAPE[0] - 1, SHAPE[1] - 1, ZCUT - 1), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    occupy(m, S)
    m.UpdateESDF()
    before = begin(m)
    third = SHAPE[0] * SHAPE[1] * (SHAPE[2] - ZCUT)
    assert int((before["d2"] == -1).sum()) == third
    m.SetOccupancyBox((0, 0, ZCUT), tuple(s - 1 for s in SHAPE), 0)
    occupy(m, new)
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (5, 0)
    got, after, upd, _ = count_and_model(m, before)
    first = before["d2"] == -1
    assert not (after["d2"] == -1).any() and upd[first].all() and got >= third
    print(f"  first observation [{engine}]: {int((after['d2'][first] == D2_INF).sum())} voxels -1 -> D2_INF, "
          f"{int((after['d2'][first] != D2_INF).sum())} -1 -> finite")
    m.close()
    check_engine(st, engine, "first observation")


def test_dense_local_map_fusion(hip_lib):
    """UpdateOccupancy(False) under an update range: a voxel observed outside the PREVIOUS range is reset (its distance reads "no
    obstacle", src/ESDFMap.cpp:256-259).  Finite -> D2_INF is an update like any other."""
    lo, hi = np.array((32, 22, 52)), np.array((55, 40, 78))          # the box observed under the second range
    outside = lambda v: ~np.all((v >= lo - 1) & (v <= hi + 1), axis=1)   # noqa: E731
    S, = pick(SHAPE, (300,), 15, outside)
    m = make_scene("rounds")
    occupy(m, S)
    m.UpdateESDF()
    before = begin(m)
    m.SetUpdateRange((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    m.SetUpdateRange((3.0, 2.0, 5.0), (6.0, 4.4, 8.2))               # the previous range is now the corner box
    m.SetOccupancyBox(tuple(lo), tuple(hi), 0)
    m.UpdateOccupancy(False)
    assert (m.last_insert, m.last_delete) == (0, 0)
    m.SetOriginalRange()
    occupy(m, np.array([[3, 3, 3], [8, 4, 6]], np.int32))            # far from the box: its wave ends long before it
    st = m.UpdateESDF()
    assert st["inserted"] == 2
    got, after, upd, _ = count_and_model(m, before)
    reset = (before["d2"] != D2_INF) & (before["d2"] >= 0) & (after["d2"] == D2_INF)
    box = int(np.prod(hi - lo + 1))
    print(f"  local-map fusion: {int(reset.sum())} of the box's {box} voxels read 'no obstacle' after the update")
    assert int(reset.sum()) > 0 and upd[reset].all() and got >= int(reset.sum())
    m.close()
    check_engine(st, "rounds", "local-map fusion")


@pytest.mark.parametrize("engine", ["cells", "rounds"])
def test_dense_grid_stride_tail(hip_lib, engine):
    """2 113 536 voxels: 16 384 more than one trip of the counting kernel's loop covers -- the plane x = 128 is counted on the
    second trip, by a fraction of the grid"""
    n = int(np.prod(TAIL_SHAPE))
    assert n - ONE_PASS == 128 * 128
    S, new = pick(TAIL_SHAPE, (1000, 40), 16)
    new[0] = (128, 64, 64)
    assert not np.any(np.all(S == new[0], axis=1)) and not np.any(np.all(new[1:] == new[0], axis=1))
    m = make_scene(engine, TAIL_SHAPE)
    occupy(m, S)
    m.UpdateESDF()
    before = begin(m)
    delta(m, new, S[:40])
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (40, 40)
    got, after, upd, _ = count_and_model(m, before)
    tail = int(upd[ONE_PASS:].sum())
    print(f"  grid-stride tail [{engine}]: {tail} of the {got} updated voxels lie past the first {ONE_PASS}")
    assert tail > 0 and 0 < got - tail
    m.close()
    check_engine(st, engine, "grid-stride tail")


def test_dense_shard_counts_its_owned_box(hip_lib):
    """One shard of a grid cut in two along x, its ghost layer filled by the exchange with its neighbour: obstacles appear and
    vanish on both sides of the face; the shard counts the updated voxels of the box it owns and none of its ghosts."""
    from fiesta_amd.sharded import ShardedESDFMap
    gs = (40, 24, 36)
    sm = ShardedESDFMap((0, 0, 0), 0.1, gs, 2, native=False)
    sm.SetParameters(*P_DEFAULT)
    sm.SetOriginalRange()
    sm.SetOccupancyBox((0, 0, 0), tuple(np.array(gs) - 1), 0)
    sm.UpdateOccupancy(True)
    sm.UpdateESDF()
    S, new = pick(gs, (80, 0), 17, lambda v: (v[:, 0] < 17) | (v[:, 0] > 22))
    near = np.array([[18, 10, 10], [19, 5, 30], [20, 18, 8], [21, 12, 20]], np.int32)   # the face lies between x = 19 and x = 20
    for _ in range(3):
        sm.SetOccupancy(np.concatenate([S, near[:2]]), 1)
        sm.UpdateOccupancy(True)
    sm.UpdateESDF()
    sh, info = sm.shards[0], sm.infos[0]
    dims, org = tuple(info["local_dims"]), np.array(info["local_origin"])
    owned = (np.array(info["owned_lo"]), np.array(info["owned_hi"]))
    assert dims[0] > owned[1][0] - owned[0][0] + 1, "the shard has no ghost layer"
    before = begin(sh)
    for _ in range(6):
        sm.SetOccupancy(near[2:], 1)             # two inserts beyond the face ...
        sm.SetOccupancy(near[:2], 0)             # ... two deletes on this side of it
        sm.SetOccupancy(S[:10], 0)
        sm.UpdateOccupancy(True)
    st = sm.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (2, 12)
    occupied = np.zeros(gs, bool)                # the global grid's occupancy: every shard's owned box
    for r, s in sm.shards.items():
        i = sm.infos[r]
        o, a, b = np.array(i["local_origin"]), np.array(i["owned_lo"]), np.array(i["owned_hi"])
        occ = s.download_field(("occ",))["occ"].reshape(tuple(i["local_dims"])) != 0
        occupied[a[0] + o[0]:b[0] + o[0] + 1, a[1] + o[1]:b[1] + o[1] + 1, a[2] + o[2]:b[2] + o[2] + 1] = occ[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1]
    assert int(occupied.sum()) == 80 - 10 + 2
    got, after, upd, _ = count_and_model(sh, before, dims, owned=owned, origin=org, occupied=occupied)
    everything = dense_count(before, after, dims, origin=org, occupied=occupied)
    print(f"  shard: {got} updated voxels in the owned box, {everything - got} more in the ghost layer")
    assert 0 < got < everything
    sm.close()


# ---- hash-block store ---------------------------------------------------------------------------------------------------------
SHIFT = np.array((-41, -23, -37), np.int32)      # negative coordinates, nothing aligned with the 16 x 16 x 32 pages (test_gpu_views.py)


def make_hash():
    import fiesta_amd
    m = fiesta_amd.ESDFMap((0.03, -0.02, 0.01), 0.1, reserve_size=1000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    return m


def hash_count_and_model(m, before, windowed=False):
    after = m.download_hash()
    got = m.snapshot_count_updated(0)
    window = m.hash_window()[0] if windowed else None
    upd, gone, inwin = hash_updated(before, after, window)
    print(f"  updated: device {got}, model {int(upd.sum())} ({int(gone.sum())} by 'old obstacle gone' alone) of {len(upd)} voxels, "
          f"{int((~inwin).sum())} of them outside the window")
    assert got == int(upd.sum())
    return got, after, upd, inwin


def hash_scene():
    m = make_hash()
    m.SetOccupancyBox(tuple(SHIFT), tuple(SHIFT + np.array(SHAPE) - 1), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    S, new = pick(SHAPE, (300, 40), 11)
    S, new = S + SHIFT, new + SHIFT
    occupy(m, S)
    m.UpdateESDF()
    return m, S, new


def test_hash_mixed_delta(hip_lib):
    """the dense mixed case on pages that exist, at negative coordinates"""
    m, S, new = hash_scene()
    before = m.download_hash()
    m.snapshot_save(0)
    delta(m, new, S[:40])
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (40, 40)
    got, after, upd, _ = hash_count_and_model(m, before)
    assert len(after["vox"]) == len(before["vox"]) and 0 < got < int(np.prod(SHAPE))
    m.close()


def test_hash_pages_appended_after_the_snapshot(hip_lib):
    """the step observes a fresh box next to the field: its pages did not exist when the snapshot was taken -- their voxels were
    never observed then, and the ones the box does not cover still are not"""
    m, S, new = hash_scene()
    before = m.download_hash()
    m.snapshot_save(0)
    lo = SHIFT + np.array((SHAPE[0], 3, 5))               # touches the field's +x face
    hi = lo + np.array((25, 20, 27))
    m.SetOccupancyBox(tuple(lo), tuple(hi), 0)
    edge = np.array([[SHIFT[0] + SHAPE[0] - 2, lo[1] + 6, lo[2] + 9]], np.int32)   # an insert whose wave runs into the new box
    assert not np.any(np.all(S == edge[0], axis=1))
    occupy(m, edge)
    st = m.UpdateESDF()
    assert st["inserted"] == 1
    got, after, upd, _ = hash_count_and_model(m, before)
    nb = len(before["vox"])
    assert len(after["vox"]) > nb
    key = lambda v: (v[:, 0].astype(np.int64) + 100000) * (1 << 40) + (v[:, 1].astype(np.int64) + 100000) * (1 << 20) + v[:, 2] + 100000  # noqa: E731
    fresh = ~np.isin(key(after["vox"]), key(before["vox"]))
    in_box = np.all((after["vox"] >= lo) & (after["vox"] <= hi), axis=1)
    assert int(fresh.sum()) == len(after["vox"]) - nb
    assert np.array_equal(upd[fresh], in_box[fresh]) and int((fresh & in_box).sum()) > 0    # observed now: counted
    assert np.all(after["d2"][fresh & ~in_box] == -1) and int((fresh & ~in_box).sum()) > 0  # still never observed: not counted
    assert int(upd[~fresh].sum()) > 0                                                        # ... and the old pages' share
    m.close()


ISLANDS = ((0, 0, 0), (900, 40, -20))     # 900 voxels apart: both fit into one window, neither can name an obstacle of the other
MIDDLE = (450, 20, -10)


def island(m, c, rng, n_obst, half=(12, 12, 8)):
    lo = np.array(c) - half
    m.SetOccupancyBox(tuple(lo), tuple(lo + 2 * np.array(half) - 1), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    obst = np.unique((lo + np.stack([rng.randint(0, 2 * h, n_obst) for h in half], -1)).astype(np.int32), axis=0)
    occupy(m, obst)
    m.UpdateESDF()
    box = lo + np.stack(np.unravel_index(rng.permutation(int(np.prod(half)) * 8), tuple(2 * h for h in half)), 1)
    spare = box[~np.isin(box @ np.array((1 << 40, 1 << 20, 1)), obst.astype(np.int64) @ np.array((1 << 40, 1 << 20, 1)))][:2].astype(np.int32)
    return lo, obst, spare      # (spare: two free voxels of the box)


def moved_window_scene():
    """Both islands resident, snapshot; a delta on the first island; then the window moves on so that the first island parks, and
    a delta on the second.  Returns the map, the snapshot's download and the islands."""
    m = make_hash()
    rng = np.random.RandomState(7)
    isl = [island(m, c, rng, 20) for c in ISLANDS]
    m.hash_recentre(MIDDLE)
    m.UpdateESDF()
    org = m.hash_window()[0]
    assert all(np.all(org <= lo) and np.all(lo + 24 <= org + 1024) for lo, _, _ in isl), "both islands must be resident"
    before = m.download_hash()
    m.snapshot_save(0)
    assert int((before["d2"] >= 0).sum()) == 2 * 24 * 24 * 16
    _, obst0, spare0 = isl[0]
    delta(m, spare0, obst0[:5])
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (2, 5)
    m.hash_recentre(ISLANDS[1])
    _, obst1, spare1 = isl[1]
    delta(m, spare1, obst1[:5])
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (2, 5)
    return m, before, isl


def test_hash_window_moved_after_the_snapshot(hip_lib):
    """a page that left the window is no longer part of the map: what changed on it since the snapshot is not counted"""
    m, before, isl = moved_window_scene()
    org = m.hash_window()[0]
    assert not np.all((org <= isl[0][0]) & (isl[0][0] + 24 <= org + 1024)), "the first island must be parked"
    got, after, upd, inwin = hash_count_and_model(m, before, windowed=True)
    everywhere, _, _ = hash_updated(before, after)
    removed = int(everywhere.sum()) - got
    print(f"  window moved: the filter removed {removed} changed voxels of the parked island")
    assert got > 0 and removed > 0 and int((~inwin).sum()) >= 24 * 24 * 16
    m.close()


def test_hash_window_moved_back(hip_lib):
    """... and when the window comes back the parked island rejoins, with everything that changed on it since the snapshot"""
    m, before, isl = moved_window_scene()
    parked = m.snapshot_count_updated(0)
    m.hash_recentre(MIDDLE)
    m.UpdateESDF()
    got, after, upd, inwin = hash_count_and_model(m, before, windowed=True)
    observed = after["d2"] >= 0
    assert inwin[observed].all() and got > parked > 0
    assert got == int(hash_updated(before, after)[0].sum())      # nothing is outside the window now
    m.close()
