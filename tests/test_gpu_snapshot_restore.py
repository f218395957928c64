"""fiesta_hip_snapshot_restore gives the map back, whole (dense store): the benchmark rewinds the map with it between timed
repetitions, so a restore that leaks any state -- the cell lists behind the incremental transform, the masked gate's counters, the
late-observation bitmap, the pending queues and counts, the update range, the distance bound of the rounds, the host brick cache --
makes the later repetitions time another update than the one reported.  Everything is compared for equality: a restored map
replays a step identically, continues like a twin that never took the detour, comes back from the middle of a frame, keeps four
independent slots, and answers scalar queries from the restored field."""
import numpy as np
import pytest

from test_gpu_cells import occupy
from test_gpu_updated_unit import SHAPE, ZCUT, check_engine, delta, make_scene, pick, served_by

pytestmark = pytest.mark.gpu

ENGINES = ("rounds", "levels", "envelope", "cells", "masked", "auto")
SLAB = 3      # the masked scene: planes ZCUT ... ZCUT + SLAB - 1 are observed late (while obstacles stand)


def build(engine, seed=21):
    """The scene every test here starts from: 300 obstacles on the fully observed map, distances up to date.  Engine masked: the
    partially observed map, and on top of the obstacles a slab of voxels that was first observed while they stood and has been
    reached by a wave since -- the late-observation bitmap still marks it, and the next rescan of the masked gate heals it.
    Returns (map, obstacles, free voxels to insert)."""
    keep = (lambda v: v[:, 2] < ZCUT) if engine == "masked" else None
    S, new = pick(SHAPE, (300, 120), seed, keep)
    m = make_scene(engine)
    occupy(m, S)
    m.UpdateESDF()
    if engine == "masked":
        m.SetOccupancyBox((0, 0, ZCUT), (SHAPE[0] - 1, SHAPE[1] - 1, ZCUT + SLAB - 1), 0)
        occupy(m, np.array([[10, 10, ZCUT + 1], [50, 30, ZCUT + 1], [30, 20, ZCUT + 1]], np.int32))
        st = m.UpdateESDF()
        assert st["inserted"] == 3 and "late_observation" in st["why"], st
        slab = m.download_field(("d2",))["d2"].reshape(SHAPE)[:, :, ZCUT:ZCUT + SLAB]
        assert np.all((slab >= 0) & (slab < 0x7FFFFFFF)), "the wave of the three inserts must have reached the whole slab"
    return m, S, new


def state(m):
    f = m.download_field(("d2", "occ", "logodds"))
    hit, miss = m.download_counts()
    return {"d2": f["d2"], "occ": f["occ"], "logodds": f["logodds"], "hit": hit, "miss": miss}


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, f"{what}: {k} differs"


def step(m, ins, gone, slot=None, pinned=True):
    """The benchmark's step: three SetOccupancy + UpdateOccupancy rounds of a mixed delta, then UpdateESDF.  Returns everything a
    repetition must reproduce and the statistics of the update.  pinned: the engine that served it is part of that (`auto` chooses
    by measured times: not reproducible, and on a fully observed map every engine gives the same field)."""
    fused = []
    for _ in range(3):
        if len(ins):
            m.SetOccupancy(ins, 1, want_ret=False)
        if len(gone):
            m.SetOccupancy(gone, 0, want_ret=False)
        fused.append((m.UpdateOccupancy(True), m.last_insert, m.last_delete))
    st = m.UpdateESDF()
    rec = state(m)
    rec.update(inserted=st["inserted"], deleted=st["deleted"], fused=fused, served=served_by(st) if pinned else None)
    if slot is not None:
        rec["updated"] = m.snapshot_count_updated(slot)
    return rec, st


@pytest.mark.parametrize("engine", ENGINES)
def test_replay_as_the_benchmark_does_it(hip_lib, engine):
    """snapshot, step, then three times restore + the same step: every repetition is the first one again (d2 rather than ids:
    which of several equidistant obstacles a voxel names is not deterministic after an update)"""
    m, S, new = build(engine)
    m.snapshot_save(1)
    first, st = step(m, new[:40], S[:40], slot=1, pinned=engine != "auto")
    assert (first["inserted"], first["deleted"]) == (40, 40) and first["updated"] > 0
    print(f"replay [{engine}]: served by {first['served']}, notes {st['why']}, nn_incremental {st['nn_incremental']}, updated {first['updated']}")
    for rep in range(3):
        m.snapshot_restore(1)
        again, st2 = step(m, new[:40], S[:40], slot=1, pinned=engine != "auto")
        same(first, again, f"repetition {rep + 1}")
        if engine == "cells":     # (the lists of the cell transform describe the field the restore replaced)
            assert st2["cells"] == 1 and st2["nn_incremental"] == 0, st2
    m.close()
    check_engine(st, engine, "replay")


def test_replay_of_an_incremental_cell_transform(hip_lib):
    """A one-voxel step is small enough for the cell transform to redo only the cells around it, from the lists of the update
    before (fiesta_hip_stats.nn_incremental).  After a restore those lists describe a field that is gone: the first update must
    start from scratch, the one after it may be incremental again -- and both give what a twin map gets."""
    m, S, new = build("cells")
    twin, _, _ = build("cells")
    m.snapshot_save(1)
    first, st = step(m, new[:1], S[:0], slot=1)
    assert st["cells"] == 1 and st["nn_incremental"] == 1, st      # (or this test would be about nothing)
    m.snapshot_restore(1)
    again, st2 = step(m, new[:1], S[:0], slot=1)
    assert st2["cells"] == 1 and st2["nn_incremental"] == 0, st2
    same(first, again, "the repetition")
    rt, _ = step(twin, new[:1], S[:0])
    again.pop("updated")
    same(again, rt, "against the twin")
    ra, sa = step(m, new[:0], S[:1])
    rb, sb = step(twin, new[:0], S[:1])
    assert sa["nn_incremental"] == sb["nn_incremental"] == 1 and (ra["inserted"], ra["deleted"]) == (0, 1)
    same(ra, rb, "one step later")
    m.close()
    twin.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_restored_map_continues_like_a_twin(hip_lib, engine):
    """a twin fed the same history without any snapshot call: after the replay both maps agree, and through two further steps --
    the last one delete-only (on the rounds its scan is bounded by the largest stored distance, which restore recomputes)"""
    a, S, new = build(engine)
    b, _, _ = build(engine)
    a.snapshot_save(1)
    step(a, new[:40], S[:40], pinned=engine != "auto")
    a.snapshot_restore(1)
    ra, st = step(a, new[:40], S[:40], pinned=engine != "auto")
    rb, _ = step(b, new[:40], S[:40], pinned=engine != "auto")
    same(ra, rb, "after the replay")
    ra, _ = step(a, new[40:80], S[40:80], pinned=engine != "auto")
    rb, _ = step(b, new[40:80], S[40:80], pinned=engine != "auto")
    assert (ra["inserted"], ra["deleted"]) == (40, 40)
    same(ra, rb, "one step later")
    ra, st3 = step(a, new[:0], S[80:140], pinned=engine != "auto")
    rb, _ = step(b, new[:0], S[80:140], pinned=engine != "auto")
    assert (ra["inserted"], ra["deleted"]) == (0, 60)
    same(ra, rb, "after the delete-only step")
    print(f"twin [{engine}]: replay served by {served_by(st)}, delete-only step by {served_by(st3)} {st3['why']}")
    a.close()
    b.close()
    check_engine(st, engine, "twin")


@pytest.mark.parametrize("engine", ["rounds", "cells"])
def test_mid_frame_snapshot_comes_back_whole(hip_lib, engine):
    """a snapshot taken with observations counted but not fused, both queues filled but not consumed and an update range in force:
    after a whole frame under another range the restore brings all of it back"""
    maps = []
    for _ in range(2):
        m, S, new = build(engine)
        for _ in range(3):
            m.SetOccupancy(new[:60], 1, want_ret=False)
            m.SetOccupancy(S[:30], 0, want_ret=False)
            m.UpdateOccupancy(True)
        m.SetOccupancy(new[60:], 1, want_ret=False)                 # counted, not fused
        m.SetUpdateRange((0.3, 0.2, 0.1), (2.5, 2.6, 2.7))          # (the range is part of the state: the getters show it)
        maps.append(m)
    a, b = maps
    a.snapshot_save(2)
    a.SetUpdateRange((1.0, 1.0, 1.0), (5.5, 4.0, 8.0))
    assert len(a.GetPointCloud(0, SHAPE[2])) != len(b.GetPointCloud(0, SHAPE[2]))
    a.UpdateOccupancy(True)
    a.UpdateESDF()
    a.SetOriginalRange()
    delta(a, new[:0], S[100:160])
    a.UpdateESDF()
    a.snapshot_restore(2)
    same(state(a), state(b), "right after the restore")
    pa, pb = a.GetPointCloud(0, SHAPE[2]), b.GetPointCloud(0, SHAPE[2])
    assert 0 < len(pa) < 300 and np.array_equal(pa[np.lexsort(pa.T)], pb[np.lexsort(pb.T)])
    for m in (a, b):
        m.SetOriginalRange()
        assert m.CheckUpdate()
    assert a.UpdateOccupancy(True) == b.UpdateOccupancy(True)
    assert (a.last_insert, a.last_delete) == (b.last_insert, b.last_delete)
    sa, sb = a.UpdateESDF(), b.UpdateESDF()
    assert (sa["inserted"], sa["deleted"]) == (sb["inserted"], sb["deleted"]) == (60, 30)
    assert served_by(sa) == served_by(sb)
    same(state(a), state(b), "after the frame was finished")
    for _ in range(2):                                               # the batch that was pending becomes obstacles
        for m in (a, b):
            m.SetOccupancy(new[60:], 1, want_ret=False)
            m.UpdateOccupancy(True)
    assert (a.last_insert, a.last_delete) == (b.last_insert, b.last_delete) == (60, 0)
    sa, sb = a.UpdateESDF(), b.UpdateESDF()
    same(state(a), state(b), "one frame later")
    a.close()
    b.close()


def test_four_slots_are_independent(hip_lib):
    """four different states in slots 0-3, restored in the order 2, 0, 3, 1: each comes back as it was downloaded when it was saved
    (ids included: no update runs in between)"""
    m, S, new = build("auto")

    def full():
        f = m.download_field()
        hit, miss = m.download_counts()
        return dict(f, hit=hit, miss=miss, cloud=(lambda p: p[np.lexsort(p.T)])(m.GetPointCloud(0, SHAPE[2])))

    saved = {}
    saved[0] = full()
    m.snapshot_save(0)
    delta(m, new[:40], S[:40])
    m.UpdateESDF()
    saved[1] = full()
    m.snapshot_save(1)
    delta(m, new[40:80], new[:0], cycles=2)              # mid-frame: two hits counted and fused, a third one pending
    m.SetOccupancy(new[40:80], 1, want_ret=False)
    m.SetUpdateRange((0.3, 0.2, 0.1), (2.5, 2.6, 2.7))
    saved[2] = full()
    m.snapshot_save(2)
    m.SetOriginalRange()
    delta(m, new[:0], S[40:120])
    m.UpdateESDF()
    m.SetUpdateRange((1.0, 1.0, 1.0), (5.5, 4.0, 8.0))
    saved[3] = full()
    m.snapshot_save(3)
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(saved[i]["logodds"], saved[j]["logodds"]), "the four states must differ"
    assert saved[2]["miss"].sum() > 0 and saved[0]["miss"].sum() == 0
    for slot in (2, 0, 3, 1):
        m.snapshot_restore(slot)
        same(full(), saved[slot], f"slot {slot}")
    m.close()


def test_scalar_queries_after_a_restore(hip_lib):
    """GetDistance on at most 8 voxels is answered from bricks of the field cached on the host: a restore must drop them"""
    m, S, new = build("auto")
    m.snapshot_save(0)
    q = new[:8]
    rng = np.random.RandomState(5)
    batch = np.concatenate([(rng.randint(0, 1 << 20, (40, 3)) % np.array(SHAPE)).astype(np.int32), q])
    before = m.GetDistance(batch)[-8:]
    assert np.all(before > 0)
    occupy(m, q)
    m.UpdateESDF()
    fetched = m.host_cache_fetches
    assert np.all(m.GetDistance(q) == 0.0)                      # the eight voxels are obstacles now; their bricks are cached
    assert m.host_cache_fetches > fetched
    m.snapshot_restore(0)
    got = m.GetDistance(q)
    assert np.array_equal(got, m.GetDistance(batch)[-8:]) and np.array_equal(got, before)
    assert np.array_equal(m.GetOccupancy(q), m.GetOccupancy(batch)[-8:]) and not m.GetOccupancy(q).any()
    m.close()


def test_bad_slots_are_refused_and_change_nothing(hip_lib):
    import fiesta_amd
    m, S, new = build("cells")
    m.snapshot_save(0)
    delta(m, new[:40], S[:40], cycles=2)                        # (pending state as well: counts and a queue)
    m.SetOccupancy(new[:40], 1, want_ret=False)
    f0, c0 = m.download_field(), m.download_counts()
    for slot in (-1, 4, 3):                                     # out of range twice, never saved
        with pytest.raises(fiesta_amd.FiestaHipError):
            m.snapshot_restore(slot)
        with pytest.raises(fiesta_amd.FiestaHipError):
            m.snapshot_count_updated(slot)
    for slot in (-1, 4):
        with pytest.raises(fiesta_amd.FiestaHipError):
            m.snapshot_save(slot)
    f1, c1 = m.download_field(), m.download_counts()
    assert all(np.array_equal(f0[k], f1[k]) for k in f0) and np.array_equal(c0[0], c1[0]) and np.array_equal(c0[1], c1[1])
    m.UpdateOccupancy(True)                                     # ... and the map goes on as if nothing had been asked
    st = m.UpdateESDF()
    assert (st["inserted"], st["deleted"]) == (40, 40)
    m.close()


def test_a_snapshot_does_not_hold_the_probability_parameters(hip_lib):
    """unlike a checkpoint file: SetParameters after a save survives the restore (include/fiesta_hip.h says so)"""
    other = (0.6, 0.4, 0.2, 0.8, 0.7)
    m, S, new = build("auto")
    twin, _, _ = build("auto")
    plain, _, _ = build("auto")
    m.snapshot_save(0)
    m.SetParameters(*other)
    m.snapshot_restore(0)
    twin.SetParameters(*other)
    for x in (m, twin, plain):
        x.SetOccupancy(new[:40], 1, want_ret=False)
        x.UpdateOccupancy(True)
    lm, lt, lp = (x.download_field(("logodds",))["logodds"] for x in (m, twin, plain))
    assert np.array_equal(lm, lt) and int((lm != lp).sum()) == 40
    for x in (m, twin, plain):
        x.close()
