"""tests/updated_model.py on hand-made 4 x 4 x 4 fields, one per clause of the definition of an "updated voxel"
(include/fiesta_hip.h, above fiesta_hip_snapshot_count_updated): the numpy model that tests/test_gpu_updated_unit.py holds the
device counts to has to be right on its own."""
import numpy as np

from updated_model import D2_INF, UNDEFINED, dense_count, dense_updated, hash_count, hash_updated

SHAPE = (4, 4, 4)
N = 64


def lin(x, y, z):
    return (x * 4 + y) * 4 + z


def field(obstacles, observed=None, names=None):
    """the exact field of `obstacles` on the 4^3 grid: every observed voxel names its nearest obstacle (the first of equals, or
    names[voxel] where given); `observed`: a boolean (64,) array, default everything"""
    v = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d2 = np.full(N, D2_INF, np.int32)
    coc = np.full((N, 3), UNDEFINED, np.int32)
    occ = np.zeros(N, np.uint8)
    for o in obstacles:
        occ[lin(*o)] = 1
        d = ((v - np.array(o)) ** 2).sum(-1)
        better = d < d2
        d2[better], coc[better] = d[better], o
    for vox, o in (names or {}).items():
        assert ((np.array(vox) - np.array(o)) ** 2).sum() == d2[lin(*vox)] and occ[lin(*o)]
        coc[lin(*vox)] = o
    if observed is not None:
        d2[~observed], coc[~observed] = -1, UNDEFINED
    return {"d2": d2, "coc": coc, "occ": occ}


def as_hash(f, shift=(0, 0, 0), order=None):
    """the same field as download_hash shows it: one row per voxel, coordinates moved by `shift`, rows in `order`"""
    v = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.array(shift)
    coc = np.where(f["coc"] == UNDEFINED, UNDEFINED, f["coc"] + np.array(shift))
    o = np.arange(N) if order is None else order
    return {"vox": v[o].astype(np.int32), "d2": f["d2"][o], "coc": coc[o].astype(np.int32), "occ": f["occ"][o]}


def test_nothing_changed_counts_nothing():
    f = field([(1, 1, 1), (3, 0, 2)])
    assert dense_count(f, f, SHAPE) == 0
    assert hash_count(as_hash(f), as_hash(f)) == 0


def test_d2_change():
    before, after = field([(0, 0, 0)]), field([(0, 0, 0), (3, 3, 3)])
    want = int((before["d2"] != after["d2"]).sum())
    assert 0 < want < N
    upd, gone = dense_updated(before, after, SHAPE)
    assert int(upd.sum()) == want and not gone.any()
    assert upd[lin(3, 3, 3)] and not upd[lin(0, 0, 0)]
    assert dense_count(after, before, SHAPE) == want          # (the delete that undoes it rewrites the same voxels)


def test_unobserved_to_observed():
    seen = np.ones(N, bool)
    seen[lin(2, 0, 0):] = False                              # x >= 2 never observed
    before = field([(0, 1, 1)], observed=seen)
    after = field([(0, 1, 1)])                               # now observed, and reached: -1 -> finite
    assert dense_count(before, after, SHAPE) == 32
    late = field([(0, 1, 1)])
    late["d2"][~seen], late["coc"][~seen] = D2_INF, UNDEFINED   # observed but not reached by a wave: -1 -> D2_INF
    assert dense_count(before, late, SHAPE) == 32
    assert dense_count(before, before, SHAPE) == 0           # -1 -> -1


def test_no_obstacle_to_finite():
    before, after = field([]), field([(2, 2, 2)])
    assert np.all(before["d2"] == D2_INF)
    assert dense_count(before, after, SHAPE) == N
    assert dense_count(after, before, SHAPE) == N            # finite -> D2_INF: the obstacle is gone and so is every d2


def test_tie_repick_with_the_old_obstacle_alive_is_not_counted():
    a, b = (0, 1, 1), (2, 1, 1)                              # mirrored about the plane x = 1
    plane = [(1, y, z) for y in range(4) for z in range(4)]
    before = field([a, b], names={p: a for p in plane})
    after = field([a, b], names={p: b for p in plane})
    assert int(np.any(before["coc"] != after["coc"], axis=1).sum()) == 16 and np.array_equal(before["d2"], after["d2"])
    assert dense_count(before, after, SHAPE) == 0
    assert hash_count(as_hash(before), as_hash(after)) == 0


def test_same_d2_with_the_old_obstacle_gone_is_counted():
    a, b, c = (0, 1, 1), (2, 1, 1), (3, 3, 3)
    plane = [(1, y, z) for y in range(4) for z in range(4)]
    near = {p: a for p in plane if ((np.array(p) - np.array(c)) ** 2).sum() > ((np.array(p) - np.array(a)) ** 2).sum()}
    before = field([a, b, c], names=near)
    after = field([b, c])                                    # a is deleted: the plane keeps its d2 through b
    upd, gone = dense_updated(before, after, SHAPE)
    same = before["d2"] == after["d2"]
    named_a = np.all(before["coc"] == np.array(a), axis=1)
    assert np.array_equal(gone, same & named_a) and int(gone.sum()) >= len(near) > 0
    assert np.array_equal(upd, ~same | gone)
    assert upd[lin(*a)] and not upd[lin(*b)] and not upd[lin(*c)]
    # the same voxels, named b all along: nothing but the d2 changes counts
    before_b = field([a, b, c], names={p: b for p in near})
    assert dense_count(before_b, after, SHAPE) == int((~same).sum()) < int(upd.sum())


def test_an_id_outside_the_array_is_not_occupied():
    before = field([(0, 0, 0)])
    after = {k: v.copy() for k, v in before.items()}
    before["coc"][lin(3, 3, 3)] = (3, 3, 7)                  # (a shard's ghost may name a voxel of its neighbour)
    before["d2"][lin(3, 3, 3)] = after["d2"][lin(3, 3, 3)] = 16
    assert dense_count(before, after, SHAPE) == 1
    occupied = np.zeros((4, 4, 8), bool)
    occupied[3, 3, 7] = occupied[0, 0, 0] = True
    assert dense_count(before, after, SHAPE, occupied=occupied) == 0


def test_ownership_box():
    before, after = field([(0, 0, 0)]), field([(0, 0, 0), (3, 3, 3)])
    upd, _ = dense_updated(before, after, SHAPE)
    v = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lo, hi = (0, 1, 0), (2, 3, 3)
    inside = np.all((v >= lo) & (v <= hi), axis=1)
    want = int((upd & inside).sum())
    assert 0 < want < int(upd.sum())
    assert dense_count(before, after, SHAPE, owned=(lo, hi)) == want
    assert dense_count(before, after, SHAPE, owned=((0, 0, 0), (3, 3, 3))) == int(upd.sum())
    # a shard's array: element (0, 0, 0) is map voxel `origin`, ids are global
    org = np.array((16, 0, 32))
    sb, sa = dict(before), dict(after)
    sb["coc"] = np.where(before["coc"] == UNDEFINED, UNDEFINED, before["coc"] + org)
    sa["coc"] = np.where(after["coc"] == UNDEFINED, UNDEFINED, after["coc"] + org)
    assert dense_count(sb, sa, SHAPE, owned=(lo, hi), origin=org) == want
    a, b = (0, 1, 1), (2, 1, 1)
    gone_b, gone_a = field([a, b]), field([b])
    gb = dict(gone_b)
    gb["coc"] = gone_b["coc"] + org
    assert dense_count(gb, gone_a, SHAPE, origin=org) == dense_count(gone_b, gone_a, SHAPE) > 0


def test_hash_rows_are_matched_by_coordinate_and_new_pages_were_unobserved():
    rng = np.random.RandomState(1)
    shift = (-41, -23, -37)
    before, after = field([(0, 0, 0)]), field([(0, 0, 0), (3, 3, 3)])
    want = dense_count(before, after, SHAPE)
    assert hash_count(as_hash(before, shift, rng.permutation(N)), as_hash(after, shift, rng.permutation(N))) == want
    # the tie rules through the coordinate lookup
    a, b = (0, 1, 1), (2, 1, 1)
    f2, f1 = field([a, b]), field([b])
    assert hash_count(as_hash(f2, shift, rng.permutation(N)), as_hash(f1, shift)) == dense_count(f2, f1, SHAPE) > 0
    # voxels that `before` does not hold: never observed then; counted only if they are observed now
    seen = np.ones(N, bool)
    seen[lin(2, 0, 0):] = False
    part = as_hash(field([(0, 1, 1)]), shift)
    first = {k: v[:32] for k, v in part.items()}
    full = as_hash(field([(0, 1, 1)], observed=seen), shift)
    full["d2"][40:48], full["coc"][40:48] = D2_INF, UNDEFINED     # 8 of the 32 new voxels got observed
    upd, gone, inwin = hash_updated(first, full)
    assert int(upd.sum()) == 8 and np.all(upd[40:48]) and not gone.any() and inwin.all()


def test_window_filter():
    far = (900, 40, -20)
    before = {k: np.concatenate([as_hash(field([(0, 0, 0)]))[k], as_hash(field([(1, 1, 1)]), far)[k]]) for k in ("vox", "d2", "coc", "occ")}
    after = {k: np.concatenate([as_hash(field([(0, 0, 0), (3, 3, 3)]))[k], as_hash(field([(1, 1, 1), (2, 3, 0)]), far)[k]])
             for k in ("vox", "d2", "coc", "occ")}
    near_n = dense_count(field([(0, 0, 0)]), field([(0, 0, 0), (3, 3, 3)]), SHAPE)
    far_n = dense_count(field([(1, 1, 1)]), field([(1, 1, 1), (2, 3, 0)]), SHAPE)
    assert near_n > 0 and far_n > 0
    assert hash_count(before, after) == near_n + far_n
    assert hash_count(before, after, window=(-512, -512, -512)) == near_n       # [-512, 512): the far island is parked
    assert hash_count(before, after, window=(384, -512, -512)) == far_n         # [384, 1408) on x
    upd, _, inwin = hash_updated(before, after, window=(-512, -512, -512))
    assert int(inwin.sum()) == N and not upd[~inwin].any()
    # the window's upper end is exclusive
    assert hash_count(before, after, window=(-1021, -512, -512)) == near_n - int(hash_updated(
        {k: v[:N] for k, v in before.items()}, {k: v[:N] for k, v in after.items()})[0][as_hash(field([]))["vox"][:, 0] == 3].sum())
