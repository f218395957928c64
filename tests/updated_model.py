"""The "updated voxel" of fiesta_hip_snapshot_count_updated (include/fiesta_hip.h) in plain numpy: the definition the GPU
counts are held to (tests/test_gpu_updated_unit.py), itself checked on hand-made fields by tests/test_updated_model.py.

A voxel is UPDATED between two exports of a map (download_field / download_hash: d2 = -1 never observed, D2_INF observed
without an obstacle, else the squared voxel distance; coc = the closest obstacle's voxel, UNDEFINED without one) iff

  * d2 differs; or
  * d2 is equal, the voxel named an obstacle BEFORE, and that obstacle's voxel is not occupied AFTER.

So a voxel that merely names another of several equidistant obstacles while its old one still stands is not updated (the
whole-grid transforms re-pick such ties all over the map), and what an export does not show -- the transient frontier tag
of a word, a stale link under "no obstacle" -- cannot count.  The formula is the one of tests/golden/make_golden_c2.py.
"""
from __future__ import annotations

import numpy as np

D2_INF = 0x7FFFFFFF
UNDEFINED = -10000       # FIESTA_HIP_UNDEFINED: coc of a voxel without an obstacle
HASH_WINDOW = 1024       # voxels per axis of a hash-block map's window


def _coords(shape):
    return np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)


def updated_flags(d2_before, d2_after, coc_before, alive_after):
    """The rule itself, per voxel: `alive_after[i]` says whether the obstacle voxel i named before (coc_before[i]) is occupied
    after; it is read only where coc_before[i] names an obstacle.  Returns (updated, only_gone): the flags, and those of them
    that hold through the second clause alone (d2 equal, old obstacle gone)."""
    d2_before, d2_after = np.asarray(d2_before, np.int64), np.asarray(d2_after, np.int64)
    named = np.asarray(coc_before)[:, 0] != UNDEFINED
    changed = d2_before != d2_after
    only_gone = ~changed & named & ~np.asarray(alive_after, bool)
    return changed | only_gone, only_gone


def dense_updated(before, after, shape, owned=None, origin=(0, 0, 0), occupied=None):
    """Flags of a dense map's voxels, in the order of download_field (x slowest, z fastest).  before / after: dictionaries with
    d2, coc, occ as download_field returns them, over an array of `shape` whose element (0, 0, 0) is map voxel `origin` (non-zero
    on a shard: ids are global).  owned = (lo, hi): an inclusive box in ARRAY coordinates; voxels outside it are not counted (a
    shard's ghost layers).  occupied: a 3-D array over map voxels (0, 0, 0) ... that replaces after["occ"] where an id may name a
    voxel outside the array (a shard: the global grid's occupancy).  An id outside the array that is looked up is not occupied.
    Returns (updated, only_gone) as updated_flags does, with `owned` applied to both."""
    shape = tuple(int(s) for s in shape)
    n = shape[0] * shape[1] * shape[2]
    cb = np.asarray(before["coc"], np.int64).reshape(n, 3)
    if occupied is None:
        occ, org = np.asarray(after["occ"]).reshape(shape) != 0, np.asarray(origin, np.int64)
    else:
        occ, org = np.asarray(occupied) != 0, np.zeros(3, np.int64)
    c = cb - org
    inside = np.all((c >= 0) & (c < np.array(occ.shape)), axis=1)
    c = np.where(inside[:, None], c, 0)
    alive = inside & occ[c[:, 0], c[:, 1], c[:, 2]]
    upd, gone = updated_flags(before["d2"], after["d2"], cb, alive)
    if owned is not None:
        v = _coords(shape)
        keep = np.all((v >= np.asarray(owned[0])) & (v <= np.asarray(owned[1])), axis=1)
        upd, gone = upd & keep, gone & keep
    return upd, gone


def dense_count(before, after, shape, **kw):
    return int(dense_updated(before, after, shape, **kw)[0].sum())


def _key(v):
    v = np.asarray(v, np.int64).reshape(-1, 3)
    return ((v[:, 0] + (1 << 20)) << 42) | ((v[:, 1] + (1 << 20)) << 21) | (v[:, 2] + (1 << 20))


def _lookup(sorted_keys, keys):
    """position of every key in sorted_keys and whether it is there"""
    if len(sorted_keys) == 0:
        return np.zeros(len(keys), np.int64), np.zeros(len(keys), bool)
    pos = np.clip(np.searchsorted(sorted_keys, keys), 0, len(sorted_keys) - 1)
    return pos, sorted_keys[pos] == keys


def hash_updated(before, after, window=None):
    """Flags of a hash-block map's voxels, one per row of after["vox"].  before / after: dictionaries with vox, d2, coc, occ as
    download_hash returns them; the rows are matched by voxel coordinate, not by position.  A voxel absent from `before` was never
    observed then (d2 -1, no obstacle named); an obstacle voxel absent from `after` is not occupied.  (Pages are never released, so
    every voxel of `before` is in `after`: checked.)  window: the map voxel of the window's lowest corner; voxels outside
    [window, window + 1024) -- pages that are parked -- are not counted.  Returns (updated, only_gone, in_window)."""
    va, vb = np.asarray(after["vox"], np.int64), np.asarray(before["vox"], np.int64)
    ka, kb = _key(va), _key(vb)
    ob = np.argsort(kb)
    pos, have = _lookup(kb[ob], ka)
    assert int(have.sum()) == len(kb) == len(np.unique(kb)), "a voxel of `before` is missing from `after`, or listed twice"
    row = ob[pos] if len(kb) else pos
    d2b = np.where(have, np.asarray(before["d2"], np.int64)[row] if len(kb) else -1, -1)
    cb = np.where(have[:, None], np.asarray(before["coc"], np.int64)[row] if len(kb) else UNDEFINED, UNDEFINED)
    oa = np.argsort(ka)
    cpos, chave = _lookup(ka[oa], _key(cb))
    alive = chave & (np.asarray(after["occ"])[oa[cpos]] != 0)
    upd, gone = updated_flags(d2b, after["d2"], cb, alive)
    inwin = np.ones(len(va), bool)
    if window is not None:
        w = np.asarray(window, np.int64)
        inwin = np.all((va >= w) & (va < w + HASH_WINDOW), axis=1)
    return upd & inwin, gone & inwin, inwin


def hash_count(before, after, window=None):
    return int(hash_updated(before, after, window)[0].sum())
