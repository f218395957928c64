"""The definition of fiesta_hip_reach_field (include/fiesta_hip.h) in numpy and plain Python: traversability from
``download_field``-style arrays, then a heap Dijkstra over the 3-4-5 chamfer moves.  Everything is integer, so a comparison with the
library is exact equality.  This is the model the GPU tests hold the kernels to; it is itself checked against a literal
Bellman-Ford triple loop in tests/test_reach_rule.py.
"""
from __future__ import annotations

import heapq

import numpy as np

REACH_THROUGH_UNKNOWN = 1      # FIESTA_HIP_REACH_THROUGH_UNKNOWN
REACH_UNREACHED = 2 ** 31 - 1  # cost of a traversable voxel no move sequence reaches (INT32_MAX)
REACH_BLOCKED = -1             # cost of a voxel that is not traversable
REACH_MAX_VOXELS = 2 ** 28     # of the clipped box


def reach_moves(connectivity):
    """[(dx, dy, dz, weight)]: the moves of `connectivity` 6 or 26 -- 1, 2 or 3 axes changed weigh 3, 4 or 5"""
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = abs(dx) + abs(dy) + abs(dz)
                if k == 1 or (k > 1 and connectivity == 26):
                    out.append((dx, dy, dz, 2 + k))
    return out


def reach_traversable(observed, occupied, dist=None, min_clearance=0.0, flags=0):
    """traversable(v) of the header over whole arrays: observed and not occupied and (only if min_clearance > 0) dist >= min_clearance,
    or -- with REACH_THROUGH_UNKNOWN -- not observed"""
    obs = np.asarray(observed, dtype=bool)
    trav = obs & ~np.asarray(occupied, dtype=bool)
    if min_clearance > 0:
        trav &= np.asarray(dist, dtype=np.float64) >= min_clearance
    if flags & REACH_THROUGH_UNKNOWN:
        trav |= ~obs
    return trav


def reach_model(observed, occupied, seeds, dist=None, lo=None, hi=None, min_clearance=0.0, connectivity=26, flags=0, targets=None,
                origin_vox=(0, 0, 0)):
    """fiesta_hip_reach_field over 3-D arrays indexed [x, y, z] whose element (0, 0, 0) is map voxel `origin_vox` (a dense map's
    array; a hash-block map scattered into an array that covers the box).  lo / hi: the inclusive map-voxel box (both None: the
    whole array), clipped to the array.  Returns a dict: cost ((ex, ey, ez) int32 -- flatten it for the library's order),
    target_cost ((n,) int32, only with `targets`), and the fields of fiesta_hip_reach_info except rounds and tile_visits."""
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi must both be given or both be None")
    if flags & ~REACH_THROUGH_UNKNOWN:
        raise ValueError("unknown flag bits")
    if min_clearance != min_clearance:
        raise ValueError("min_clearance is NaN")
    moves = reach_moves(connectivity)
    obs = np.asarray(observed, dtype=bool)
    org = np.asarray(origin_vox, dtype=np.int64).reshape(3)
    shape = np.array(obs.shape, dtype=np.int64)
    blo = np.zeros(3, np.int64) if lo is None else np.maximum(np.asarray(lo, dtype=np.int64).reshape(3) - org, 0)
    bhi = shape - 1 if hi is None else np.minimum(np.asarray(hi, dtype=np.int64).reshape(3) - org, shape - 1)
    seeds = np.asarray(seeds, dtype=np.int64).reshape(-1, 3)
    tg = None if targets is None else np.asarray(targets, dtype=np.int64).reshape(-1, 3)
    out = {"box_lo": [0, 0, 0], "box_hi": [0, 0, 0], "n_traversable": 0, "n_seeds_used": 0, "n_reached": 0, "max_cost": 0}
    if np.any(blo > bhi):
        out["cost"] = np.zeros((0, 0, 0), np.int32)
        if tg is not None:
            out["target_cost"] = np.full(len(tg), REACH_BLOCKED, np.int32)
        return out
    ext = bhi - blo + 1
    if int(ext[0]) * int(ext[1]) * int(ext[2]) > REACH_MAX_VOXELS:
        raise ValueError("the clipped box holds more than 2^28 voxels")
    box = tuple(slice(int(a), int(b) + 1) for a, b in zip(blo, bhi))
    trav = reach_traversable(obs[box], np.asarray(occupied, dtype=bool)[box], None if dist is None else np.asarray(dist)[box],
                             min_clearance, flags)
    # a border of blocked voxels around the box: no move needs a bounds test
    pad = np.zeros(tuple(int(e) + 2 for e in ext), bool)
    pad[1:-1, 1:-1, 1:-1] = trav
    sy, sx = int(ext[2]) + 2, (int(ext[1]) + 2) * (int(ext[2]) + 2)
    steps = [(dx * sx + dy * sy + dz, w) for dx, dy, dz, w in moves]
    ok = pad.reshape(-1).tolist()
    cost = [REACH_UNREACHED] * len(ok)
    heap = []
    s = seeds - (org + blo)
    inside = np.all((s >= 0) & (s < ext), axis=1)
    for x, y, z in s[inside]:
        i = (int(x) + 1) * sx + (int(y) + 1) * sy + int(z) + 1
        if ok[i]:
            out["n_seeds_used"] += 1
            if cost[i]:
                cost[i] = 0
                heap.append((0, i))
    while heap:
        c, i = heapq.heappop(heap)
        if c > cost[i]:
            continue
        for step, w in steps:
            j = i + step
            if ok[j] and c + w < cost[j]:
                cost[j] = c + w
                heapq.heappush(heap, (c + w, j))
    field = np.array(cost, dtype=np.int64).reshape(pad.shape)[1:-1, 1:-1, 1:-1]
    field = np.where(trav, field, REACH_BLOCKED).astype(np.int32)
    reached = trav & (field != REACH_UNREACHED)
    out.update(cost=field, box_lo=[int(v) for v in blo + org], box_hi=[int(v) for v in bhi + org], n_traversable=int(trav.sum()),
               n_reached=int(reached.sum()), max_cost=int(field[reached].max()) if reached.any() else 0)
    if tg is not None:
        t = tg - (org + blo)
        tin = np.all((t >= 0) & (t < ext), axis=1)
        tc = np.full(len(tg), REACH_BLOCKED, np.int32)
        tc[tin] = field[t[tin, 0], t[tin, 1], t[tin, 2]]
        out["target_cost"] = tc
    return out
