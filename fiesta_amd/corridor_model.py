"""The definition of fiesta_hip_free_boxes and fiesta_hip_path_corridor (include/fiesta_hip.h) in plain Python and numpy:
traversability from ``download_field``-style arrays (fiesta_amd.reach_traversable, the reach calls' own), the face-by-face inflation of
an axis-aligned box, the two candidate voxel chains of a segment and the greedy corridor along a voxel polyline.  Everything is
integer apart from the traversal, the clearance comparison and the metric corners, so a comparison with the library is exact
equality.  This is the model the GPU tests hold the kernels to; tests/test_corridor_rule.py checks it against literal per-voxel loops.
"""
from __future__ import annotations

import numpy as np

from .reach_model import REACH_PATH_MAX_MANHATTAN, reach_traversable, reach_walk

CORRIDOR_THROUGH_UNKNOWN = 1   # FIESTA_HIP_CORRIDOR_THROUGH_UNKNOWN
CORRIDOR_MAX_GROW = 256        # FIESTA_HIP_CORRIDOR_MAX_GROW
CORRIDOR_STOP_BLOCKED = 1      # FIESTA_HIP_CORRIDOR_STOP_*: why a face stopped growing
CORRIDOR_STOP_EDGE = 2
CORRIDOR_STOP_LIMIT = 3
FREE_BOX_OK = 0                # FIESTA_HIP_FREE_BOX_*: the per-seed status
FREE_BOX_OUTSIDE = 1
FREE_BOX_BLOCKED = 2
CORRIDOR_OK = 0                # FIESTA_HIP_CORRIDOR_*: the per-path status
CORRIDOR_INVALID = 1
CORRIDOR_BLOCKED = 2
CORRIDOR_COORD_MAX = 2 ** 30   # waypoint coordinates and a hash-block map's window lie within +-2^30
INT32_MIN = -2 ** 31


class CorridorSpace:
    """traversable(v) over the window W: 3-D arrays indexed [x, y, z] whose element (0, 0, 0) is map voxel `origin_vox`.
    bounded (a dense map or a shard): W is [lo, hi] intersected with the array, both None: the whole array.  Not bounded (a
    hash-block map scattered into an array): what lies outside the array was never observed, [lo, hi] is clamped to +-2^30 and both
    None means everything within +-2^30.  An empty W is `self.empty`."""

    def __init__(self, observed, occupied, dist=None, lo=None, hi=None, min_clearance=0.0, flags=0, origin_vox=(0, 0, 0), bounded=True):
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        if flags & ~CORRIDOR_THROUGH_UNKNOWN:
            raise ValueError("unknown flag bits")
        if min_clearance != min_clearance:
            raise ValueError("min_clearance is NaN")
        self.through = bool(flags & CORRIDOR_THROUGH_UNKNOWN)
        self.trav = reach_traversable(observed, occupied, dist, min_clearance, flags)
        self.org = [int(v) for v in np.asarray(origin_vox).reshape(3)]
        self.shape = [int(v) for v in self.trav.shape]
        big = CORRIDOR_COORD_MAX
        wlo = [-big] * 3 if lo is None else [min(max(int(v), -big), big) for v in np.asarray(lo).reshape(3)]
        whi = [big] * 3 if hi is None else [min(max(int(v), -big), big) for v in np.asarray(hi).reshape(3)]
        if bounded:
            wlo = [self.org[c] if lo is None else max(int(np.asarray(lo).reshape(3)[c]), self.org[c]) for c in range(3)]
            whi = [self.org[c] + self.shape[c] - 1 if hi is None else min(int(np.asarray(hi).reshape(3)[c]), self.org[c] + self.shape[c] - 1)
                   for c in range(3)]
        self.wlo, self.whi = wlo, whi
        self.empty = any(wlo[c] > whi[c] for c in range(3))

    def inside(self, v):
        return not self.empty and all(self.wlo[c] <= v[c] <= self.whi[c] for c in range(3))

    def all_traversable(self, lo, hi):
        """every voxel of the inclusive map-voxel box [lo, hi], which lies inside W, is traversable"""
        a = [max(lo[c] - self.org[c], 0) for c in range(3)]
        b = [min(hi[c] - self.org[c], self.shape[c] - 1) for c in range(3)]
        whole = all(a[c] == lo[c] - self.org[c] and b[c] == hi[c] - self.org[c] for c in range(3))
        if not whole and not self.through:                 # part of the box lies outside the array: never observed
            return False
        if any(a[c] > b[c] for c in range(3)):
            return True
        return bool(self.trav[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1].all())

    def traversable(self, v):
        return self.inside(v) and self.all_traversable(v, v)


def corridor_inflate(space, lo0, hi0, max_grow):
    """inflate(lo0, hi0, max_grow) of the header: faces f = 0 .. 5 are -x, +x, -y, +y, -z, +z; returns (lo, hi, stop)"""
    lo, hi = [int(v) for v in lo0], [int(v) for v in hi0]
    g, stop = [0] * 6, [0] * 6
    while not all(stop):
        for f in range(6):
            if stop[f]:
                continue
            a = f >> 1
            if g[f] == max_grow:
                stop[f] = CORRIDOR_STOP_LIMIT
                continue
            c = hi[a] + 1 if f & 1 else lo[a] - 1
            if c < space.wlo[a] or c > space.whi[a]:
                stop[f] = CORRIDOR_STOP_EDGE
                continue
            slo, shi = list(lo), list(hi)
            slo[a] = shi[a] = c
            if not space.all_traversable(slo, shi):
                stop[f] = CORRIDOR_STOP_BLOCKED
                continue
            if f & 1:
                hi[a] = c
            else:
                lo[a] = c
            g[f] += 1
    return lo, hi, stop


def _box_pos(lo, hi, resolution, origin):
    org = np.asarray(origin, np.float64).reshape(3)
    res = np.float64(resolution)
    return np.concatenate([np.asarray(lo, np.float64) * res + org, (np.asarray(hi, np.float64) + 1.0) * res + org])


def free_box_model(observed, occupied, seeds, dist=None, lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0, origin_vox=(0, 0, 0),
                   bounded=True, resolution=1.0, origin=(0.0, 0.0, 0.0)):
    """fiesta_hip_free_boxes: per seed ((n, 3) map voxels) the box inflate([seed, seed]) in the window W of CorridorSpace.  Returns a
    dict: box ((n, 6) int32: lo xyz, hi xyz), box_pos ((n, 6) f64 metres: the lower corner of lo, the upper corner of hi), stop
    ((n, 6) uint8), volume ((n,) int64) and status ((n,) int32)"""
    if not 0 <= max_grow <= CORRIDOR_MAX_GROW:
        raise ValueError("max_grow must lie in 0 .. 256")
    space = CorridorSpace(observed, occupied, dist, lo, hi, min_clearance, flags, origin_vox, bounded)
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 3)
    n = len(s)
    out = {"box": np.full((n, 6), INT32_MIN, np.int32), "box_pos": np.full((n, 6), np.nan), "stop": np.zeros((n, 6), np.uint8),
           "volume": np.zeros(n, np.int64), "status": np.zeros(n, np.int32)}
    memo = {}
    for i in range(n):
        v = tuple(int(c) for c in s[i])
        if v not in memo:
            if not space.inside(v):
                memo[v] = FREE_BOX_OUTSIDE
            elif not space.all_traversable(v, v):
                memo[v] = FREE_BOX_BLOCKED
            else:
                memo[v] = corridor_inflate(space, v, v, max_grow)
        r = memo[v]
        if isinstance(r, int):
            out["status"][i] = r
            continue
        blo, bhi, stop = r
        out["box"][i] = blo + bhi
        out["box_pos"][i] = _box_pos(blo, bhi, resolution, origin)
        out["stop"][i] = stop
        out["volume"][i] = (bhi[0] - blo[0] + 1) * (bhi[1] - blo[1] + 1) * (bhi[2] - blo[2] + 1)
    return out


_chain_memo = {}


def corridor_chain(p, q):
    """The two candidate chains of the segment p -> q (map voxels): A = walk(p, q) followed by q unless q is its last element,
    B = the reverse of (walk(q, p) followed by p, with the same exception); walk = fiesta_amd.reach_walk, the reference traversal
    from centre to centre.  Both run from p to q.  Lists of (x, y, z) tuples; p == q: ([p], [p])."""
    p = tuple(int(v) for v in p)
    q = tuple(int(v) for v in q)
    d = (q[0] - p[0], q[1] - p[1], q[2] - p[2])
    if d not in _chain_memo:                                # (a translation by integers changes no bit of the walk)
        zero = (0, 0, 0)
        a = reach_walk(zero, d) or [zero]
        if a[-1] != d:
            a.append(d)
        b = reach_walk(d, zero) or [d]
        if b[-1] != zero:
            b.append(zero)
        if len(_chain_memo) > 200000:
            _chain_memo.clear()
        _chain_memo[d] = (a, b[::-1])
    a, b = _chain_memo[d]
    return [(p[0] + x, p[1] + y, p[2] + z) for x, y, z in a], [(p[0] + x, p[1] + y, p[2] + z) for x, y, z in b]


def corridor_model(observed, occupied, waypoints_vox, offsets, dist=None, lo=None, hi=None, max_grow=16, min_clearance=0.0, flags=0,
                   origin_vox=(0, 0, 0), bounded=True, resolution=1.0, origin=(0.0, 0.0, 0.0), stats=None):
    """fiesta_hip_path_corridor: per path of the CSR polylines (`waypoints_vox` (n, 3) map voxels, `offsets` (n_paths + 1,)) the greedy
    sequence of inflated boxes along its voxel chain.  Returns a dict: offsets ((n_paths + 1,) int64, CSR over the boxes), boxes
    ((N, 6) int32), boxes_pos ((N, 6) f64), stop ((N, 6) uint8), entry ((N,) int32: the chain index at which the box was made),
    status, n_chain, blocked_segment ((n_paths,) int32) and blocked_vox ((n_paths, 3) int32).  `stats`: a dict that receives
    segments_b, the segments that took candidate B."""
    if not 0 <= max_grow <= CORRIDOR_MAX_GROW:
        raise ValueError("max_grow must lie in 0 .. 256")
    space = CorridorSpace(observed, occupied, dist, lo, hi, min_clearance, flags, origin_vox, bounded)
    w = np.asarray(waypoints_vox, dtype=np.int64).reshape(-1, 3)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    n = len(off) - 1
    if n < 0:
        raise ValueError("offsets must hold n_paths + 1 entries")
    status, n_chain = np.zeros(n, np.int32), np.zeros(n, np.int32)
    blocked_segment, blocked_vox = np.full(n, -1, np.int32), np.full((n, 3), INT32_MIN, np.int32)
    boxes, stops, entries, counts = [], [], [], []
    inflate_memo, trav_memo = {}, {}
    taken_b = 0

    def trav(v):
        if v not in trav_memo:
            trav_memo[v] = space.traversable(v)
        return trav_memo[v]

    for p in range(n):
        a, b = int(off[p]), int(off[p + 1])
        counts.append(0)
        if b < a or a < 0 or b > len(w):
            status[p] = CORRIDOR_INVALID
            continue
        pts = [tuple(int(c) for c in w[k]) for k in range(a, b)]
        if any(abs(c) > CORRIDOR_COORD_MAX for v in pts for c in v) or \
                any(sum(abs(u[c] - v[c]) for c in range(3)) > REACH_PATH_MAX_MANHATTAN for u, v in zip(pts[:-1], pts[1:])):
            status[p] = CORRIDOR_INVALID
            continue
        if not pts:
            continue
        if not trav(pts[0]):
            status[p], blocked_vox[p] = CORRIDOR_BLOCKED, pts[0]
            continue
        last, prev, idx = None, None, 0

        def visit(v):
            nonlocal last, prev, idx
            if last is None or not all(last[0][c] <= v[c] <= last[1][c] for c in range(3)):
                seed = (v, v) if prev is None else (tuple(min(prev[c], v[c]) for c in range(3)), tuple(max(prev[c], v[c]) for c in range(3)))
                if seed not in inflate_memo:
                    inflate_memo[seed] = corridor_inflate(space, seed[0], seed[1], max_grow)
                last = inflate_memo[seed]
                boxes.append(last[0] + last[1])
                stops.append(last[2])
                entries.append(idx)
                counts[-1] += 1
            prev = v
            idx += 1

        visit(pts[0])
        for j in range(len(pts) - 1):
            if pts[j] == pts[j + 1]:
                continue
            ca, cb = corridor_chain(pts[j], pts[j + 1])
            bad = next((v for v in ca if not trav(v)), None)
            chain = ca
            if bad is not None:
                if all(trav(v) for v in cb):
                    chain = cb
                    taken_b += 1
                else:
                    status[p], blocked_segment[p], blocked_vox[p] = CORRIDOR_BLOCKED, j, bad
                    break
            for v in chain[1:]:
                visit(v)
        n_chain[p] = idx
    if stats is not None:
        stats["segments_b"] = taken_b
    out_off = np.zeros(n + 1, np.int64)
    out_off[1:] = np.cumsum(counts)
    bx = np.array(boxes, np.int64).reshape(-1, 6)
    pos = np.zeros((len(bx), 6))
    if len(bx):
        org = np.asarray(origin, np.float64).reshape(3)
        res = np.float64(resolution)
        pos[:, :3] = bx[:, :3].astype(np.float64) * res + org
        pos[:, 3:] = (bx[:, 3:].astype(np.float64) + 1.0) * res + org
    return {"offsets": out_off, "boxes": bx.astype(np.int32), "boxes_pos": pos, "stop": np.array(stops, np.uint8).reshape(-1, 6),
            "entry": np.array(entries, np.int32), "status": status, "n_chain": n_chain, "blocked_segment": blocked_segment,
            "blocked_vox": blocked_vox}
