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


# ---- fiesta_hip_reach_matrix: pairwise travel costs, one flood per source ---------------------------------------------------------
REACH_SITE_OK = 0              # FIESTA_HIP_REACH_SITE_*: the per-source status
REACH_SITE_OUTSIDE = 1         # the source lies outside the clipped box
REACH_SITE_BLOCKED = 2         # inside, not traversable


def reach_matrix_model(observed, occupied, sources, targets=None, dist=None, lo=None, hi=None, min_clearance=0.0, connectivity=26, flags=0,
                       origin_vox=(0, 0, 0)):
    """The definition of fiesta_hip_reach_matrix (include/fiesta_hip.h), plain and slow: one reach_model run per usable source.  The
    arrays, the box and the traversability arguments are reach_model's; `sources` (n, 3) map voxels, `targets` (m, 3) the columns
    (None: the sources themselves, the square form).  Row s of a source with status OK is reach_model(seeds=[source s],
    targets=columns)["target_cost"]; the row of a source outside the clipped box (OUTSIDE) or not traversable (BLOCKED) is all -1.
    Returns a dict: cost ((n, n_cols) int32), source_status ((n,) int32), source_reached ((n,) int64: n_reached of the source's
    flood, 0 unless OK), box_lo, box_hi, n_traversable and n_sources_used."""
    src = np.asarray(sources, dtype=np.int64).reshape(-1, 3)
    cols = src if targets is None else np.asarray(targets, dtype=np.int64).reshape(-1, 3)
    kw = dict(dist=dist, lo=lo, hi=hi, min_clearance=min_clearance, connectivity=connectivity, flags=flags, origin_vox=origin_vox)
    base = reach_model(observed, occupied, np.zeros((0, 3), np.int64), targets=src, **kw)   # no seed: the box and traversable(source)
    n = len(src)
    out = {"cost": np.full((n, len(cols)), REACH_BLOCKED, np.int32), "source_status": np.full(n, REACH_SITE_OUTSIDE, np.int32),
           "source_reached": np.zeros(n, np.int64), "box_lo": base["box_lo"], "box_hi": base["box_hi"],
           "n_traversable": base["n_traversable"], "n_sources_used": 0}
    if base["cost"].size == 0:
        return out
    blo, bhi = np.array(base["box_lo"], np.int64), np.array(base["box_hi"], np.int64)
    for s in range(n):
        if np.any(src[s] < blo) or np.any(src[s] > bhi):
            continue
        if base["target_cost"][s] == REACH_BLOCKED:
            out["source_status"][s] = REACH_SITE_BLOCKED
            continue
        r = reach_model(observed, occupied, src[s:s + 1], targets=cols, **kw)
        out["source_status"][s] = REACH_SITE_OK
        out["cost"][s] = r["target_cost"]
        out["source_reached"][s] = r["n_reached"]
        out["n_sources_used"] += 1
    return out


# ---- fiesta_hip_reach_paths: paths out of a cost field -------------------------------------------------------------------------
REACH_PATHS_SHORTCUT = 1       # FIESTA_HIP_REACH_PATHS_SHORTCUT
REACH_PATH_OK = 0              # FIESTA_HIP_REACH_PATH_*: the per-target status
REACH_PATH_OUTSIDE = 1         # the target lies outside the field's box
REACH_PATH_BLOCKED = 2         # cost -1
REACH_PATH_UNREACHED = 3       # cost INT32_MAX
REACH_PATH_BROKEN = 4          # the field is no fixed point here: a voxel without predecessor, or a cost below -1
REACH_PATH_MAX_MANHATTAN = 4095  # voxel steps between the two ends of a visibility test


def reach_walk(p, q):
    """The voxels the reference traversal (src/raycast.cpp:56-158; fiesta_amd.ray_walk's loop) emits from the centre of map voxel
    p to the centre of map voxel q, a = p + 0.5 and b = q + 0.5 in voxel units, without clipping box, without the 1500-voxel
    exception and WITHOUT the ray query's substitution of the last voxel: the traversal may stop one voxel beside q.  A list of
    (x, y, z) tuples; empty for p == q."""
    c = [int(p[0]), int(p[1]), int(p[2])]
    e = [int(q[0]), int(q[1]), int(q[2])]
    a = [c[0] + 0.5, c[1] + 0.5, c[2] + 0.5]
    b = [e[0] + 0.5, e[1] + 0.5, e[2] + 0.5]
    r0, r1, r2 = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    reach2 = r0 * r0 + r1 * r1 + r2 * r2
    step, tmax, tstep = [0] * 3, [0.0] * 3, [0.0] * 3
    for i in range(3):
        delta = float(e[i] - c[i])
        step[i] = (delta > 0) - (delta < 0)
        # intbound of a centre: mod(+-(x + 0.5), 1) is 0.5 for either sign; a zero delta divides by +0
        tmax[i] = (1 - 0.5) / abs(delta) if delta != 0 else float("inf")
        tstep[i] = step[i] / delta if delta != 0 else float("nan")
    out = []
    if step == [0, 0, 0]:
        return out
    for _ in range(8192):
        out.append((c[0], c[1], c[2]))
        q0, q1, q2 = c[0] - a[0], c[1] - a[1], c[2] - a[2]
        if q0 * q0 + q1 * q1 + q2 * q2 > reach2 or c == e:
            break
        if tmax[0] < tmax[1]:
            ax = 0 if tmax[0] < tmax[2] else 2
        else:
            ax = 1 if tmax[1] < tmax[2] else 2
        c[ax] += step[ax]
        tmax[ax] += tstep[ax]
    return out


def reach_visible(cost3d, box_lo, p, q):
    """visible(p, q) of fiesta_hip_reach_paths for map voxels p and q: at most 4095 voxel steps apart, and every voxel of
    reach_walk(p, q) lies inside the field's box (element (0, 0, 0) of `cost3d` is map voxel `box_lo`) and has a cost >= 0"""
    cost = np.asarray(cost3d)
    if sum(abs(int(p[c]) - int(q[c])) for c in range(3)) > REACH_PATH_MAX_MANHATTAN:
        return False
    for v in reach_walk(p, q):
        l = [v[c] - int(box_lo[c]) for c in range(3)]
        if not all(0 <= l[c] < cost.shape[c] for c in range(3)) or cost[l[0], l[1], l[2]] < 0:
            return False
    return True


def reach_paths_model(cost3d, box_lo, targets, connectivity=26, flags=0, max_span=4096, origin=(0.0, 0.0, 0.0), resolution=1.0, stats=None):
    """The definition of fiesta_hip_reach_paths (include/fiesta_hip.h) in plain Python: `cost3d` is a cost field indexed
    [x, y, z] whose element (0, 0, 0) is map voxel `box_lo` (reach_model's "cost" and "box_lo"), `targets` (n, 3) map voxels.
    Per target the descent D[0] = target, D[k + 1] = the first move of reach_moves(connectivity) whose voxel lies in the box, has a
    cost >= 0 and cost + weight == cost(D[k]), down to cost 0; with REACH_PATHS_SHORTCUT the anchors of the greedy line-of-sight
    rule (reach_visible, at most max_span moves per segment), else every voxel; the waypoints are the anchors from the seed to the
    target.  Returns a dict: offsets ((n + 1,) int64, CSR), waypoints_vox ((N, 3) int32), waypoints_pos ((N, 3) f64: Vox2Pos with
    `origin` and `resolution`), status and n_moves ((n,) int32).  `stats`: a dict that receives visibility_tests and voxel_tests, the
    work of the rule target by target with nothing shared: visible() calls, and the voxels they read up to the first that fails."""
    moves = reach_moves(connectivity)
    if flags & ~REACH_PATHS_SHORTCUT:
        raise ValueError("unknown flag bits")
    shortcut = bool(flags & REACH_PATHS_SHORTCUT)
    if shortcut and max_span < 1:
        raise ValueError("max_span must be >= 1 with REACH_PATHS_SHORTCUT")
    cost = np.asarray(cost3d)
    if cost.ndim != 3:
        raise ValueError("cost3d must be a 3-D array")
    ex, ey, ez = cost.shape
    flat = cost.reshape(-1).tolist()
    lo = [int(v) for v in np.asarray(box_lo).reshape(3)]
    tg = np.asarray(targets, dtype=np.int64).reshape(-1, 3)
    step_memo, span_memo, seen = {}, {}, {}

    def descend(v):
        """the voxel after v (cost > 0) on the way down; None: broken"""
        if v in step_memo:
            return step_memo[v]
        x, y, z = v
        c = flat[(x * ey + y) * ez + z]
        found, bad = None, False
        for dx, dy, dz, w in moves:
            a, b, d = x + dx, y + dy, z + dz
            if 0 <= a < ex and 0 <= b < ey and 0 <= d < ez:
                cn = flat[(a * ey + b) * ez + d]
                bad = bad or cn < -1                       # every neighbour of the step is read: one below -1 breaks the path
                if found is None and cn >= 0 and cn + w == c:
                    found = (a, b, d)
        step_memo[v] = None if bad else found
        return step_memo[v]

    def visible(p, q):
        """(visible, voxels read)"""
        if abs(p[0] - q[0]) + abs(p[1] - q[1]) + abs(p[2] - q[2]) > REACH_PATH_MAX_MANHATTAN:
            return False, 0
        if (p, q) not in seen:
            ok, read = True, 0
            for x, y, z in reach_walk(p, q):               # (box-local voxels: a translation by integers changes no bit of the walk)
                read += 1
                if not (0 <= x < ex and 0 <= y < ey and 0 <= z < ez) or flat[(x * ey + y) * ez + z] < 0:
                    ok = False
                    break
            seen[(p, q)] = (ok, read)
        return seen[(p, q)]

    n = len(tg)
    work = [0, 0]                                          # visibility tests, voxels read
    status = np.zeros(n, np.int32)
    n_moves = np.full(n, -1, np.int32)
    paths = []
    for t in range(n):
        v = tuple(int(tg[t, c]) - lo[c] for c in range(3))
        paths.append([])
        if not (0 <= v[0] < ex and 0 <= v[1] < ey and 0 <= v[2] < ez):
            status[t] = REACH_PATH_OUTSIDE
            continue
        c = flat[(v[0] * ey + v[1]) * ez + v[2]]
        if c == REACH_BLOCKED or c == REACH_UNREACHED or c < -1:
            status[t] = REACH_PATH_BLOCKED if c == REACH_BLOCKED else (REACH_PATH_UNREACHED if c == REACH_UNREACHED else REACH_PATH_BROKEN)
            continue
        D = [v]
        while D[-1] is not None and flat[(D[-1][0] * ey + D[-1][1]) * ez + D[-1][2]] > 0:
            D.append(descend(D[-1]))
        if D[-1] is None:
            status[t] = REACH_PATH_BROKEN
            continue
        L = len(D) - 1
        K = list(range(L + 1))
        if shortcut:
            K, i = [0], 0
            while i < L:
                # (the anchor after D[i] depends on D[i] alone: the rest of the descent follows from it)
                if D[i] not in span_memo:
                    j, tests, read = i + 1, 0, 0
                    while j < L and j + 1 - i <= max_span:
                        ok, r = visible(D[i], D[j + 1])
                        tests, read = tests + 1, read + r
                        if not ok:
                            break
                        j += 1
                    span_memo[D[i]] = (j - i, tests, read)
                span, tests, read = span_memo[D[i]]
                work[0], work[1] = work[0] + tests, work[1] + read
                i += span
                K.append(i)
        n_moves[t] = L
        paths[-1] = [D[k] for k in reversed(K)]
    if stats is not None:
        stats["visibility_tests"], stats["voxel_tests"] = work
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(p) for p in paths])
    vox = np.array([w for p in paths for w in p], np.int64).reshape(-1, 3) + np.array(lo, np.int64)
    pos = (vox.astype(np.float64) + 0.5) * float(resolution) + np.asarray(origin, np.float64).reshape(3)
    return {"offsets": offsets, "waypoints_vox": vox.astype(np.int32), "waypoints_pos": pos, "status": status, "n_moves": n_moves}


# ---- fiesta_hip_leg_paths: the legs of a tour, out of the reach matrix's floods ---------------------------------------------------
LEG_NO_SOURCE = 5              # FIESTA_HIP_LEG_NO_SOURCE: the leg's source is not REACH_SITE_OK
LEG_BAD_INDEX = 6              # FIESTA_HIP_LEG_BAD_INDEX: from, or to, is no index into the sources


def leg_paths_model(observed, occupied, sources, from_, to=None, to_vox=None, dist=None, lo=None, hi=None, min_clearance=0.0, connectivity=26,
                    flags=0, path_flags=0, max_span=4096, origin_vox=(0, 0, 0), origin=(0.0, 0.0, 0.0), resolution=1.0, floods=None):
    """The definition of fiesta_hip_leg_paths (include/fiesta_hip.h), plain and slow.  The arrays, `sources`, the box and the
    traversability arguments are reach_matrix_model's: they stand for the batch the matrix call retained.  Leg k runs from source
    from_[k] to source to[k], or to map voxel to_vox[k]; exactly one of `to` and `to_vox` is given.  One reach_model flood per
    distinct usable `from`, then reach_paths_model (path_flags: REACH_PATHS_SHORTCUT or 0; max_span) on that flood's cost for the
    legs that start there.  Status by precedence: LEG_BAD_INDEX (from or to outside 0 .. n - 1), LEG_NO_SOURCE (the source is not
    REACH_SITE_OK), else reach_paths_model's.  Returns reach_paths_model's dict -- the paths run from the source to the target --
    plus cost ((n_legs,) int32: the source's flood at the target voxel, -1 outside the box, -1 for NO_SOURCE and BAD_INDEX) and
    box_lo, box_hi, connectivity, n_sources.  An empty clipped box or no source retains no batch: ValueError.  `floods`: a dict
    that keeps reach_model's result per source index between calls on the SAME batch (same arrays, sources, box and traversability)."""
    if (to is None) == (to_vox is None):
        raise ValueError("exactly one of to and to_vox must be given")
    src = np.asarray(sources, dtype=np.int64).reshape(-1, 3)
    n = len(src)
    kw = dict(dist=dist, lo=lo, hi=hi, min_clearance=min_clearance, connectivity=connectivity, flags=flags, origin_vox=origin_vox)
    base = reach_model(observed, occupied, np.zeros((0, 3), np.int64), targets=src, **kw)   # no seed: the box and traversable(source)
    if n == 0 or base["cost"].size == 0:
        raise ValueError("no batch is retained: no source, or an empty clipped box")
    blo, bhi = np.array(base["box_lo"], np.int64), np.array(base["box_hi"], np.int64)
    usable = np.all((src >= blo) & (src <= bhi), axis=1) & (base["target_cost"] != REACH_BLOCKED)
    fr = np.asarray(from_, dtype=np.int64).reshape(-1)
    legs = len(fr)
    if to is not None:
        ti = np.asarray(to, dtype=np.int64).reshape(-1)
        good = (fr >= 0) & (fr < n) & (ti >= 0) & (ti < n)
        tv = src[np.where(good, ti, 0)]
    else:
        tv = np.asarray(to_vox, dtype=np.int64).reshape(-1, 3)
        good = (fr >= 0) & (fr < n)
    if len(tv) != legs:
        raise ValueError("from and to / to_vox differ in length")
    status = np.full(legs, LEG_BAD_INDEX, np.int32)
    n_moves = np.full(legs, -1, np.int32)
    cost = np.full(legs, REACH_BLOCKED, np.int32)
    paths = [(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float64))] * legs
    status[good & ~usable[np.where(good, fr, 0)]] = LEG_NO_SOURCE
    for s in sorted(set(fr[good & usable[np.where(good, fr, 0)]].tolist())):
        k = np.flatnonzero(good & (fr == s))
        if floods is None or s not in floods:
            field = reach_model(observed, occupied, src[s:s + 1], **kw)
            if floods is not None:
                floods[s] = field
        field = field if floods is None else floods[s]
        r = reach_paths_model(field["cost"], field["box_lo"], tv[k], connectivity, path_flags, max_span, origin, resolution)
        status[k], n_moves[k] = r["status"], r["n_moves"]
        loc = tv[k] - blo
        inside = np.all((loc >= 0) & (loc <= bhi - blo), axis=1)
        cost[k[inside]] = field["cost"][loc[inside, 0], loc[inside, 1], loc[inside, 2]]
        for j, leg in enumerate(k):
            a, b = int(r["offsets"][j]), int(r["offsets"][j + 1])
            paths[leg] = (r["waypoints_vox"][a:b], r["waypoints_pos"][a:b])
    offsets = np.zeros(legs + 1, np.int64)
    offsets[1:] = np.cumsum([len(p[0]) for p in paths])
    vox = np.concatenate([p[0] for p in paths] + [np.zeros((0, 3), np.int32)]).astype(np.int32)
    pos = np.concatenate([p[1] for p in paths] + [np.zeros((0, 3), np.float64)]).astype(np.float64)
    return {"offsets": offsets, "waypoints_vox": vox, "waypoints_pos": pos, "status": status, "n_moves": n_moves, "cost": cost,
            "box_lo": base["box_lo"], "box_hi": base["box_hi"], "connectivity": int(connectivity), "n_sources": n}
