"""The definition of fiesta_hip_site_tour (include/fiesta_hip.h) in numpy: order the sites of a symmetric cost matrix into a tour.

Restart-parallel best-improvement local search (2-opt and Or-opt of 1, 2 and 3 sites) over the sites the start can reach; every
number is an integer and every tie has a rule, so the library is held to these bits.  The words of the contract:

  connection   an entry c with 0 <= c < 2^31 - 1 (the reach matrix's convention: -1 unusable site, 2^31 - 1 not reached)
  visited      site j == start, or cost[start][j] is a connection; the m visited sites in ascending order with the start moved to
               the front are the LOCAL indices 0 .. m - 1
  C(a, b)      the cost between the sites at tour POSITIONS a and b; position m is position 0 of a closed tour and does not exist
               in an open one: every term that names it is dropped
  key          (type, i, x): type 0 is 2-opt(i, j = x), type L = 1, 2, 3 is Or-opt(i, p = x) of the L sites t[i .. i + L - 1]
"""
import numpy as np

TOUR_CLOSED = 1
TOUR_MAX_SITES = 512
TOUR_MAX_RESTARTS = 4096
TOUR_SITE_VISITED = 0
TOUR_SITE_SKIPPED = 1
INT32_MAX = 2 ** 31 - 1
_M64 = (1 << 64) - 1
_NONE = np.int64(2 ** 62)          # the delta of a move that does not exist


def tour_mix(x: int) -> int:
    x &= _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x


def tour_rnd(seed: int, r: int, k: int) -> int:
    return tour_mix(tour_mix(seed + r * 0x9E3779B97F4A7C15) + k)


def initial_tour(cost, r: int, seed: int):
    """restart r's first tour over the LOCAL m x m matrix `cost`: nearest neighbour (r = 0) or the seeded shuffle (r >= 1)"""
    m = len(cost)
    if r == 0:
        left = np.ones(m, bool)
        left[0] = False
        t = [0]
        for _ in range(m - 1):
            row = np.where(left, cost[t[-1]].astype(np.int64), _NONE)
            t.append(int(np.argmin(row)))          # (the first least entry: ties go to the lowest index)
            left[t[-1]] = False
        return np.array(t, np.int64)
    t = np.arange(m, dtype=np.int64)
    for k in range(m - 1, 1, -1):
        j = 1 + tour_rnd(seed, r, k) % k
        t[k], t[j] = t[j], t[k]
    return t


def _positional(cost, tour, closed):
    """P[a, b] = C(a, b) for positions 0 .. m (int64); column m is position 0 (closed) or all zero (open: the term is dropped)"""
    te = np.append(tour, tour[0])
    P = np.asarray(cost, np.int64)[np.ix_(te, te)]
    if not closed:
        P[:, -1] = 0
    return P


def tour_length(cost, tour, closed) -> int:
    P = _positional(cost, np.asarray(tour, np.int64), closed)
    k = np.arange(len(tour))
    return int(P[k, k + 1].sum())


def best_move(cost, tour, closed):
    """the move a best-improvement step applies to `tour` (local indices into the m x m `cost`): (delta, type, i, x) with the most
    negative delta, ties to the lowest key; None when no move has delta < 0"""
    tour = np.asarray(tour, np.int64)
    m = len(tour)
    if m < 3:
        return None
    P = _positional(cost, tour, closed)
    I = np.arange(1, m)[:, None]
    X = np.arange(m)[None, :]
    leg = P[np.arange(m), np.arange(m) + 1]                     # C(k, k + 1)
    planes = np.full((4, m - 1, m), _NONE, np.int64)            # [type, i - 1, x]: row-major order is key order
    J = np.maximum(X, 1)
    d = P[I - 1, J] - P[I - 1, I] + P[I, J + 1] - leg[J]
    planes[0] = np.where(X > I, d, _NONE)
    for L in (1, 2, 3):
        if m - L < 1:
            break
        i = np.arange(1, m - L + 1)[:, None]
        e = i + L - 1
        d = (P[i - 1, e + 1] - P[i - 1, i] - leg[e]) + (P[X, i] + P[e, X + 1] - leg[X])
        planes[L, :m - L] = np.where((X < i - 1) | (X > e), d, _NONE)
    at = int(np.argmin(planes))
    delta = int(planes.reshape(-1)[at])
    if delta >= 0:
        return None
    typ, rest = divmod(at, (m - 1) * m)
    return delta, typ, rest // m + 1, rest % m


def apply_move(tour, typ, i, x):
    t = list(tour)
    if typ == 0:
        t[i:x + 1] = t[i:x + 1][::-1]
        return np.array(t, np.int64)
    e = i + typ - 1
    seg = t[i:e + 1]
    if x < i:
        out = t[:x + 1] + seg + t[x + 1:i] + t[e + 1:]
    else:
        out = t[:i] + t[e + 1:x + 1] + seg + t[x + 1:]
    return np.array(out, np.int64)


def tour_model(cost, start=0, closed=False, restarts=64, seed=0, max_moves=0) -> dict:
    """fiesta_hip_site_tour on a host matrix ((n, ld) int32 with ld >= n: the columns past n are ignored).  ValueError where the
    call returns FIESTA_HIP_ERR_INVALID.  Returns order, site_status, leg_cost ((n,) int32), restart_length ((R,) int64) and the
    fields of fiesta_hip_tour_info."""
    if cost is None:
        raise ValueError("site_tour: cost is null")
    cost = np.asarray(cost)
    if cost.ndim != 2 or not 1 <= cost.shape[0] <= TOUR_MAX_SITES or cost.shape[1] < cost.shape[0]:
        raise ValueError("site_tour: n must be 1 .. 512 and ld >= n")
    n = cost.shape[0]
    cost = cost[:, :n].astype(np.int64)
    if not 0 <= start < n:
        raise ValueError("site_tour: start is no site")
    if not 1 <= restarts <= TOUR_MAX_RESTARTS:
        raise ValueError("site_tour: restarts must be 1 .. 4096")
    if max_moves < 0:
        raise ValueError("site_tour: max_moves is negative")
    seed = int(seed) & _M64
    conn = (cost >= 0) & (cost < INT32_MAX)
    visited = conn[start].copy()
    visited[start] = True
    sites = np.array([start] + [j for j in range(n) if visited[j] and j != start], np.int64)
    m = len(sites)
    local = cost[np.ix_(sites, sites)]
    off = ~np.eye(m, dtype=bool)
    if not conn[np.ix_(sites, sites)][off].all():
        raise ValueError("site_tour: two visited sites have no connection")
    if not (local == local.T)[off].all():
        raise ValueError("site_tour: the matrix is not symmetric among the visited sites")
    local[~off] = 0
    cap = max_moves if max_moves > 0 else 8 * m
    lengths = np.zeros(restarts, np.int64)
    best, best_tour, moves, capped, nn_length = -1, None, 0, 0, 0
    for r in range(restarts):
        t = initial_tour(local, r, seed)
        if r == 0:
            nn_length = tour_length(local, t, closed)
        done = 0
        while True:
            mv = best_move(local, t, closed)
            if mv is None:
                break
            if done == cap:
                capped += 1
                break
            t = apply_move(t, *mv[1:])
            done += 1
        moves += done
        lengths[r] = tour_length(local, t, closed)
        if best < 0 or lengths[r] < lengths[best]:
            best, best_tour = r, t
    order = np.full(n, -1, np.int32)
    order[:m] = sites[best_tour]
    leg = np.full(n, -1, np.int32)
    leg[0] = local[best_tour[-1], 0] if closed else 0
    leg[1:m] = local[best_tour[:-1], best_tour[1:]]
    return {"order": order, "site_status": np.where(visited, TOUR_SITE_VISITED, TOUR_SITE_SKIPPED).astype(np.int32), "leg_cost": leg,
            "restart_length": lengths, "n_visited": m, "length": int(lengths[best]), "best_restart": best, "nn_length": int(nn_length),
            "moves": moves, "capped": capped}
