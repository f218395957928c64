"""CPU side of the site tour (fiesta_hip_site_tour, include/fiesta_hip.h): the definition and the plumbing.

fiesta_amd.tour_model is the definition: here it is held to the optimum of a Held-Karp dynamic programme on small matrices, to
its own invariants (the length is the sum of the legs and never above the nearest-neighbour tour, the order is a permutation of
the visited sites, no improving move is left unless a restart was capped), to the skip and error rules and to the edge cases
m = 1, 2, 3.  Also: the header declares the two calls, the built library exports them and _lib binds them, the ctypes mirrors
follow the header, the argument rules are checked before any device is touched, and the new kernels use no scratch and spill
nothing.  Everything is integer: comparisons are exact.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fiesta_amd.tour_model import (TOUR_CLOSED, TOUR_SITE_SKIPPED, TOUR_SITE_VISITED, apply_move, best_move, initial_tour, tour_length, tour_mix,
                                   tour_model, tour_rnd)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1


def points_matrix(m, s):
    """the 3-4-5 chamfer distance in free space between m random voxels of a 64^3 block"""
    p = np.random.default_rng(s).integers(0, 64, (m, 3))
    d = np.sort(np.abs(p[:, None, :] - p[None, :, :]), axis=2)
    return (3 * d[..., 2] + d[..., 1] + d[..., 0]).astype(np.int32)


def random_matrix(m, s):
    c = np.random.default_rng(s).integers(1, 1000, (m, m))
    c = np.minimum(c, c.T)
    np.fill_diagonal(c, 0)
    return c.astype(np.int32)


FIXTURES = {"points": points_matrix, "random": random_matrix}


def held_karp(cost, closed):
    """the least length of a path from site 0 through every site (closed: and back), by dynamic programming over subsets"""
    m = len(cost)
    c = cost.astype(np.int64)
    k = m - 1                                            # sites 1 .. m - 1 are bits 0 .. k - 1
    best = np.full((1 << k, k), np.iinfo(np.int64).max // 4, np.int64)
    for j in range(k):
        best[1 << j, j] = c[0, j + 1]
    for mask in range(1, 1 << k):
        ins = np.array([j for j in range(k) if mask >> j & 1])
        for j in range(k):
            if not mask >> j & 1:
                best[mask | 1 << j, j] = min(best[mask | 1 << j, j], (best[mask, ins] + c[ins + 1, j + 1]).min())
    full = best[(1 << k) - 1]
    return int((full + (c[1:, 0] if closed else 0)).min())


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("kind", ["points", "random"])
@pytest.mark.parametrize("scene_seed", range(5))
def test_model_finds_the_optimum(kind, closed, scene_seed):
    cost = FIXTURES[kind](13, scene_seed)
    got = tour_model(cost, closed=closed, restarts=32, seed=12345)
    want = held_karp(cost, closed)
    print(f"{kind} closed={closed} seed {scene_seed}: optimum {want}, model {got['length']}, nearest neighbour {got['nn_length']}, "
          f"first optimal restart {int(np.argmax(got['restart_length'] == want))}")
    assert got["length"] == want


def check_valid(cost, got, start, closed):
    """the invariants of any result; returns the visited sites"""
    n = len(cost)
    m = got["n_visited"]
    visited = np.flatnonzero(got["site_status"] == TOUR_SITE_VISITED)
    assert len(visited) == m and got["order"][0] == start
    assert sorted(got["order"][:m].tolist()) == visited.tolist() and (got["order"][m:] == -1).all() and (got["leg_cost"][m:] == -1).all()
    o = got["order"][:m]
    legs = [int(cost[o[k - 1], o[k]]) for k in range(1, m)]
    first = int(cost[o[-1], o[0]]) if closed and m > 1 else 0
    assert got["leg_cost"][:m].tolist() == [first] + legs
    assert got["length"] == int(got["leg_cost"][:m].astype(np.int64).sum()) <= got["nn_length"]
    assert got["length"] == got["restart_length"].min() == got["restart_length"][got["best_restart"]]
    assert got["best_restart"] == int(np.argmin(got["restart_length"]))
    if got["capped"] == 0:                                      # the returned tour is a local optimum of every move type
        sites = np.array([start] + [j for j in visited if j != start])
        local = cost[np.ix_(sites, sites)]
        tour = [int(np.flatnonzero(sites == s)[0]) for s in o]
        assert best_move(local, tour, closed) is None
    return visited


@pytest.mark.parametrize("closed", [False, True])
def test_validity_and_local_optimality(closed):
    for kind, m, start in (("points", 40, 0), ("random", 33, 7)):
        cost = FIXTURES[kind](m, 11)
        got = tour_model(cost, start=start, closed=closed, restarts=6, seed=5)
        assert got["capped"] == 0 and got["moves"] > 0 and got["n_visited"] == m
        check_valid(cost, got, start, closed)


def test_rng_and_initial_tours():
    x = 0x0123456789ABCDEF                                                    # the mixer, step by step in Python integers
    y = x ^ x >> 30
    y = y * 0xBF58476D1CE4E5B9 % 2 ** 64
    y ^= y >> 27
    y = y * 0x94D049BB133111EB % 2 ** 64
    assert tour_mix(0) == 0 and tour_mix(x) == y ^ y >> 31 and tour_mix(x + 2 ** 64) == tour_mix(x)
    assert tour_rnd(0, 0, 0) == 0 and tour_rnd(7, 3, 5) == tour_mix(tour_mix(7 + 3 * 0x9E3779B97F4A7C15) + 5)
    cost = random_matrix(9, 3)
    nn = initial_tour(cost, 0, 99)
    left = set(range(1, 9))
    for a, b in zip(nn[:-1], nn[1:]):
        assert cost[a, b] == min(cost[a, j] for j in left) and b == min(j for j in left if cost[a, j] == cost[a, b])
        left.remove(b)
    for r in (1, 2, 500):
        t = initial_tour(cost, r, 99)
        assert t[0] == 0 and sorted(t.tolist()) == list(range(9))
    assert not np.array_equal(initial_tour(cost, 1, 99), initial_tour(cost, 2, 99))
    assert not np.array_equal(initial_tour(cost, 1, 99), initial_tour(cost, 1, 100))


def test_best_move_is_the_brute_force_best():
    """the vectorised evaluation against the sentences of the contract, move by move, with the move applied and measured"""
    for closed in (False, True):
        for m, s in ((3, 0), (4, 1), (5, 2), (9, 3), (12, 4)):
            cost = random_matrix(m, s) // 100 + 1                    # small costs: many ties
            np.fill_diagonal(cost, 0)
            tour = initial_tour(cost, 1, s)
            base = tour_length(cost, tour, closed)
            moves = [(0, i, j) for i in range(1, m) for j in range(i + 1, m)]
            moves += [(L, i, p) for L in (1, 2, 3) for i in range(1, m - L + 1) for p in range(m) if not i - 1 <= p <= i + L - 1]
            scored = sorted((tour_length(cost, apply_move(tour, *mv), closed) - base, *mv) for mv in moves)
            want = scored[0] if scored and scored[0][0] < 0 else None
            assert best_move(cost, tour, closed) == want, (closed, m)


def skip_scene():
    """9 sites: site 2 unusable (-1 row and column), sites 5 and 6 a sealed box (INT32_MAX to everyone else)"""
    cost = points_matrix(9, 21)
    cost[2, :] = cost[:, 2] = -1
    for j in (5, 6):
        for k in range(9):
            if k not in (2, 5, 6):
                cost[j, k] = cost[k, j] = INF
    return cost


def test_skips():
    cost = skip_scene()
    got = tour_model(cost, start=3, restarts=4, seed=1)
    assert got["site_status"].tolist() == [0, 0, 1, 0, 0, 1, 1, 0, 0] and got["n_visited"] == 6
    assert check_valid(cost, got, 3, False).tolist() == [0, 1, 3, 4, 7, 8]
    box = tour_model(cost, start=6, closed=True, restarts=2)                    # from inside the box: the box alone
    assert box["order"].tolist() == [6, 5] + [-1] * 7 and box["length"] == 2 * cost[5, 6] and box["leg_cost"][:2].tolist() == [cost[5, 6]] * 2
    alone = tour_model(cost, start=2)                                           # an unusable start reaches nothing
    assert alone["n_visited"] == 1 and alone["order"][0] == 2 and alone["length"] == 0
    assert alone["site_status"].tolist() == [1, 1, 0] + [1] * 6


def test_errors_among_visited_sites():
    cost = skip_scene()
    bad = cost.copy()
    bad[1, 7] = bad[7, 1] = INF                                                 # both reachable from the start, not from each other
    with pytest.raises(ValueError, match="connection"):
        tour_model(bad, start=3)
    bad = cost.copy()
    bad[4, 8] = -1
    bad[8, 4] = -1
    with pytest.raises(ValueError, match="connection"):
        tour_model(bad, start=3)
    bad = cost.copy()
    bad[0, 8] += 1
    with pytest.raises(ValueError, match="symmetric"):
        tour_model(bad, start=3)
    bad[5, 0] = 17                                                              # among skipped sites anything goes
    bad[0, 8] -= 1
    assert tour_model(bad, start=3, restarts=2)["n_visited"] == 6
    for kw in ({"start": 9}, {"start": -1}, {"restarts": 0}, {"restarts": 4097}, {"max_moves": -1}):
        with pytest.raises(ValueError):
            tour_model(cost, **kw)
    with pytest.raises(ValueError):
        tour_model(np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError):
        tour_model(np.zeros((513, 513), np.int32))


def test_edge_cases():
    cost = random_matrix(6, 8)
    for closed in (False, True):
        one = tour_model(cost[:1, :1], closed=closed, restarts=3)
        assert one["order"].tolist() == [0] and one["leg_cost"].tolist() == [0] and one["length"] == 0 and one["moves"] == 0
        assert one["restart_length"].tolist() == [0] * 3
        two = tour_model(cost[:2, :2], closed=closed, restarts=2)
        assert two["order"].tolist() == [0, 1] and two["length"] == cost[0, 1] * (2 if closed else 1) and two["moves"] == 0
        assert two["leg_cost"].tolist() == [cost[0, 1] if closed else 0, cost[0, 1]]
        three = tour_model(cost[:3, :3], closed=closed, restarts=4, seed=3)
        check_valid(cost[:3, :3], three, 0, closed)
        want = 2 * 0 + cost[0, 1] + cost[1, 2] + cost[0, 2] if closed else min(cost[0, 1] + cost[1, 2], cost[0, 2] + cost[1, 2])
        assert three["length"] == want
    # start != 0 and ld > n: the same tour as the matrix with the start's row and column moved to the front
    wide = np.full((6, 9), -5, np.int32)
    wide[:, :6] = cost
    a = tour_model(wide, start=4, closed=True, restarts=5, seed=2)
    perm = [4, 0, 1, 2, 3, 5]
    b = tour_model(cost[np.ix_(perm, perm)], closed=True, restarts=5, seed=2)
    assert a["order"].tolist() == [perm[k] for k in b["order"]] and np.array_equal(a["leg_cost"], b["leg_cost"])
    assert np.array_equal(a["restart_length"], b["restart_length"]) and a["moves"] == b["moves"]
    # max_moves = 1 stops restarts that had more to do
    big = points_matrix(30, 2)
    free = tour_model(big, restarts=4, seed=9)
    cut = tour_model(big, restarts=4, seed=9, max_moves=1)
    assert free["capped"] == 0 and cut["capped"] > 0 and cut["moves"] <= 4 and cut["length"] >= free["length"]
    assert cut["nn_length"] == free["nn_length"]
    check_valid(big, cut, 0, False)


def test_header_library_and_bindings_agree():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    assert fiesta_amd.tour_model is tour_model and fiesta_amd.best_move is best_move and fiesta_amd.TOUR_CLOSED == TOUR_CLOSED
    names = ("fiesta_hip_site_tour", "fiesta_hip_site_tour_dev")
    assert all(n in _lib.declared_symbols() for n in names)
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    for n in names:
        assert n in lib._fiesta_signatures and getattr(lib, n) is not None
    text = open(_lib.HEADER_PATH).read()
    for struct, mirror in (("fiesta_hip_tour_result", _lib.TourResult), ("fiesta_hip_tour_info", _lib.TourInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[.*?\]", "", n).strip(" *") for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(_lib.TourInfo) == 2 * 4 + 4 * 8 and C.sizeof(_lib.TourResult) == 4 * C.sizeof(C.c_void_p)
    for name, value in (("TOUR_MAX_SITES", 512), ("TOUR_MAX_RESTARTS", 4096), ("TOUR_CLOSED", TOUR_CLOSED), ("TOUR_SITE_VISITED", TOUR_SITE_VISITED),
                        ("TOUR_SITE_SKIPPED", TOUR_SITE_SKIPPED)):
        assert re.search(r"#define FIESTA_HIP_%s (\d+)" % name, text).group(1) == str(value)
    block = re.search(r"---- site tour.*?#define FIESTA_HIP_TOUR_MAX_SITES", text, re.S).group(0)
    assert "0x9E3779B97F4A7C15" in block and "0xBF58476D1CE4E5B9" in block and "0x94D049BB133111EB" in block and "RETAINS" in block


def test_argument_rules_are_checked_before_any_device_use():
    """every whole-call error that needs no map is refused, with its own message, before the handle is looked at"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    lib = fiesta_amd.load()
    cost = (C.c_int32 * 4)(0, 5, 5, 0)
    out = (C.c_int32 * 2)(77, 77)
    res = _lib.TourResult(C.cast(out, C.c_void_p), None, None, None)
    #        cost  n    ld start flags R  max_moves   the message names
    cases = [(None, 2, 2, 0, 0, 1, 0, "cost"),
             (cost, 0, 2, 0, 0, 1, 0, "n must"),
             (cost, 513, 513, 0, 0, 1, 0, "n must"),
             (cost, 2, 2, 2, 0, 1, 0, "start"),
             (cost, 2, 2, -1, 0, 1, 0, "start"),
             (cost, 2, 1, 0, 0, 1, 0, "ld"),
             (cost, 2, 2, 0, 0, 0, 0, "restarts"),
             (cost, 2, 2, 0, 0, 4097, 0, "restarts"),
             (cost, 2, 2, 0, 2, 1, 0, "flag"),
             (cost, 2, 2, 0, 0, 1, -1, "max_moves"),
             (cost, 2, 2, 0, 1, 4096, 7, "null map")]                        # nothing wrong but the missing map
    for fn in (lib.fiesta_hip_site_tour, lib.fiesta_hip_site_tour_dev):
        for c, n, ld, start, flags, R, mm, word in cases:
            st = fn(None, c, n, ld, start, flags, R, 12345, mm, C.byref(res), None)
            assert st == 1, (word, st)                                       # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    assert out[0] == 77 and out[1] == 77


def test_tour_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_tour_" in k}
    for kernel, copies in (("k_tour_prepare", 1), ("k_tour_search", 2), ("k_tour_pick", 1)):
        assert sum(kernel in k for k in res) == copies, (kernel, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
