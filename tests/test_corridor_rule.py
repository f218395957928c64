"""CPU side of the free-space corridors (fiesta_hip_free_boxes and fiesta_hip_path_corridor, include/fiesta_hip.h): the definition
and the plumbing.

fiesta_amd.free_box_model / corridor_chain / corridor_model are the definition: here they are held to literal per-voxel loops on
small random maps, to the six guarantees of the header, and to the facts about the two candidate chains of a segment that the
header states (6-connected, monotone, 1 + |p - q|_1 voxels from p to q, with the appended end voxel where the traversal stops
beside it).  Also: the header declares the four calls, the built library exports them and _lib binds them, the ctypes mirrors
follow the header, the argument rules are checked before any device is touched, and the new kernels spill nothing.  Everything is
integer or bit-exact f64: comparisons are exact.
"""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from fiesta_amd.corridor_model import (CORRIDOR_BLOCKED, CORRIDOR_INVALID, CORRIDOR_MAX_GROW, CORRIDOR_OK, CORRIDOR_STOP_BLOCKED, CORRIDOR_STOP_EDGE,
                                       CORRIDOR_STOP_LIMIT, CORRIDOR_THROUGH_UNKNOWN, FREE_BOX_BLOCKED, FREE_BOX_OK, FREE_BOX_OUTSIDE, corridor_chain,
                                       corridor_model, free_box_model)
from fiesta_amd.reach_model import reach_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = -2 ** 31


def random_map(seed, shape=(9, 8, 11), p_occ=0.12, p_unknown=0.1):
    rng = np.random.RandomState(seed)
    obs = rng.rand(*shape) >= p_unknown
    occ = obs & (rng.rand(*shape) < p_occ)
    dist = np.where(occ, 0.0, rng.rand(*shape) * 0.6)          # (any numbers: the model compares, it does not derive them)
    return obs, occ, dist


class Literal:
    """traversable(v) and inflate() voxel by voxel, straight from the header's sentences"""

    def __init__(self, obs, occ, dist, lo, hi, clearance, flags, origin_vox, bounded):
        self.obs, self.occ, self.dist, self.clr, self.flags, self.org, self.bounded = obs, occ, dist, clearance, flags, origin_vox, bounded
        big = 2 ** 30
        if bounded:
            self.wlo = [origin_vox[c] if lo is None else max(lo[c], origin_vox[c]) for c in range(3)]
            self.whi = [origin_vox[c] + obs.shape[c] - 1 if hi is None else min(hi[c], origin_vox[c] + obs.shape[c] - 1) for c in range(3)]
        else:
            self.wlo = [-big if lo is None else max(min(lo[c], big), -big) for c in range(3)]
            self.whi = [big if hi is None else max(min(hi[c], big), -big) for c in range(3)]

    def in_w(self, v):
        return all(self.wlo[c] <= v[c] <= self.whi[c] for c in range(3))

    def trav(self, v):
        if not self.in_w(v):
            return False
        l = [v[c] - self.org[c] for c in range(3)]
        if not all(0 <= l[c] < self.obs.shape[c] for c in range(3)):
            return bool(self.flags & CORRIDOR_THROUGH_UNKNOWN)          # (only an unbounded map has voxels of W outside the arrays)
        l = tuple(l)
        if not self.obs[l]:
            return bool(self.flags & CORRIDOR_THROUGH_UNKNOWN)
        return not self.occ[l] and (self.clr <= 0 or self.dist[l] >= self.clr)

    def inflate(self, lo0, hi0, max_grow):
        lo, hi, g, stop = list(lo0), list(hi0), [0] * 6, [0] * 6
        while 0 in stop:
            for f in range(6):
                if stop[f]:
                    continue
                a = f >> 1
                if g[f] == max_grow:
                    stop[f] = 3
                    continue
                c = hi[a] + 1 if f & 1 else lo[a] - 1
                if not self.wlo[a] <= c <= self.whi[a]:
                    stop[f] = 2
                    continue
                rng = [range(lo[k], hi[k] + 1) for k in range(3)]
                rng[a] = [c]
                if not all(self.trav(v) for v in itertools.product(*rng)):
                    stop[f] = 1
                    continue
                if f & 1:
                    hi[a] = c
                else:
                    lo[a] = c
                g[f] += 1
        return lo, hi, stop


CASES = [(None, None, 0.0, 0, True), ((1, 2, 3), (7, 6, 9), 0.0, 0, True), (None, None, 0.25, CORRIDOR_THROUGH_UNKNOWN, True),
         ((-4, -4, -4), (20, 20, 20), 0.0, CORRIDOR_THROUGH_UNKNOWN, True), ((0, 1, 0), (12, 9, 14), 0.0, CORRIDOR_THROUGH_UNKNOWN, False),
         (None, None, 0.3, 0, False), ((5, 5, 5), (4, 9, 9), 0.0, 0, True)]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("max_grow", [0, 1, 3, 256])
def test_free_boxes_against_literal_loops(case, max_grow):
    lo, hi, clr, flags, bounded = CASES[case]
    seen_status, seen_stop = set(), set()
    for seed in range(3):
        obs, occ, dist = random_map(seed + 10 * case)
        org = (2, -3, 1) if seed == 1 else (0, 0, 0)
        shift = lambda v: None if v is None else tuple(v[c] + org[c] for c in range(3))   # noqa: E731
        L = Literal(obs, occ, dist, shift(lo), shift(hi), clr, flags, org, bounded)
        seeds = np.array(list(itertools.product(range(-1, obs.shape[0] + 1, 2), range(-1, obs.shape[1] + 1, 2), range(-1, obs.shape[2] + 1, 3)))) + org
        got = free_box_model(obs, occ, seeds, dist, shift(lo), shift(hi), max_grow, clr, flags, org, bounded, 0.1, (0.3, -0.2, 1.0))
        for i, v in enumerate(seeds.tolist()):
            if not L.in_w(v):
                want = (FREE_BOX_OUTSIDE, [INT32_MIN] * 6, [0] * 6, 0)
            elif not L.trav(v):
                want = (FREE_BOX_BLOCKED, [INT32_MIN] * 6, [0] * 6, 0)
            else:
                blo, bhi, stop = L.inflate(v, v, max_grow)
                want = (FREE_BOX_OK, blo + bhi, stop, int(np.prod([bhi[c] - blo[c] + 1 for c in range(3)])))
            assert (got["status"][i], got["box"][i].tolist(), got["stop"][i].tolist(), got["volume"][i]) == want, (seed, v)
            if want[0] == FREE_BOX_OK:
                pos = [np.float64(want[1][c]) * np.float64(0.1) + (0.3, -0.2, 1.0)[c] for c in range(3)] + \
                      [(np.float64(want[1][3 + c]) + 1.0) * np.float64(0.1) + (0.3, -0.2, 1.0)[c] for c in range(3)]
                assert got["box_pos"][i].tolist() == pos
                if max_grow == 0:
                    assert want[1] == v + v and want[2] == [3] * 6                     # guarantee 5
            else:
                assert np.isnan(got["box_pos"][i]).all()
            seen_status.add(want[0])
            seen_stop |= set(want[2])
    if case in (0, 1, 3) and max_grow in (1, 3):
        assert seen_status == {FREE_BOX_OK, FREE_BOX_OUTSIDE, FREE_BOX_BLOCKED} and seen_stop >= {1, 2, 3}, (seen_status, seen_stop)
    if case == 6:
        assert seen_status == {FREE_BOX_OUTSIDE}


def check_chain(p, q, chain):
    n = sum(abs(p[c] - q[c]) for c in range(3))
    assert chain[0] == p and chain[-1] == q and len(chain) == n + 1, (p, q, chain)
    sg = [np.sign(q[c] - p[c]) for c in range(3)]
    for u, v in zip(chain[:-1], chain[1:]):
        d = [v[c] - u[c] for c in range(3)]
        assert sorted(map(abs, d)) == [0, 0, 1] and all(d[c] in (0, sg[c]) for c in range(3)), (p, q, u, v)     # 6-connected, monotone


def test_chain_facts():
    """both candidates are 6-connected monotone chains of 1 + |p - q|_1 voxels from p to q; the traversal may stop beside q"""
    beside = 0
    pairs = [((0, 0, 0), d) for d in itertools.product(range(-6, 7), repeat=3)]
    rng = np.random.RandomState(5)
    a = rng.randint(-500, 500, (20000, 3))
    b = a + rng.randint(-60, 61, (20000, 3))
    pairs += [(tuple(int(v) for v in a[i]), tuple(int(v) for v in b[i])) for i in range(len(a))]
    assert len(pairs) == 2197 + 20000
    for p, q in pairs:
        ca, cb = corridor_chain(p, q)
        if p == q:
            assert ca == cb == [p]
            continue
        check_chain(p, q, ca)
        check_chain(p, q, cb)
        w = reach_walk(p, q)
        assert ca[:len(w)] == w and len(ca) - len(w) in (0, 1)
        beside += len(ca) - len(w)
        w = reach_walk(q, p)
        assert cb[::-1][:len(w)] == w and len(cb) - len(w) in (0, 1)
    assert beside > 100                                                     # (the appended q is needed, and it suffices)
    # a diagonal move: A and B are two different axis orders
    ca, cb = corridor_chain((0, 0, 0), (1, 1, 0))
    assert len(ca) == len(cb) == 3 and ca[1] != cb[1] and {ca[1], cb[1]} == {(1, 0, 0), (0, 1, 0)}


def literal_corridor(L, pts, max_grow):
    """the corridor of one valid path, from the header's sentences; returns (status, boxes, stops, entries, n_chain, bseg, bvox)"""
    boxes, stops, entries = [], [], []
    if not pts:
        return CORRIDOR_OK, boxes, stops, entries, 0, -1, [INT32_MIN] * 3
    if not L.trav(pts[0]):
        return CORRIDOR_BLOCKED, boxes, stops, entries, 0, -1, list(pts[0])
    prev, idx = None, 0
    chain_all = [(pts[0], None)]
    status, bseg, bvox = CORRIDOR_OK, -1, [INT32_MIN] * 3
    for j in range(len(pts) - 1):
        if pts[j] == pts[j + 1]:
            continue
        ca, cb = corridor_chain(pts[j], pts[j + 1])
        if all(L.trav(v) for v in ca):
            use = ca
        elif all(L.trav(v) for v in cb):
            use = cb
        else:
            status, bseg, bvox = CORRIDOR_BLOCKED, j, list(next(v for v in ca if not L.trav(v)))
            break
        chain_all += [(v, None) for v in use[1:]]
    for v, _ in chain_all:
        if not boxes or not all(boxes[-1][c] <= v[c] <= boxes[-1][3 + c] for c in range(3)):
            s = (v, v) if prev is None else ([min(prev[c], v[c]) for c in range(3)], [max(prev[c], v[c]) for c in range(3)])
            blo, bhi, stop = L.inflate(s[0], s[1], max_grow)
            boxes.append(blo + bhi)
            stops.append(stop)
            entries.append(idx)
        prev = v
        idx += 1
    return status, boxes, stops, entries, idx, bseg, bvox


def random_paths(rng, shape, org, n_paths):
    pts, off = [], [0]
    for k in range(n_paths):
        m = int(rng.randint(0, 7))
        v = rng.randint(0, shape, 3)
        for _ in range(m):
            pts.append(v + org)
            step = rng.randint(-3, 4, 3) if rng.rand() < 0.5 else rng.randint(-1, 2, 3)
            v = np.clip(v + step, -1, np.array(shape))
        off.append(len(pts))
    return np.array(pts, np.int64).reshape(-1, 3), np.array(off, np.int64)


@pytest.mark.parametrize("case", range(len(CASES) - 1))
def test_corridor_against_literal_loops_and_guarantees(case):
    lo, hi, clr, flags, bounded = CASES[case]
    seen, total_b = set(), 0
    for seed in range(4):
        obs, occ, dist = random_map(100 + seed + 10 * case, p_occ=0.06, p_unknown=0.04)
        org = (2, -3, 1) if seed % 2 else (0, 0, 0)
        shift = lambda v: None if v is None else tuple(v[c] + org[c] for c in range(3))   # noqa: E731
        L = Literal(obs, occ, dist, shift(lo), shift(hi), clr, flags, org, bounded)
        w, off = random_paths(np.random.RandomState(seed), obs.shape, np.array(org), 60)
        for max_grow in (0, 2, 256):
            stats = {}
            got = corridor_model(obs, occ, w, off, dist, shift(lo), shift(hi), max_grow, clr, flags, org, bounded, 0.1, (0.3, -0.2, 1.0), stats)
            total_b += stats["segments_b"]
            for p in range(len(off) - 1):
                pts = [tuple(int(c) for c in v) for v in w[off[p]:off[p + 1]]]
                st, boxes, stops, entries, n_chain, bseg, bvox = literal_corridor(L, pts, max_grow)
                a, b = got["offsets"][p], got["offsets"][p + 1]
                assert (got["status"][p], got["boxes"][a:b].tolist(), got["stop"][a:b].tolist(), got["entry"][a:b].tolist(), got["n_chain"][p],
                        got["blocked_segment"][p], got["blocked_vox"][p].tolist()) == (st, boxes, stops, entries, n_chain, bseg, bvox), (seed, p)
                seen.add(st)
                # the guarantees, on the model's output
                for k, (bx, sp) in enumerate(zip(boxes, stops)):
                    vox = list(itertools.product(*[range(bx[c], bx[3 + c] + 1) for c in range(3)]))
                    assert all(L.trav(v) for v in vox)                                         # 1
                    if k:
                        pb = boxes[k - 1]
                        assert all(max(pb[c], bx[c]) <= min(pb[3 + c], bx[3 + c]) for c in range(3))   # 2
                    for f in range(6):                                                         # 4
                        a_ = f >> 1
                        c = bx[3 + a_] + 1 if f & 1 else bx[a_] - 1
                        if sp[f] == CORRIDOR_STOP_EDGE:
                            assert not L.wlo[a_] <= c <= L.whi[a_]
                        elif sp[f] == CORRIDOR_STOP_BLOCKED:
                            r = [range(bx[k2], bx[3 + k2] + 1) for k2 in range(3)]
                            r[a_] = [c]
                            assert not all(L.trav(v) for v in itertools.product(*r))
                        else:
                            assert sp[f] == CORRIDOR_STOP_LIMIT
                    if max_grow == 0:
                        assert np.prod([bx[3 + c] - bx[c] + 1 for c in range(3)]) <= 2 and sp == [3] * 6    # 5
            pos = got["boxes_pos"]
            bx = got["boxes"].astype(np.float64)
            assert np.array_equal(pos[:, :3], bx[:, :3] * np.float64(0.1) + np.array((0.3, -0.2, 1.0)))
            assert np.array_equal(pos[:, 3:], (bx[:, 3:] + 1.0) * np.float64(0.1) + np.array((0.3, -0.2, 1.0)))
    assert seen >= {CORRIDOR_OK, CORRIDOR_BLOCKED}
    if case == 0:
        assert total_b > 0


def test_entry_is_the_chain_index_and_every_visit_lies_in_the_last_box():
    """guarantee 3, replayed from the outputs: walking the chain, the box whose entry was passed last holds the voxel"""
    obs, occ, dist = random_map(7, shape=(14, 12, 10), p_occ=0.03, p_unknown=0.0)
    w, off = random_paths(np.random.RandomState(3), obs.shape, np.zeros(3, int), 240)
    got = corridor_model(obs, occ, w, off, max_grow=3)
    L = Literal(obs, occ, dist, None, None, 0.0, 0, (0, 0, 0), True)
    checked = 0
    for p in np.flatnonzero(got["status"] == CORRIDOR_OK):
        pts = [tuple(int(c) for c in v) for v in w[off[p]:off[p + 1]]]
        if not pts:
            continue
        chain = [pts[0]]
        for u, v in zip(pts[:-1], pts[1:]):
            if u != v:
                ca, cb = corridor_chain(u, v)
                chain += (ca if all(L.trav(x) for x in ca) else cb)[1:]
        a, b = got["offsets"][p], got["offsets"][p + 1]
        entry, boxes = got["entry"][a:b], got["boxes"][a:b]
        assert got["n_chain"][p] == len(chain) and entry[0] == 0 and (np.diff(entry) > 0).all()
        for i, v in enumerate(chain):
            k = int(np.searchsorted(entry, i, side="right")) - 1
            assert all(boxes[k][c] <= v[c] <= boxes[k][3 + c] for c in range(3))
            checked += 1
    assert checked > 200


def test_invalid_paths_and_argument_rules_of_the_model():
    obs, occ, _ = random_map(1, p_occ=0.0, p_unknown=0.0)
    w = np.array([(1, 1, 1), (1, 1, 1), (2, 2, 2), (1, 1, 1), (1, 4097, 1), (2 ** 30 + 1, 0, 0), (3, 3, 3)])
    off = np.array([0, 3, 5, 6, 6, 7, 5, 9])
    got = corridor_model(obs, occ, w, off, max_grow=0)        # (every chain voxel after the first starts a box of two voxels)
    assert got["status"].tolist() == [CORRIDOR_OK, CORRIDOR_INVALID, CORRIDOR_INVALID, CORRIDOR_OK, CORRIDOR_OK, CORRIDOR_INVALID, CORRIDOR_INVALID]
    assert got["offsets"].tolist() == [0, 4, 4, 4, 4, 5, 5, 5] and got["n_chain"].tolist() == [4, 0, 0, 0, 1, 0, 0]
    assert got["entry"].tolist() == [0, 1, 2, 3, 0] and (got["blocked_segment"] == -1).all() and (got["blocked_vox"] == INT32_MIN).all()
    for kw in ({"max_grow": -1}, {"max_grow": CORRIDOR_MAX_GROW + 1}, {"flags": 2}, {"min_clearance": float("nan")}, {"lo": (0, 0, 0)}):
        with pytest.raises(ValueError):
            free_box_model(obs, occ, [(1, 1, 1)], **kw)
        with pytest.raises(ValueError):
            corridor_model(obs, occ, w, off, **kw)


def test_header_library_and_bindings_agree():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    assert fiesta_amd.corridor_model is corridor_model and fiesta_amd.free_box_model is free_box_model and fiesta_amd.corridor_chain is corridor_chain
    names = ("fiesta_hip_free_boxes", "fiesta_hip_free_boxes_dev", "fiesta_hip_path_corridor", "fiesta_hip_path_corridor_dev")
    assert all(n in _lib.declared_symbols() for n in names)
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    for n in names:
        assert n in lib._fiesta_signatures and getattr(lib, n) is not None
    text = open(_lib.HEADER_PATH).read()
    for struct, mirror in (("fiesta_hip_free_boxes_result", _lib.FreeBoxesResult), ("fiesta_hip_corridor_result", _lib.CorridorResult)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[.*?\]", "", n).strip(" *") for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(_lib.FreeBoxesResult) == 5 * C.sizeof(C.c_void_p) and C.sizeof(_lib.CorridorResult) == 9 * C.sizeof(C.c_void_p)
    for name, value in (("CORRIDOR_THROUGH_UNKNOWN", CORRIDOR_THROUGH_UNKNOWN), ("CORRIDOR_MAX_GROW", CORRIDOR_MAX_GROW),
                        ("CORRIDOR_STOP_BLOCKED", CORRIDOR_STOP_BLOCKED), ("CORRIDOR_STOP_EDGE", CORRIDOR_STOP_EDGE),
                        ("CORRIDOR_STOP_LIMIT", CORRIDOR_STOP_LIMIT), ("FREE_BOX_OK", FREE_BOX_OK), ("FREE_BOX_OUTSIDE", FREE_BOX_OUTSIDE),
                        ("FREE_BOX_BLOCKED", FREE_BOX_BLOCKED), ("CORRIDOR_OK", CORRIDOR_OK), ("CORRIDOR_INVALID", CORRIDOR_INVALID),
                        ("CORRIDOR_BLOCKED", CORRIDOR_BLOCKED)):
        assert re.search(r"#define FIESTA_HIP_%s (\d+)" % name, text).group(1) == str(value), name
        assert getattr(fiesta_amd, name) == value
    block = re.search(r"---- free-space corridors.*?#define FIESTA_HIP_CORRIDOR_THROUGH_UNKNOWN", text, re.S).group(0)
    assert "Guarantees" in block and "fiesta_amd.corridor_model" in block and "LIMIT (3)" in block


def test_argument_rules_are_checked_before_any_device_use():
    """every whole-call error that needs no map is refused, with its own message, before the handle is looked at; nothing is written"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd import _lib
    lib = fiesta_amd.load()
    box3 = (C.c_int32 * 3)(0, 0, 0)
    vox = (C.c_int32 * 6)(1, 1, 1, 2, 2, 2)
    off = (C.c_int64 * 2)(0, 2)
    bad_off = (C.c_int64 * 3)(0, 2, 1)
    out = (C.c_int64 * 12)(*([77] * 12))
    fres = _lib.FreeBoxesResult(C.cast(out, C.c_void_p), None, None, None, None)
    cres = _lib.CorridorResult(C.cast(out, C.c_void_p), None, None, None, None, None, None, None, None)
    nan = float("nan")
    #        lo    hi    seeds n  clearance max_grow flags result          the message names
    free = [(None, None, vox, 2, 0.0, 4, 0, None, "result"),
            (None, None, vox, 2, nan, 4, 0, fres, "NaN"),
            (box3, None, vox, 2, 0.0, 4, 0, fres, "lo and hi"),
            (None, box3, vox, 2, 0.0, 4, 0, fres, "lo and hi"),
            (None, None, vox, 2, 0.0, -1, 0, fres, "max_grow"),
            (None, None, vox, 2, 0.0, 257, 0, fres, "max_grow"),
            (None, None, vox, 2, 0.0, 4, 2, fres, "flag"),
            (None, None, vox, -1, 0.0, 4, 0, fres, "negative"),
            (None, None, None, 2, 0.0, 4, 0, fres, "seeds"),
            (box3, box3, vox, 2, 0.25, 256, 1, fres, "null map")]              # nothing wrong but the missing map
    for fn in (lib.fiesta_hip_free_boxes, lib.fiesta_hip_free_boxes_dev):
        for lo, hi, s, n, clr, mg, flags, res, word in free:
            st = fn(None, lo, hi, s, n, clr, mg, flags, None if res is None else C.byref(res))
            assert st == 1, (word, st)                                          # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    #        lo    hi    wp   n_wp offsets n_paths clearance max_grow flags capacity result
    path = [(None, None, vox, 2, off, 1, 0.0, 4, 0, 0, None, "result"),
            (None, None, vox, 2, off, 1, 0.0, 4, 0, 0, _lib.CorridorResult(), "offsets"),
            (None, None, vox, 2, off, 1, nan, 4, 0, 0, cres, "NaN"),
            (box3, None, vox, 2, off, 1, 0.0, 4, 0, 0, cres, "lo and hi"),
            (None, None, vox, 2, off, 1, 0.0, 257, 0, 0, cres, "max_grow"),
            (None, None, vox, 2, off, 1, 0.0, 4, 4, 0, cres, "flag"),
            (None, None, vox, -2, off, 1, 0.0, 4, 0, 0, cres, "negative"),
            (None, None, vox, 2, off, -1, 0.0, 4, 0, 0, cres, "negative"),
            (None, None, None, 2, off, 1, 0.0, 4, 0, 0, cres, "waypoints_vox"),
            (None, None, vox, 2, off, 1, 0.0, 4, 0, -1, cres, "capacity"),
            (None, None, vox, 2, None, 1, 0.0, 4, 0, 0, cres, "offsets is null"),
            (None, None, vox, 2, off, 1, 0.0, 0, 1, 9, cres, "null map")]
    for fn in (lib.fiesta_hip_path_corridor, lib.fiesta_hip_path_corridor_dev):
        for lo, hi, w, nw, o, n, clr, mg, flags, cap, res, word in path:
            st = fn(None, lo, hi, w, nw, o, n, clr, mg, flags, cap, None if res is None else C.byref(res))
            assert st == 1, (word, st)
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    # bad offsets are a whole-call error of the host variant alone (the device variant cannot read them)
    assert lib.fiesta_hip_path_corridor(None, None, None, vox, 2, bad_off, 2, 0.0, 4, 0, 0, C.byref(cres)) == 1
    assert "non-decreasing" in lib.fiesta_hip_last_error().decode()
    assert lib.fiesta_hip_path_corridor(None, None, None, vox, 1, off, 1, 0.0, 4, 0, 0, C.byref(cres)) == 1
    assert "n_waypoints" in lib.fiesta_hip_last_error().decode()
    assert lib.fiesta_hip_path_corridor_dev(None, None, None, vox, 2, bad_off, 2, 0.0, 4, 0, 0, C.byref(cres)) == 1
    assert "null map" in lib.fiesta_hip_last_error().decode()
    assert all(v == 77 for v in out)


def test_corridor_kernels_spill_nothing_and_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_free_boxes" in k or "k_corridor_" in k}
    for kernel in ("k_free_boxes", "k_corridor_count", "k_corridor_write"):
        assert sum(kernel in k for k in res) == 2, (kernel, sorted(res))          # the dense and the hash-block source
    for k, v in res.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
