"""Which engines an UpdateESDF tries (fiesta_amd/csrc/engine_choice.hpp: bulk_pays_model, choose_engines, cells_verdict) checked
on the CPU: tests/cpp/engine_choice_model.cpp compiles the very header dense_map.hip, hash_map.hip and shard_group.hip include.
The expected side is a transcription of the expressions DenseMap::update_esdf, DenseMap::bulk_pays_model and
DenseMap::cells_wanted held inline before the header existed (commit caf5a54, dense_map.hip 2196-2232, 2001-2008, 1550-1574),
written from that commit and not from the header.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "engine_choice_model.cpp")
LIB = os.path.join(HERE, "cpp", "libengine_choice_model.so")
HEADER = os.path.join(os.path.dirname(HERE), "fiesta_amd", "csrc", "engine_choice.hpp")

# include/fiesta_hip.h: FIESTA_HIP_NOTE_*
PARTLY_OBSERVED, SMALL_DELTA, SHARDED, ID_WRAP, ENGINE_PINNED = 0x0001, 0x0200, 0x1000, 0x2000, 0x4000


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HEADER)):
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    lib = C.CDLL(LIB)
    lib.engine_choice_bulk_pays.restype = C.c_int
    lib.engine_choice_bulk_pays.argtypes = [C.c_double] * 5
    lib.engine_choice_rows.restype = None
    lib.engine_choice_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.engine_choice_cells.restype = C.c_int
    lib.engine_choice_cells.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_longlong]
    return lib


# ---- the parent's expressions -------------------------------------------------------------------------------------------------
def parent_bulk_pays(delta, nocc, n, ft_last_ms, bulk_ratio):
    delta, nocc, n = float(delta), float(nocc), float(n)
    if bulk_ratio >= 0:
        return delta >= bulk_ratio * max(nocc, 1.0)
    updated = min(n, delta * n / max(nocc, 1.0))
    if delta <= 128 and ft_last_ms > 1.25 * n * 6e-9:
        return False
    return n <= 1.3e8 + 50.0 * updated


def parent_choice(ni, nd, nocc, observed, owned, n, engine, seed_only, sharded, wrap, gate_open, small_update, insert_cap, ft_last_ms,
                  bulk_ratio):
    """(try_levels, try_bulk, masked asked, notes) as update_esdf computed them; masked asked: everything ahead of `&& masked_eligible(ni, nd)`"""
    pays = lambda: parent_bulk_pays(ni + nd, nocc, n, ft_last_ms, bulk_ratio)   # noqa: E731  (the member bulk_pays)
    pinned = engine in (2, 4, 5)                                               # (bulk_pinned)
    notes = 0
    if observed != owned:
        notes |= PARTLY_OBSERVED
    if sharded:
        notes |= SHARDED
    if wrap:
        notes |= ID_WRAP
    if engine != 0:
        notes |= ENGINE_PINNED
    try_levels = (not seed_only and not sharded and not wrap and engine != 1 and
                  (engine == 3 or (not gate_open and ni + nd <= small_update and ni <= insert_cap)))
    try_bulk = gate_open and (pinned or pays())
    if gate_open and not try_bulk:
        notes |= SMALL_DELTA
    if not gate_open and not seed_only and observed < n and not pinned and not pays():
        notes |= SMALL_DELTA
    ask_masked = (not seed_only and not gate_open and not try_bulk and observed < n and
                  (engine == 6 or (not try_levels and (engine == 0 or pinned) and pays())))
    return int(try_levels), int(try_bulk), int(ask_masked), notes


def parent_cells_wanted(engine, fits, nocc, n, nn_skip, nn_last_ms, ft_last_ms, nn_last_nocc):
    """0: true; false by 1: engine or size, 2: density (the DENSITY note), 3: nn_skip_ (--nn_skip_, CELLS_BACKOFF), 4: timings (CELLS_BACKOFF)"""
    if engine == 4 or not fits:
        return 1
    if engine == 5:
        return 0
    if nocc * 15000 < n or nocc * 400 > n:
        return 2
    if nn_skip > 0:
        return 3
    if nn_last_ms > 0 and ft_last_ms > 0 and nn_last_ms > ft_last_ms and abs(nocc - nn_last_nocc) * 4 <= nn_last_nocc:
        return 4
    return 0


# ---- choose_engines ---------------------------------------------------------------------------------------------------------------
DELTAS = [(0, 1), (1, 0), (100, 28), (129, 0), (512, 0), (513, 0), (4096, 0), (4097, 0), (0, 5000)]


def sweep_rows():
    rows, left_out = [], 0
    for n in (64 ** 3, 512 ** 3, 640 ** 3):
        for engine, seed_only, sharded, wrap, gate_open, observed, owned, (ni, nd), nocc, ft, ratio in itertools.product(
                range(7), (0, 1), (0, 1), (0, 1), (0, 1), (n, n - 1), (n, n // 2), DELTAS, (1, 1000, n // 400),
                (0.0, 2.5 * n * 6e-9), (-1.0, 0.5)):
            # the gate is asked only on maps that are no shard and not being seeded, and engines 1 and 3 shut it (bulk_eligible)
            if gate_open and (seed_only or sharded or engine in (1, 3)):
                left_out += 1
                continue
            rows.append((ni, nd, nocc, observed, owned, n, engine, seed_only, sharded, wrap, gate_open, 4096, 512, ft, ratio))
    return rows, left_out


def test_choose_engines_equals_the_inline_choice_on_the_whole_sweep(model):
    rows, left_out = sweep_rows()
    assert (len(rows), left_out) == (85536, 59616)   # 145152 rows in the product; the caller never forms the ones left out
    a = np.array(rows, np.float64)
    assert np.array_equal(a[:, :13], np.rint(a[:, :13])) and a[:, :13].max() < 2.0 ** 53
    got = np.empty((len(rows), 4), np.int32)
    model.engine_choice_rows(a.ctypes.data, len(rows), got.ctypes.data)
    want = np.array([parent_choice(*r) for r in rows], np.int32)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, [(rows[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    # (the sweep does reach every output both ways, and SMALL_DELTA by both of its routes)
    for k in range(3):
        assert 0 < want[:, k].sum() < len(rows)
    small = (want[:, 3] & SMALL_DELTA) != 0
    assert (small & (a[:, 10] == 1)).any() and (small & (a[:, 10] == 0)).any() and not small.all()


def test_bulk_pays_model(model):
    n = 512 ** 3
    cases = [(d, nocc, nn, ft, r) for d in (0.5, 1, 100, 128, 129, 5000, 1e6) for nocc in (0, 0.25, 1, 1000, 335544.32)
             for nn in (64 ** 3, n, 640 ** 3, 1024 ** 3) for ft in (0.0, 1.25 * nn * 6e-9, 2.5 * nn * 6e-9) for r in (-1.0, 0.0, 0.02, 0.5)]
    for c in cases:
        assert bool(model.engine_choice_bulk_pays(*c)) == parent_bulk_pays(*c), c
    assert {parent_bulk_pays(*c) for c in cases} == {True, False}


# ---- cells_verdict --------------------------------------------------------------------------------------------------------------------
def test_cells_verdict_equals_cells_wanted(model):
    cases = []
    for nocc in (1, 7, 655, 20000):   # the density bounds: nocc * 15000 == n -/+ 1 and nocc * 400 == n +/- 1, and the bounds themselves
        for n in (nocc * 15000 - 1, nocc * 15000, nocc * 15000 + 1, nocc * 400 - 1, nocc * 400, nocc * 400 + 1):
            cases += [(e, 1, nocc, n, skip, 0.0, 0.0, -1) for e in range(7) for skip in (0, 1)]
    n = 64 ** 3
    for last in (400, 401, 1):      # the timing back-off: |nocc - nn_last_nocc| * 4 == nn_last_nocc, and one past it on either side
        for nocc in (last + last // 4, last + last // 4 + 1, last - last // 4, last - last // 4 - 1, last):
            for nn_ms, ft_ms in ((0.5, 0.4), (0.4, 0.5), (0.4, 0.4), (0.5, 0.0), (0.0, 0.4)):
                cases += [(e, fits, nocc, n, skip, nn_ms, ft_ms, last) for e in (0, 2, 4, 5, 6) for fits in (0, 1) for skip in (0, 3)]
    seen = set()
    for c in cases:
        want = parent_cells_wanted(*c)
        assert model.engine_choice_cells(*c) == want, c
        seen.add(want)
    assert seen == {0, 1, 2, 3, 4}
    # the bounds, spelled out: in range at exactly 15000 and 400 voxels per obstacle, out of it one voxel beyond either
    in_range = lambda nocc, n: model.engine_choice_cells(0, 1, nocc, n, 0, 0.0, 0.0, -1) == 0   # noqa: E731
    assert in_range(7, 7 * 15000) and not in_range(7, 7 * 15000 + 1) and in_range(7, 7 * 400) and not in_range(7, 7 * 400 - 1)
    backs_off = lambda nocc: model.engine_choice_cells(0, 1, nocc, n, 0, 0.5, 0.4, 400) == 4   # noqa: E731
    assert backs_off(500) and not backs_off(501) and backs_off(300) and not backs_off(299)
