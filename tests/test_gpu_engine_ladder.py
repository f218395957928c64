"""DenseMap::update_esdf as a ladder (dense_map.hip; the choice itself: engine_choice.hpp, tests/test_engine_choice.py): every
rung an update can be made to take on maps of 64^3 and 96^3 voxels, in the scenes by which test_gpu_cells.py,
test_gpu_incremental.py, test_gpu_masked.py, test_gpu_path_notes.py and test_gpu_level_grid.py reach them.  At each step the
statistics that say which engines ran and why -- (bulk, cells, levels, masked, nn_incremental, nn_failed > 0, sorted(why)) --
must equal a literal table, recorded on commit caf5a54 (update_esdf with the choice inline); where the map is fully observed
the field must be the exact transform as well.

The level engine hands an update on twice: `auto` after a window (600 voxels that changed, 300 of them inserts), and engine 3
behind a grid that gives up at its first barrier (level_tuning, as in test_gpu_level_grid.py) -- its own lists hold 2^20 entries,
more than these maps have voxels, so no update here can outgrow them.  Not reached at these sizes: the SMALL_DELTA note (a
transform always pays below 1.3e8 voxels) and seed_only, which is the sharded driver's (test_gpu_sharded.py)."""
import numpy as np
import pytest

from scenarios import P_DEFAULT
from test_gpu_cells import check_exact, free, make_map, occupy
from test_gpu_path_notes import scatter

pytestmark = pytest.mark.gpu

ONE = np.array([[80, 80, 80]], np.int32)

#        bulk cells levels masked nn_incremental nn_failed > 0  why
TABLE = {
    "cells clean": (1, 1, 0, 0, 0, False, []),
    "incremental": (1, 1, 0, 0, 1, False, []),
    "density": (1, 0, 0, 0, 0, False, ["density"]),
    "cells failed": (1, 0, 0, 0, 0, True, ["cells_failed", "engine_pinned"]),
    "cells not retried": (1, 0, 0, 0, 0, False, ["cells_backoff", "engine_pinned"]),
    "masked": (1, 1, 0, 1, 0, False, ["partly_observed"]),
    "levels": (0, 0, 1, 0, 0, False, ["partly_observed"]),
    "partial window": (0, 0, 1, 0, 0, False, ["partial_window", "partly_observed"]),
    "window history": (0, 0, 0, 0, 0, False, ["levels_gave_up", "partly_observed", "window_history"]),
    "levels gave up": (0, 0, 0, 0, 0, False, ["engine_pinned", "levels_gave_up"]),
    "rounds pinned": (0, 0, 0, 0, 0, False, ["engine_pinned"]),
}


def row(st):
    return (st["bulk"], st["cells"], st["levels"], st["masked"], st["nn_incremental"], st["nn_failed"] > 0, sorted(st["why"]))


def rungs():
    """(rung, statistics of the UpdateESDF that took it, the map, its shape if every voxel is observed), one after the other"""
    import fiesta_amd
    # fully observed, the library's choice: the cell transform, its incremental form on one voxel more, the envelope passes
    shape = (64, 64, 64)
    m = make_map(shape, "auto")
    occupy(m, scatter(shape, 200, 1))
    yield "cells clean", m.UpdateESDF(), m, shape
    occupy(m, np.array([[5, 5, 5]], np.int32))   # (one voxel dirties 180 cells at the most: under half of this map's 512)
    yield "incremental", m.UpdateESDF(), m, shape
    occupy(m, scatter(shape, 3000, 2))           # more than a 400th of the voxels
    yield "density", m.UpdateESDF(), m, shape
    m.close()
    # 216 obstacles in one corner: in the density range, but most cells have nothing within reach -- failed cells, then back-off
    shape = (96, 96, 96)
    m = make_map(shape, "bulk")
    occupy(m, np.array([(x, y, z) for x in range(6) for y in range(6) for z in range(6)], np.int32) + 3)
    yield "cells failed", m.UpdateESDF(), m, shape
    occupy(m, ONE, 6)
    yield "cells not retried", m.UpdateESDF(), m, shape
    m.close()
    # a third of the map never observed: the masked transform, the level engine on one voxel, a window, and its history on an
    # update the level engine starts and the rounds finish
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, tuple((s - 0.5) * 0.1 for s in shape), update_engine="auto")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((0, 0, 0), (95, 95, 63), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    S = scatter((96, 96, 64), 700, 5)
    occupy(m, S)
    yield "masked", m.UpdateESDF(), m, None
    occupy(m, np.array([[40, 40, 10]], np.int32))
    yield "levels", m.UpdateESDF(), m, None
    m.SetUpdateRange((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    occupy(m, np.array([[20, 20, 20]], np.int32))
    yield "partial window", m.UpdateESDF(), m, None
    m.SetOriginalRange()
    free(m, S[:300])
    occupy(m, scatter((96, 96, 64), 300, 6))
    yield "window history", m.UpdateESDF(), m, None
    m.close()
    # engine 3 and an update it hands on: the rounds finish it; engine 1: the rounds alone
    shape = (64, 64, 64)
    m = make_map(shape, "levels")
    m.level_tuning(-1, 0)
    occupy(m, scatter(shape, 400, 7))
    yield "levels gave up", m.UpdateESDF(), m, shape
    m.close()
    m = make_map(shape, "rounds")
    occupy(m, scatter(shape, 200, 3))
    yield "rounds pinned", m.UpdateESDF(), m, shape
    m.close()


def test_every_rung_runs_the_engines_it_ran_before(hip_lib):
    seen = []
    for rung, st, m, shape in rungs():
        assert row(st) == TABLE[rung], (rung, row(st), st)
        if shape:
            check_exact(m, shape)
        seen.append(rung)
    assert seen == list(TABLE)
