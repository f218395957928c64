"""bench.py as a comparison tool: a plain run times exactly --steps steps and reports ms_per_step, --dump-outputs writes the
last timed step's field (float arrays, at most 64 MB, identical from run to run with the same arguments), --full adds the
self-check, the parity quote and the CPU baseline.  C2's shape on a 64^3 grid so that each run takes seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--grid", "64", "--warmup", "1"]

pytestmark = pytest.mark.gpu


def bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def load_dir(d):
    out = {}
    for f in sorted(os.listdir(d)):
        assert f.endswith(".npy"), f
        out[f] = np.load(os.path.join(d, f))
    return out


def test_plain_run_dumps_the_same_outputs_every_time(tmp_path):
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        line = bench("--steps", "3", "--dump-outputs", str(d))
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["metric"] == "esdf_updated_voxels_per_sec" and line["unit"] == "voxels/s" and line["higher_is_better"] is True
        for moved in ("cpu_baseline", "verify", "parity", "scatter_full_update"):
            assert moved not in line, moved
        runs.append(load_dir(d))
    a, b = runs
    assert set(a) == {"sample_voxels.npy", "sample_distance.npy", "sample_occupancy.npy", "mid_plane_distance.npy"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name, v in a.items():
        assert v.dtype in (np.float32, np.float64), name
        assert np.array_equal(v, b[name]), name
    assert a["mid_plane_distance.npy"].shape == (64, 64)
    occ = a["sample_occupancy.npy"]
    assert np.all((occ == 0) | (occ == 1)) and occ.sum() > 0
    d = a["sample_distance.npy"]
    assert np.all(d[occ == 1] == 0) and np.all(d[occ == 0] > 0)


def test_full_run_still_carries_the_checks():
    line = bench("--steps", "2", "--full", "--cpu-grid", "32")
    assert line["steps"] == 2
    assert line["verify"]["sampled"] > 0 and line["verify"]["mismatches"] == 0
    assert "pinned_by" in line["parity"]
    assert line["scatter_full_update"]["updated_voxels"] > 0
    assert line["cpu_baseline"]["value"] > 0
