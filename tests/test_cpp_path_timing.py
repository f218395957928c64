"""Path timing through the C++ drop-in class (include/fiesta/ESDFMap.h: PathTiming, GetPathDuration).

CPU: examples/path_timing.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- the
paths and samples timed, the total duration, the paths below the margin, the frontier voxels nearest in time and in length -- equal
the Python class on the same scene.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from test_cpp_reach import example_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp):
    import __graft_entry__ as g
    g.build_hip()
    exe = os.path.join(str(tmp), "path_timing")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "path_timing.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "TimingSet PathTiming(const std::vector<double> &waypoints, const std::vector<int64_t> &offsets, const TimingParams &p)" in src
    assert "double GetPathDuration(const std::vector<Eigen::Vector3d> &waypoints, const TimingParams &p" in src


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-3000:], run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    fv, _ = m.GetFrontierVoxels()
    fv = np.array(sorted(fv.tolist()), np.int32)
    m.ReachField([(12, 20, 10)], want_cost=False)
    paths = m.ReachPaths(fv)
    got = m.PathTiming(paths["waypoints_pos"], paths["offsets"], step=0.2, margin=0.3, v_max=2.0, v_min=0.1, a_max=1.5, corner_dev=0.05)
    timed = (got["status"] == 0) & (got["n_samples"] >= 2)
    idx = np.flatnonzero(timed)
    assert out["paths"] == len(fv) > 500 and out["timed"] == len(idx) > 100
    assert out["samples"] == int(got["n_samples"][timed].sum()) > 1000
    assert out["duration"] == float(np.cumsum(got["duration"][timed])[-1]) > 0            # (the example adds in path order, as cumsum does)
    assert out["below"] == int((got["n_below"][timed] > 0).sum())
    by_time, by_length = idx[np.argmin(got["duration"][idx])], idx[np.argmin(got["length"][idx])]   # (ties to the lowest index)
    assert out["nearest_time"] == fv[by_time].tolist() and out["nearest_time_duration"] == float(got["duration"][by_time])
    assert out["nearest_length"] == fv[by_length].tolist() and out["nearest_length_length"] == float(got["length"][by_length])
    m.close()
