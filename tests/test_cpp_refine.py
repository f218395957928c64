"""Path refinement through the C++ drop-in class (include/fiesta/ESDFMap.h: RefinePaths).

CPU: examples/path_refine.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- how many
corridors are whole, the iterations run, J before and after, the refined waypoints of the longest path -- equal the Python class on
the same scene, with the bounds fiesta_amd.corridor_bounds computes (the example computes them itself).
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
    exe = os.path.join(str(tmp), "path_refine")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "path_refine.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert ("RefineSet RefinePaths(const std::vector<double> &waypoints, const std::vector<int64_t> &offsets, const std::vector<double> &bounds, "
            "const RefineParams &p)") in src


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    import fiesta_amd
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
    cor = m.PathCorridor(paths["waypoints_vox"], paths["offsets"], max_grow=8)
    bounds, ok = fiesta_amd.corridor_bounds(paths["waypoints_vox"], paths["offsets"], cor, inset=0.2 * 2.0 ** -20)
    w, off = paths["waypoints_pos"], paths["offsets"]
    got = m.PathRefine(w, off, bounds, margin=0.8, w_obstacle=1.0, w_smooth=2.0, alpha=0.02, max_step=0.05, tolerance=0.0, iterations=32)
    valid = got["status"] == 0
    assert out["paths"] == len(fv) > 500 and out["waypoints"] == len(w) and out["ok"] == int(ok.sum()) > 400
    assert out["valid"] == int(valid.sum()) and out["iterations"] == int(got["iterations"][valid].sum()) > 32
    assert out["n_below"] == int(got["n_below"][valid].sum())
    assert out["moved"] == int((got["waypoints"] != w).sum()) > 1000 and out["largest_move"] == float(np.abs(got["waypoints"] - w).max()) > 0.05
    # (the example adds in path order, as cumsum does)
    assert out["cost_before"] == float(np.cumsum(got["cost"][valid, 0])[-1]) and out["cost_after"] == float(np.cumsum(got["cost"][valid, 1])[-1])
    assert out["cost_after"] < out["cost_before"]
    longest = int(np.argmax(np.diff(off)))                                   # (the first of the longest, as the example takes it)
    assert out["longest"] == fv[longest].tolist()
    assert out["longest_pos"] == got["waypoints"][off[longest]:off[longest + 1]].reshape(-1).tolist()
    assert out["longest_min_dist"] == float(got["min_dist"][longest])
    m.close()
