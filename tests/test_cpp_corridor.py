"""The corridor calls of the C++ drop-in class (include/fiesta/ESDFMap.h: FreeBoxes, PathCorridor).

CPU: examples/corridor.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- how many
corridors are whole, how many boxes and voxels they hold, the boxes of the longest corridor, the robot's own box -- are compared
with the Python class on the same scene, and with fiesta_amd.corridor_model / free_box_model on the map's dump.
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
    exe = os.path.join(str(tmp), "corridor")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "corridor.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "FreeBoxSet FreeBoxes(const std::vector<Eigen::Vector3i> &seeds, int32_t max_grow = 16, double min_clearance = 0.0, int32_t flags = 0," in src
    assert "CorridorSet PathCorridor(const std::vector<int32_t> &waypoints_vox, const std::vector<int64_t> &offsets, int32_t max_grow = 16," in src


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    from fiesta_amd import corridor_model, free_box_model
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    robot = [(12, 20, 10)]
    fv, _ = m.GetFrontierVoxels()
    fv = np.array(sorted(fv.tolist()), np.int32)
    m.ReachField(robot, want_cost=False)
    paths = m.ReachPaths(fv, shortcut=True, max_span=64)
    got = m.PathCorridor(paths["waypoints_vox"], paths["offsets"], max_grow=8)
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    kw = dict(resolution=0.2, origin=(-4.0, -4.0, 0.0))
    want = corridor_model(obs, occ, paths["waypoints_vox"], paths["offsets"], max_grow=8, **kw)
    for k in want:
        assert np.array_equal(got[k].view(np.int64) if got[k].dtype == np.float64 else got[k],
                              want[k].view(np.int64) if want[k].dtype == np.float64 else want[k]), k
    n = len(fv)
    assert out["frontier"] == n > 500 and out["reached"] == int((paths["status"] == 0).sum()) > 400
    assert [out["ok"], out["blocked"], out["invalid"]] == [int((want["status"] == s).sum()) for s in (0, 2, 1)] and out["ok"] == n
    b = want["boxes"].astype(np.int64)
    assert out["boxes"] == len(b) >= out["reached"] and out["volume"] == int(np.prod(b[:, 3:] - b[:, :3] + 1, axis=1).sum())
    assert out["chain"] == int(want["n_chain"].sum())
    longest = int(np.argmax(np.diff(want["offsets"])))                       # (the first of the longest, as the example takes it)
    assert out["longest"] == fv[longest].tolist() and out["longest_boxes"] == b[want["offsets"][longest]:want["offsets"][longest + 1]].tolist()
    assert len(out["longest_boxes"]) >= 2
    own = free_box_model(obs, occ, robot, max_grow=8, **kw)
    assert out["robot_box"] == own["box"][0].tolist() and out["robot_volume"] == int(own["volume"][0]) and out["robot_corner"] == float(own["box_pos"][0, 3])
    mine = m.FreeBoxes(robot, max_grow=8)
    assert np.array_equal(mine["box"], own["box"]) and np.array_equal(mine["box_pos"], own["box_pos"])
    m.close()
