"""The articulated body queries of the C++ drop-in class (include/fiesta/ESDFMap.h: ArticulatedQueryBatch, IsConfigurationFree).

CPU: examples/arm_check.cpp compiles against the header with a plain host compiler.  GPU: what it prints for its 12 shoulder angles
equals ESDFMap.ArticulatedQuery on the same scene through the Python class (the configurations are the frame poses the example
printed, so no sine or cosine is computed twice), and the arm reaches through the doorway at some angles and not at others.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp):
    import __graft_entry__ as g
    g.build_hip()
    exe = os.path.join(str(tmp), "arm_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "arm_check.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "struct ArticulatedResult {" in src
    assert ("ArticulatedResult ArticulatedQueryBatch(const BodySpheres &spheres, const std::vector<int32_t> &sphere_frame, int n_frames,\n"
            "                                          const std::vector<double> &frame_poses, double margin) {") in src
    assert ("bool IsConfigurationFree(const BodySpheres &spheres, const std::vector<int32_t> &sphere_frame, int n_frames,\n"
            "                           const std::vector<double> &frame_poses, double margin) {") in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    from test_cpp_skeleton import example_scene
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    rows = out["configurations"]
    assert [r["shoulder_deg"] for r in rows] == list(range(-60, 60, 10)) and out["n_frames"] == 3
    assert out["sphere_frame"] == [0, 0, 0, 1, 1, 1, 2, 2] and len(out["spheres"]) == 8
    m = example_scene()
    poses = np.array([r["frame_poses"] for r in rows])
    assert poses.shape == (12, 3, 7)
    got = m.ArticulatedQuery(np.array(out["spheres"]), np.array(out["sphere_frame"], np.int32), poses, out["margin"])
    for k, r in enumerate(rows):
        for name in ("min_clearance", "cost"):
            assert r[name] == got[name][k], (k, name, r[name], got[name][k])       # (%.17g round-trips a double)
        assert r["min_sphere"] == got["min_sphere"][k] and r["n_below"] == got["n_below"][k]
        assert r["frame_clearance"] == got["frame_clearance"][k].tolist() and r["frame_cost"] == got["frame_cost"][k].tolist()
        assert r["frame_grad"] == got["frame_grad"][k].tolist()
        assert r["passes"] == bool(got["min_clearance"][k] >= out["margin"])
        assert r["min_clearance"] == min(r["frame_clearance"])
    # pointed at the doorway the arm reaches through it; swung to the side the hand comes within the margin of a door post
    by_angle = {r["shoulder_deg"]: r for r in rows}
    assert any(r["passes"] for r in rows) and not all(r["passes"] for r in rows)
    assert by_angle[-10]["passes"] and by_angle[-10]["n_below"] == 0 and by_angle[-10]["cost"] == 0 and by_angle[-10]["min_clearance"] > 0.25
    assert not by_angle[20]["passes"] and by_angle[20]["n_below"] >= 1 and by_angle[20]["cost"] > 0
    assert by_angle[20]["min_sphere"] in (6, 7) and by_angle[20]["frame_cost"][2] > 0 and by_angle[20]["frame_cost"][0] == 0
    m.close()
