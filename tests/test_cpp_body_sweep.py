"""The body sweeps of the C++ drop-in class (include/fiesta/ESDFMap.h: BodySweepBatch, IsMotionFree).

CPU: examples/body_sweep.cpp compiles against the header with a plain host compiler.  GPU: what it prints for its three motions
equals ESDFMap.BodySweep on the same scene through the Python class (the poses are the ones the example printed, so no sine or
cosine is computed twice); the bar passes the doorway lengthwise and when it turns in the rooms, and not when it turns in the doorway.
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
    exe = os.path.join(str(tmp), "body_sweep")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "body_sweep.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "typedef std::vector<std::array<double, 7>> BodyPoses;" in src and "struct SweepResult {" in src
    assert "SweepResult BodySweepBatch(const BodySpheres &spheres, const BodyPoses &waypoints, const std::vector<int64_t> &offsets, " in src
    assert "bool IsMotionFree(const BodySpheres &spheres, const BodyPoses &waypoints, double step, double margin)" in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    from test_cpp_skeleton import example_scene
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    rows = out["motions"]
    assert [r["name"] for r in rows] == ["lengthwise", "turn in rooms", "turn in doorway"] and len(out["spheres"]) == 7
    m = example_scene()
    poses = np.array([p for r in rows for p in r["poses"]])
    off = np.concatenate([[0], np.cumsum([len(r["poses"]) for r in rows])])
    got = m.BodySweep(np.array(out["spheres"]), poses, off, out["step"], out["margin"])
    centre = m.PathClearance(poses[:, :3], off, out["step"], out["margin"])
    for k, r in enumerate(rows):
        assert r["min_clearance"] == got["min_clearance"][k] and r["centre_min_dist"] == centre["min_dist"][k]   # (%.17g round-trips a double)
        for name in ("n_samples", "min_sample", "min_sphere", "first_below", "first_below_sphere", "n_below"):
            assert r[name] == got[name][k], (k, name, r[name], got[name][k])
        assert r["free"] == bool(got["first_below"][k] < 0)
    by_name = {r["name"]: r for r in rows}
    for name in ("lengthwise", "turn in rooms"):
        assert by_name[name]["free"] and by_name[name]["n_below"] == 0 and by_name[name]["min_clearance"] > 0.2
    turn = by_name["turn in doorway"]
    assert not turn["free"] and turn["n_below"] >= 3 and turn["min_clearance"] < out["margin"] and turn["min_sphere"] in (0, 6)
    assert 0 < turn["first_below"] < turn["min_sample"] < turn["n_samples"] - 1
    assert by_name["turn in rooms"]["n_samples"] > by_name["lengthwise"]["n_samples"]          # turning takes samples of its own
    assert all(r["centre_min_dist"] > out["margin"] for r in rows)                             # the point robot sees nothing
    m.close()
