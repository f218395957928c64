"""The body queries of the C++ drop-in class (include/fiesta/ESDFMap.h: BodyQueryBatch, IsPoseFree).

CPU: examples/body_check.cpp compiles against the header with a plain host compiler.  GPU: what it prints for its 12 yaw angles
equals ESDFMap.BodyQuery on the same scene through the Python class (the poses are the quaternions the example printed, so no sine
or cosine is computed twice), and the bar passes the doorway lengthwise and not crosswise.
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
    exe = os.path.join(str(tmp), "body_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "body_check.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "typedef std::vector<std::array<double, 4>> BodySpheres;" in src and "struct BodyResult {" in src
    assert "BodyResult BodyQueryBatch(const BodySpheres &spheres, const std::vector<Eigen::Vector3d> &pos, " in src
    assert "bool IsPoseFree(const BodySpheres &spheres, const Eigen::Vector3d &pos, " in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    from test_cpp_skeleton import example_scene
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    rows = out["poses"]
    assert [r["yaw_deg"] for r in rows] == list(range(0, 180, 15)) and len(out["spheres"]) == 7
    m = example_scene()
    poses = np.array([out["position"] + r["quat"] for r in rows])
    got = m.BodyQuery(np.array(out["spheres"]), poses, out["margin"])
    for k, r in enumerate(rows):
        for name in ("min_clearance", "cost"):
            assert r[name] == got[name][k], (k, name, r[name], got[name][k])       # (%.17g round-trips a double)
        assert r["min_sphere"] == got["min_sphere"][k] and r["n_below"] == got["n_below"][k] and r["grad"] == got["grad"][k].tolist()
        assert r["passes"] == bool(got["min_clearance"][k] >= out["margin"])
    # lengthwise the bar goes through the doorway, crosswise its ends come within the margin of the door posts
    by_yaw = {r["yaw_deg"]: r for r in rows}
    assert by_yaw[0]["passes"] and by_yaw[0]["n_below"] == 0 and by_yaw[0]["cost"] == 0 and by_yaw[0]["min_clearance"] > 0.2
    assert not by_yaw[90]["passes"] and by_yaw[90]["n_below"] >= 2 and by_yaw[90]["cost"] > 0
    assert by_yaw[90]["min_sphere"] in (0, 6) and by_yaw[90]["min_clearance"] == min(r["min_clearance"] for r in rows)
    m.close()
