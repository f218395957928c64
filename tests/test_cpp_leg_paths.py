"""The leg paths of the C++ drop-in class (include/fiesta/ESDFMap.h: LegPaths, TourRoute).

CPU: examples/tour_route.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- the
sites, the order, every leg's ends, status, moves, cost and waypoints (voxels and f64 positions), the corridor offsets -- equal
TourRoute of the Python class on the same scene, and fiesta_amd.leg_paths_model on that map's own dump.
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
    exe = os.path.join(str(tmp), "tour_route")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "tour_route.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "struct LegPathsResult {" in src and "struct TourRouteResult {" in src
    assert ("LegPathsResult LegPaths(const std::vector<int32_t> &from, const std::vector<int32_t> &to, bool shortcut = false, int32_t max_span = 4096,\n"
            "                          const std::vector<Eigen::Vector3i> *to_vox = nullptr)") in src
    assert "TourRouteResult TourRoute(const std::vector<Eigen::Vector3i> &sites, int32_t start = 0, bool closed = false" in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route_and_the_model(hip_lib, tmp_path):
    from fiesta_amd import leg_paths_model
    from test_cpp_reach import example_scene
    from test_gpu_reach_paths import dump
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    sites = np.array(out["sites"], np.int32)                               # (tests/test_cpp_tour.py holds the sites to the Python chain)
    assert len(sites) >= 3 and out["n_sources"] == len(sites) and out["connectivity"] == 26
    route = m.TourRoute(sites, restarts=64, seed=2024, shortcut=True, max_span=64)
    k = route["n_visited"]
    legs = route["legs"]
    assert out["order"] == route["order"][:k].tolist() and out["tour_leg_cost"] == route["leg_cost"][:k].tolist() and out["length"] == route["length"]
    assert out["from"] == legs["from"].tolist() == out["order"][:-1] and out["to"] == legs["to"].tolist() == out["order"][1:] and k >= 3
    obs, occ, _ = dump(m)
    want = leg_paths_model(obs, occ, sites, legs["from"], to=legs["to"], path_flags=1, max_span=64, origin=m.origin, resolution=m.resolution)
    for r in (legs, want):
        for key in ("offsets", "status", "n_moves", "cost"):
            assert out[key] == r[key].tolist(), key
        assert out["waypoints_vox"] == r["waypoints_vox"].reshape(-1).tolist()
        assert np.array_equal(np.array(out["waypoints_pos"], np.float64), r["waypoints_pos"].reshape(-1))       # (%.17g: the f64 bits)
    assert set(out["status"]) == {0} and out["cost"] == out["tour_leg_cost"][1:] and sum(out["cost"]) == out["length"]
    assert 2 * (k - 1) <= out["offsets"][-1] < sum(out["n_moves"]) + k - 1                   # pulled tight, not the staircase
    assert out["corridor_offsets"] == m.PathCorridor(legs["waypoints_vox"], legs["offsets"], max_grow=8)["offsets"].tolist()
    m.close()
