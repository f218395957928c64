"""The site tour of the C++ drop-in class (include/fiesta/ESDFMap.h: SiteTour).

CPU: examples/frontier_tour.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- the
sites, the order, the legs, the statuses, every restart's length and the info -- equal the same chain through the Python class on
the same scene, and fiesta_amd.tour_model on the matrix that chain produced.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO = ("n_visited", "length", "nn_length", "best_restart", "moves", "capped")


def build_example(tmp):
    import __graft_entry__ as g
    g.build_hip()
    exe = os.path.join(str(tmp), "frontier_tour")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frontier_tour.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "struct SiteTourResult {" in src
    assert ("SiteTourResult SiteTour(const std::vector<int32_t> &cost, int32_t n, int32_t start = 0, bool closed = false, int32_t restarts = 64,\n"
            "                          uint64_t seed = 0, int32_t max_moves = 0, int64_t ld = 0)") in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route_and_the_model(hip_lib, tmp_path):
    from fiesta_amd import tour_model, view_ring
    from test_cpp_reach import example_scene
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    deg = np.pi / 180.0
    pose = []
    for y0, y1 in ((0, 13), (14, 26), (27, 39)):                             # the example's 3 x 2 boxes over y and z
        for z0, z1 in ((0, 9), (10, 19)):
            fv = m.FrontierViews((0, y0, z0), (39, y1, z1), connectivity=26, min_size=5, ring=view_ring([0.8, 1.6], 12, [0.0]), min_range=0.2,
                                 max_range=3.0, tan_h=np.tan(40.0 * deg), tan_v=np.tan(30.0 * deg), block_mask=3, view_clearance=0.3, min_visible=3)
            has = fv["best_view"] >= 0
            pose.append(np.floor((fv["best_pos"][has] - np.asarray(m.origin)) / m.resolution).astype(np.int32).reshape(-1, 3))
    pose = np.concatenate(pose)
    pose = np.unique(pose, axis=0)                                         # (sorted by x, then y, then z)
    sites = np.concatenate([np.array([(12, 20, 10)], np.int32), pose])
    assert out["sites"] == sites.tolist() and len(sites) >= 3
    cost = m.ReachMatrix(sites)["cost"]
    got = m.SiteTour(cost, restarts=64, seed=2024)
    want = tour_model(cost, restarts=64, seed=2024)
    mv = got["n_visited"]
    for r in (got, want):
        assert out["order"] == r["order"][:mv].tolist() and out["leg_cost"] == r["leg_cost"][:mv].tolist()
        assert (r["order"][mv:] == -1).all() and (r["leg_cost"][mv:] == -1).all()
        assert out["site_status"] == r["site_status"].tolist() and out["restart_length"] == r["restart_length"].tolist()
        assert all(out[k] == r[k] for k in INFO), [(k, out[k], r[k]) for k in INFO]
    assert 3 <= out["n_visited"] <= len(sites) and out["order"][0] == 0 and out["length"] == sum(out["leg_cost"]) <= out["nn_length"]
    assert out["capped"] == 0
    m.close()
