"""The reachability query of the C++ drop-in class (include/fiesta/ESDFMap.h: ReachField).

CPU: examples/reach.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- frontier
voxels, how many of them the flood reaches with and without a clearance, the nearest one and its cost -- are compared with the Python
class on the same scene, and with fiesta_amd.reach_model on the map's dump.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1


def build_example(tmp):
    import __graft_entry__ as g
    g.build_hip()
    exe = os.path.join(str(tmp), "reach")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "reach.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    sig = ("fiesta_hip_reach_info ReachField(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, const std::vector<Eigen::Vector3i> &seeds,\n"
           "                                   const std::vector<Eigen::Vector3i> &targets, double min_clearance, int32_t connectivity, int32_t flags,\n"
           "                                   std::vector<int32_t> *target_cost, std::vector<int32_t> *cost = nullptr)")
    assert sig in src


def example_scene():
    """the scene of examples/reach.cpp through the Python class"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap((-4.0, -4.0, 0.0), 0.2, (8.0, 8.0, 4.0))
    assert m.grid_size == (40, 40, 20)
    m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80)
    m.SetOriginalRange()
    V = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(20), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    d = V - (5, 20, 10)
    cone = (V[:, 0] >= 6) & (V[:, 0] <= 30) & (d[:, 1] ** 2 + d[:, 2] ** 2 <= d[:, 0] ** 2) & ((d ** 2).sum(1) <= 28 * 28)
    hit = (V[:, 0] == 30) | ((V[:, 0] == 18) & (V[:, 1] >= 19) & (V[:, 1] <= 21))
    pocket = (V[:, 0] >= 33) & (V[:, 0] <= 36) & (V[:, 1] >= 18) & (V[:, 1] <= 21) & (V[:, 2] >= 8) & (V[:, 2] <= 11)
    for cycle in range(3):
        if cycle == 0:
            m.SetOccupancy(V[(cone & ~hit) | pocket].astype(np.int32), 0, want_ret=False)
        m.SetOccupancy(V[cone & hit].astype(np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    from fiesta_amd import reach_model
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    robot = [(12, 20, 10)]
    fv, _ = m.GetFrontierVoxels()
    got = m.ReachField(robot, targets=fv)
    clear = m.ReachField(robot, targets=fv, min_clearance=0.3, want_cost=False)
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    V = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(20), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    dist = m.GetDistance(V).reshape(m.grid_size)
    for r, c in ((got, 0.0), (clear, 0.3)):
        want = reach_model(obs, occ, robot, dist, min_clearance=c, targets=fv)
        assert np.array_equal(r["target_cost"], want["target_cost"])
        assert all(r[k] == want[k] for k in ("n_traversable", "n_reached", "max_cost", "n_seeds_used", "box_lo", "box_hi"))
        if r["cost"] is not None:
            assert np.array_equal(r["cost"], want["cost"])
    tc = got["target_cost"]
    ok = (tc >= 0) & (tc != INF)
    assert out["frontier"] == len(fv) > 500
    assert out["reachable"] == int(ok.sum()) and out["out_of_reach"] == int((tc == INF).sum())
    assert out["reachable_clear"] == int(((clear["target_cost"] >= 0) & (clear["target_cost"] != INF)).sum())
    assert out["cost_sum"] == int(tc[ok].astype(np.int64).sum())
    assert [out["n_reached"], out["n_traversable"], out["max_cost"]] == [got["n_reached"], got["n_traversable"], got["max_cost"]]
    # the nearest reachable frontier voxel; among equals the smallest (x, y, z)
    cand = fv[ok][tc[ok] == tc[ok].min()]
    assert out["nearest_cost"] == int(tc[ok].min()) > 0 and out["nearest"] == sorted(cand.tolist())[0]
    # the scene shows the point of the call: the pocket's frontier voxels are free, and out of reach
    assert out["out_of_reach"] >= 40 and 0 < out["reachable_clear"] < out["reachable"] < out["frontier"]
    in_pocket = (fv[:, 0] >= 33)
    assert in_pocket.any() and (tc[in_pocket] == INF).all() and (tc[~in_pocket] < INF).all()
    m.close()
