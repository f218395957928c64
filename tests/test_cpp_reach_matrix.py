"""The reach matrix of the C++ drop-in class (include/fiesta/ESDFMap.h: ReachMatrix).

CPU: examples/reach_matrix.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- the
number of sites, the matrix's checksum, its INT32_MAX and -1 entries, the greedy tour and its length -- equal the same chain through
the Python class on the same scene, and the matrix equals fiesta_amd.reach_matrix_model on the map's dump.
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
    exe = os.path.join(str(tmp), "reach_matrix")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "reach_matrix.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    sig = ("fiesta_hip_reach_matrix_info ReachMatrix(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, const std::vector<Eigen::Vector3i> &sources,\n"
           "                                           const std::vector<Eigen::Vector3i> &targets, double min_clearance, int32_t connectivity, int32_t flags,\n"
           "                                           std::vector<int32_t> *cost, std::vector<int32_t> *source_status = nullptr, int32_t max_fields = 0)")
    assert sig in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


def greedy_tour(cost):
    """nearest neighbour from site 0 over finite entries; among equals the lower site index"""
    n = len(cost)
    tour, length = [0], 0
    while True:
        row = cost[tour[-1]].astype(np.int64)
        ok = [j for j in range(n) if j not in tour and 0 <= row[j] < INF]
        if not ok:
            return tour, length
        best = min(ok, key=lambda j: (row[j], j))
        length += int(row[best])
        tour.append(best)


@pytest.mark.gpu
def test_example_output_equals_the_python_route_and_the_model(hip_lib, tmp_path):
    from fiesta_amd import reach_matrix_model
    from test_cpp_reach import example_scene
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    fv, _ = m.GetFrontierVoxels()
    fv = np.ascontiguousarray(fv[np.lexsort((fv[:, 2], fv[:, 1], fv[:, 0]))])
    robot = np.array([(12, 20, 10)], np.int32)
    key = m.ReachField(robot, targets=fv, want_cost=False)["target_cost"]
    clusters = m.ClusterVoxels(fv, key=key, connectivity=26, min_size=5)
    arg = clusters["key_argmin"]
    sites = np.concatenate([robot, fv[arg[arg >= 0]]])
    got = m.ReachMatrix(sites)
    cost = got["cost"]
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    want = reach_matrix_model(obs, occ, sites)
    for k in ("cost", "source_status", "source_reached"):
        assert np.array_equal(got[k], want[k]), k
    assert all(got[k] == want[k] for k in ("box_lo", "box_hi", "n_traversable", "n_sources_used"))
    finite = (cost >= 0) & (cost != INF)
    assert out["sites"] == len(sites) >= 3
    assert out["checksum"] == int(cost[finite].astype(np.int64).sum()) > 0
    assert out["unreached"] == int((cost == INF).sum()) and out["blocked"] == int((cost == -1).sum()) == 0
    tour, length = greedy_tour(cost)
    assert out["tour"] == tour and out["tour_length"] == length > 0
    # the scene shows the point: the pocket's site is a place to be (0 on the diagonal) that no other site reaches
    assert np.array_equal(cost, cost.T) and (np.diag(cost) == 0).all()
    pocket = [s for s in range(len(sites)) if sites[s][0] >= 33]
    assert len(pocket) == 1 and pocket[0] not in tour and len(tour) == len(sites) - 1
    assert out["unreached"] == 2 * (len(sites) - 1)
    m.close()
