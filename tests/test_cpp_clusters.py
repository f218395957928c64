"""The voxel clusters of the C++ drop-in class (include/fiesta/ESDFMap.h: ClusterVoxels, GetFrontierClusters).

CPU: examples/frontier_clusters.cpp compiles against the header with a plain host compiler.  GPU: the clusters it prints -- sizes,
boxes, centroids (all 17 digits), masks, cheapest members and their costs -- equal the Python class on the same scene and
fiesta_amd.cluster_model on the same list.
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
    exe = os.path.join(str(tmp), "frontier_clusters")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frontier_clusters.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "struct VoxelClusters {" in src
    assert ("VoxelClusters ClusterVoxels(const std::vector<Eigen::Vector3i> &vox, const std::vector<uint8_t> *mask = nullptr,\n"
            "                              const std::vector<int32_t> *key = nullptr, int32_t connectivity = 26, int32_t min_size = 1)") in src
    assert "VoxelClusters GetFrontierClusters(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, double min_clearance, int32_t connectivity," in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route_and_the_model(hip_lib, tmp_path):
    from fiesta_amd import cluster_model
    from test_cpp_reach import example_scene
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    fv, mask = m.GetFrontierVoxels()
    order = np.lexsort((fv[:, 2], fv[:, 1], fv[:, 0]))
    fv, mask = np.ascontiguousarray(fv[order]), np.ascontiguousarray(mask[order])
    cost = m.ReachField([(12, 20, 10)], targets=fv, want_cost=False)["target_cost"]
    got = m.ClusterVoxels(fv, mask=mask, key=cost, connectivity=26, min_size=5)
    want = cluster_model(fv, mask=mask, key=cost, connectivity=26, min_size=5, resolution=m.resolution, origin=m.origin)
    assert out["frontier"] == len(fv) > 500 and len(out["clusters"]) == out["n_clusters"] == want["n_clusters"] >= 2
    for r in (got, want):
        for k in ("n_clusters", "n_dropped_clusters", "n_members", "largest"):
            assert out[k] == r[k], k
        for c, row in enumerate(out["clusters"]):
            for k in ("size", "root", "mask_or", "key_min", "key_argmin"):
                assert row[k] == int(r[k][c]), (c, k)
            assert row["box_lo"] == r["box_lo"][c].tolist() and row["box_hi"] == r["box_hi"][c].tolist()
            assert np.array(row["centroid"], np.float64).view(np.int64).tolist() == r["centroid"][c].view(np.int64).tolist(), (c, "centroid bits")
    # the scene shows the point of the call: the pocket behind the wall is a frontier of its own, and out of reach
    far = [row for row in out["clusters"] if row["box_lo"][0] >= 33]
    assert len(far) == 1 and far[0]["key_min"] == INF
    near = [c for c, row in enumerate(out["clusters"]) if row["key_min"] != INF]
    assert len(near) == len(out["path_moves"]) >= 1 and all(v > 0 for v in out["path_moves"])
    goals = fv[[out["clusters"][c]["key_argmin"] for c in near]]
    paths = m.ReachPaths(goals, connectivity=26, shortcut=True)
    assert out["path_moves"] == paths["n_moves"].tolist() and out["path_waypoints"] == int(paths["offsets"][-1])
    m.close()
