"""Cluster splitting through the C++ drop-in class (include/fiesta/ESDFMap.h: SplitClusters).

CPU: examples/frontier_split.cpp compiles against the header with a plain host compiler.  GPU: the parts it prints -- counts, sizes,
parents, centroids (all 17 digits) and a checksum over parent, depth, size, root and box of every part -- equal the Python class on
the same scene and fiesta_amd.split_model on the same list.
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
    exe = os.path.join(str(tmp), "frontier_split")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frontier_split.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def checksum(r):
    """FNV-1a over the little-endian int64 of (parent, depth, size, root, box_lo / box_hi per axis) of every part, in part order"""
    h = 1469598103934665603
    for k in range(len(r["size"])):
        row = [r["parent"][k], r["depth"][k], r["size"][k], r["root"][k]]
        for a in range(3):
            row += [r["box_lo"][k][a], r["box_hi"][k][a]]
        for x in row:
            for b in int(x).to_bytes(8, "little", signed=True):
                h = ((h ^ b) * 1099511628211) % 2 ** 64
    return h


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "struct ClusterParts {" in src
    assert ("ClusterParts SplitClusters(const std::vector<Eigen::Vector3i> &vox, const std::vector<int64_t> &offsets, const std::vector<int64_t> &members,\n"
            "                             const std::vector<uint8_t> *mask = nullptr, const std::vector<int32_t> *key = nullptr, int32_t max_size = 0,\n"
            "                             int32_t max_extent = 0, int32_t max_depth = FIESTA_HIP_SPLIT_MAX_DEPTH)") in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route_and_the_model(hip_lib, tmp_path):
    from fiesta_amd import split_model
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
    cl = m.ClusterVoxels(fv, mask=mask, connectivity=26, min_size=5)
    got = m.SplitClusters(fv, cl["offsets"], cl["members"], mask=mask, max_size=96, max_extent=12)
    want = split_model(fv, cl["offsets"], cl["members"], mask=mask, max_size=96, max_extent=12, resolution=m.resolution, origin=m.origin)
    assert out["frontier"] == len(fv) > 500 and out["n_clusters"] == cl["n_clusters"] >= 2
    assert out["n_parts"] == want["n_parts"] > out["n_clusters"] and out["n_oversize"] == 0 and out["status"] == 0
    for r in (got, want):
        for k in ("n_parts", "n_members", "n_split_clusters", "n_oversize", "largest", "status"):
            assert out[k] == r[k], k
        assert out["depth"] == r["deepest"]
        assert out["sizes"] == r["size"].tolist() and out["parents"] == r["parent"].tolist() and out["checksum"] == checksum(r)
        assert np.array(out["centroids"], np.float64).view(np.int64).tolist() == r["centroid"].view(np.int64).tolist(), "centroid bits"
    assert max(out["sizes"]) <= 96 and ((want["box_hi"] - want["box_lo"]).max() + 1) <= 12
    m.close()
