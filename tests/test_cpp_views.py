"""View coverage through the C++ drop-in class (include/fiesta/ESDFMap.h: ViewCoverage, GetFrontierViews).

CPU: examples/frontier_views.cpp compiles against the header with a plain host compiler.  GPU: the numbers it prints -- per view,
per frontier voxel and per cluster -- equal the Python class on the same scene with the ring and the sensor the example printed
(17 digits), and fiesta_amd.view_coverage_model on the same lists.
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
    exe = os.path.join(str(tmp), "frontier_views")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frontier_views.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "struct ViewCoverageResult {" in src and "struct FrontierViewSet {" in src
    assert "ViewCoverageResult ViewCoverage(const std::vector<Eigen::Vector3i> &vox, const std::vector<ViewPose> &views, const fiesta_hip_view_sensor &sensor," in src
    assert "FrontierViewSet GetFrontierViews(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, double min_clearance, int32_t connectivity, int32_t min_size," in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route_and_the_model(hip_lib, tmp_path):
    from fiesta_amd import view_coverage_model, view_ring
    from test_cpp_reach import example_scene
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["chain_ok"] is True
    ring = np.array(out["ring"], np.float64)
    assert ring.shape == (24, 5) and np.allclose(ring, view_ring([0.8, 1.6], 12, [0.0]), atol=1e-15)
    mn, mx, th, tv, clear = out["sensor"]
    sensor = dict(min_range=mn, max_range=mx, tan_h=th, tan_v=tv, block_mask=3, min_clearance=clear, min_visible=3)
    m = example_scene()
    fv, mask = m.GetFrontierVoxels()
    order = np.lexsort((fv[:, 2], fv[:, 1], fv[:, 0]))
    fv, mask = np.ascontiguousarray(fv[order]), np.ascontiguousarray(mask[order])
    cl = m.ClusterVoxels(fv, mask=mask, connectivity=26, min_size=5)
    got = m.ViewCoverage(fv, centroid=cl["centroid"], ring=ring, offsets=cl["offsets"], members=cl["members"], **sensor)
    f = m.download_field(("d2", "occ"))
    shape = m.grid_size
    all_vox = np.argwhere(np.ones(shape, bool)).astype(np.int32)
    want = view_coverage_model((f["d2"] >= 0).reshape(shape), f["occ"].reshape(shape) != 0, m.origin, m.resolution, fv, centroid=cl["centroid"], ring=ring,
                               offsets=cl["offsets"], members=cl["members"], dist=m.GetDistance(all_vox).reshape(shape), pos_range=m.pos_range, **sensor)
    assert out["frontier"] == len(fv) > 500 and out["n_clusters"] == cl["n_clusters"] >= 2
    for r in (got, want):
        for k in ("n_usable", "n_pairs", "pairs_in_view", "pairs_visible"):
            assert out[k] == r[k], k
        for k in ("best_view", "best_count", "n_visible", "cover_count"):
            assert out[k] == r[k].tolist(), k
    assert out["unseen"] == int((got["cover_count"] == 0).sum())
    # the scene shows the point of the call: some pose sees a good part of a frontier, none sees through the wall
    assert max(out["best_count"]) >= 10 and 0 < out["pairs_visible"] < out["pairs_in_view"] < out["n_pairs"] and out["unseen"] > 0
    m.close()
