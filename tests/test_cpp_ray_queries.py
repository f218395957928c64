"""The ray queries of the C++ drop-in class (include/fiesta/ESDFMap.h: RayQueryBatch, RayQuery, IsSegmentFree).

CPU: examples/line_of_sight.cpp compiles against the header with a plain host compiler.  GPU: the example checks by itself that the
one-ray RayQuery and IsSegmentFree agree with the batch call on each of its rays; its printed numbers are compared here with the
Python class on the same scene and rays, and with fiesta_amd.ray_query_model on the map's dump.
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
    exe = os.path.join(str(tmp), "line_of_sight")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "line_of_sight.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    for sig in ("void RayQueryBatch(const double *start, const double *end, int64_t n, int32_t stop_mask, const fiesta_hip_ray_result &result)",
                "RayHit RayQuery(const Eigen::Vector3d &start, const Eigen::Vector3d &end, int32_t stop_mask)",
                "bool IsSegmentFree(const Eigen::Vector3d &a, const Eigen::Vector3d &b)"):
        assert sig in src, sig


def centre(x, y, z):
    return [-4.0 + (x + 0.5) * 0.2, -4.0 + (y + 0.5) * 0.2, 0.0 + (z + 0.5) * 0.2]


def example_rays():
    """the rays of examples/line_of_sight.cpp, in its order and arithmetic"""
    a, b = [], []
    for y in range(2, 39, 3):
        for z in range(1, 20, 3):
            a.append(centre(6, 20, 10)), b.append(centre(36, y, z))
    for y in range(12, 29, 2):
        a.append(centre(12.25, y, 10.25)), b.append(centre(26.5, 40 - y, 9.75))
        a.append(centre(22, y, 6)), b.append(centre(28, y, 14))
    a.append(centre(10, 20, 10)), b.append(centre(45, 20, 10))
    a.append(centre(8, 20, 10)), b.append(centre(8, 20, 10))
    return np.array(a), np.array(b)


def example_scene():
    """the scene of examples/line_of_sight.cpp through the Python class"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap((-4.0, -4.0, 0.0), 0.2, (8.0, 8.0, 4.0))
    assert m.grid_size == (40, 40, 20)
    m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80)
    m.SetOriginalRange()
    V = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(20), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    d = V - (5, 20, 10)
    cone = (V[:, 0] >= 6) & (V[:, 0] <= 30) & (d[:, 1] ** 2 + d[:, 2] ** 2 <= d[:, 0] ** 2) & ((d ** 2).sum(1) <= 28 * 28)
    hit = (V[:, 0] == 30) | ((V[:, 0] == 18) & (V[:, 1] >= 19) & (V[:, 1] <= 21))
    for cycle in range(3):
        if cycle == 0:
            m.SetOccupancy(V[cone & ~hit].astype(np.int32), 0, want_ret=False)
        m.SetOccupancy(V[cone & hit].astype(np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)
    return m


@pytest.mark.gpu
def test_example_output_and_facade_agreement(hip_lib, tmp_path):
    from fiesta_amd import ray_query_model
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, "the example's own check failed: RayQuery / IsSegmentFree disagree with RayQueryBatch"
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert "agree with the batch: yes" in run.stdout and out["agree"] == 1
    m = example_scene()
    a, b = example_rays()
    los, view = m.RayQuery(a, b, 7), m.RayQuery(a, b, 1)
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    for mask, got in ((7, los), (1, view)):
        want = ray_query_model(obs, occ, m.origin, 0.2, a, b, mask, pos_range=m.pos_range)
        for k in want:
            ok = ~np.isnan(want[k]) if k == "hit_dist" else np.ones(len(a), bool)
            assert np.array_equal(got[k][ok], want[k][ok]) and (k != "hit_dist" or np.isnan(got[k][~ok]).all()), (mask, k)
    assert out["rays"] == len(a) == 13 * 7 + 18 + 2
    assert out["clear"] == int((los["hit_index"] < 0).sum())
    assert [out["occupied"], out["unknown"], out["outside"]] == [int((los["hit_class"] == c).sum()) for c in (1, 2, 4)]
    assert out["gain"] == int(view["counts"][:, 2].sum())
    d = view["hit_dist"]
    assert out["depth_mm"] == int(sum(int(np.floor(v * 1000.0 + 0.5)) for v in d[~np.isnan(d)]))
    # the scene shows each answer: free segments, the pillar and the wall, the cone's unknown rim, the map's end
    assert out["clear"] >= 3 and out["occupied"] >= 5 and out["unknown"] >= 5 and out["gain"] > 0 and out["depth_mm"] > 0
    assert los["hit_index"][-1] == -1 and los["n_visited"][-1] == 1            # zero length, in free space
    assert view["hit_vox"][-2].tolist() == [18, 20, 10] and view["counts"][-2].tolist() == [8, 0, 0, 0]     # the pillar
    m.close()
