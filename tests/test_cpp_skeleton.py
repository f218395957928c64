"""The skeleton voxels of the C++ drop-in class (include/fiesta/ESDFMap.h: GetSkeletonVoxels).

CPU: examples/skeleton.cpp compiles against the header with a plain host compiler.  GPU: the clusters of skeleton voxels it prints
-- sizes, boxes, masks, narrowest members and their squared clearances -- equal the Python class on the same scene, and the
skeleton itself equals fiesta_amd.skeleton_model on that map's own dump.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (40, 40, 20)


def build_example(tmp):
    import __graft_entry__ as g
    g.build_hip()
    exe = os.path.join(str(tmp), "skeleton")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "skeleton.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def example_scene():
    """the scene of examples/skeleton.cpp through the Python class"""
    import fiesta_amd
    m = fiesta_amd.ESDFMap((-4.0, -4.0, 0.0), 0.2, (8.0, 8.0, 4.0))
    assert m.grid_size == SHAPE
    m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80)
    m.SetOriginalRange()
    V = np.stack(np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    hit = (V[:, 0] == 20) & ((V[:, 1] <= 17) | (V[:, 1] >= 22))
    for cycle in range(3):
        if cycle == 0:
            m.SetOccupancy(V[~hit], 0, want_ret=False)
        m.SetOccupancy(V[hit], 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h")).read()
    assert "struct SkeletonVoxels {" in src
    assert ("SkeletonVoxels GetSkeletonVoxels(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, int32_t min_sep2, "
            "double min_clearance = 0.0)") in src
    assert "hip/hip_runtime" not in src and "hipStream" not in src          # header-only, free of HIP types


@pytest.mark.gpu
def test_example_output_equals_the_python_route_and_the_model(hip_lib, tmp_path):
    from fiesta_amd import cluster_model, skeleton_model
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    f = m.download_field(("d2", "coc", "occ"))
    want_sk = skeleton_model(f["d2"].reshape(SHAPE), f["coc"].reshape(SHAPE + (3,)), f["occ"].reshape(SHAPE), 9)
    sk = m.GetSkeletonVoxels(min_sep2=9)
    order = np.lexsort((sk["vox"][:, 2], sk["vox"][:, 1], sk["vox"][:, 0]))
    sk = {k: np.ascontiguousarray(sk[k][order]) for k in ("vox", "mask", "d2", "sep2")}
    for k in ("vox", "mask", "d2", "sep2"):
        assert np.array_equal(sk[k], want_sk[k]), k
    got = m.ClusterVoxels(sk["vox"], mask=sk["mask"], key=sk["d2"], connectivity=26, min_size=5)
    want = cluster_model(sk["vox"], mask=sk["mask"], key=sk["d2"], connectivity=26, min_size=5, resolution=m.resolution, origin=m.origin)
    assert out["skeleton"] == len(sk["vox"]) > 500 and len(out["clusters"]) == out["n_clusters"] == want["n_clusters"] >= 1
    for r in (got, want):
        for k in ("n_clusters", "n_dropped_clusters", "n_members", "largest"):
            assert out[k] == r[k], k
        for c, row in enumerate(out["clusters"]):
            for k in ("size", "root", "mask_or", "key_min", "key_argmin"):
                assert row[k] == int(r[k][c]), (c, k)
            assert row["box_lo"] == r["box_lo"][c].tolist() and row["box_hi"] == r["box_hi"][c].tolist()
            assert row["narrowest"] == sk["vox"][row["key_argmin"]].tolist() and row["sep2"] == int(sk["sep2"][row["key_argmin"]])
    # the scene shows the point of the call: the largest piece runs through the doorway, and its narrowest member stands in it,
    # half way between the two door posts (y = 17 and y = 22), two voxels from either
    big = max(out["clusters"], key=lambda row: row["size"])
    assert big["box_lo"][0] < 20 < big["box_hi"][0]
    assert big["narrowest"][0] == 20 and big["narrowest"][1] in (19, 20) and big["key_min"] == 4 and big["sep2"] >= 25
    m.close()
