"""Corridor bounds through the C++ drop-in class (include/fiesta/ESDFMap.h: CorridorBounds).

CPU: examples/corridor_bounds.cpp compiles against the header with a plain host compiler.  GPU: the example's printed numbers -- how
many corridors are whole, how many rows are void, a checksum over the bit patterns of all bounds, the refined waypoints of the
longest path -- equal the Python class on the same scene.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from test_cpp_reach import example_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp):
    import __graft_entry__ as g
    g.build_hip()
    exe = os.path.join(str(tmp), "corridor_bounds")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "corridor_bounds.cpp"), "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
    return exe


def test_example_compiles_with_host_compiler_only(tmp_path):
    assert os.path.exists(build_example(tmp_path))
    src = open(os.path.join(ROOT, "include", "fiesta", "ESDFMap.h"), encoding="utf-8").read()
    assert ("BoundsSet CorridorBounds(const std::vector<int32_t> &waypoints_vox, const std::vector<int64_t> &offsets, const CorridorSet &corridor, "
            "double inset = -1 /* resolution·2⁻²⁰ */, bool void_broken = false)") in src


@pytest.mark.gpu
def test_example_output_equals_the_python_route(hip_lib, tmp_path):
    exe = build_example(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-3000:], run.stderr)
    assert run.returncode == 0
    out = json.loads(run.stdout.strip().splitlines()[-1])
    m = example_scene()
    fv, _ = m.GetFrontierVoxels()
    fv = np.array(sorted(fv.tolist()), np.int32)
    m.ReachField([(12, 20, 10)], want_cost=False)
    paths = m.ReachPaths(fv)
    wv, w, off = paths["waypoints_vox"], paths["waypoints_pos"], paths["offsets"]
    cor = m.PathCorridor(wv, off, lo=(0, 0, 0), hi=(39, 39, 13), max_grow=8)
    bnd = m.CorridorBounds(wv, off, cor, void_broken=True)
    got = m.PathRefine(w, off, bnd["bounds"], margin=0.8, w_obstacle=1.0, w_smooth=2.0, alpha=0.02, max_step=0.05, tolerance=0.0, iterations=32)
    assert out["paths"] == len(fv) > 500 and out["waypoints"] == len(w) and out["boxes"] == len(cor["entry"])
    assert out["ok"] == int(bnd["ok"].sum()) > 100 and out["ok"] < out["paths"]
    nan_rows = np.isnan(bnd["bounds"][:, 0])
    assert out["nan_rows"] == int(nan_rows.sum()) > 0 and np.array_equal(nan_rows, np.repeat(bnd["ok"] == 0, np.diff(off)))
    assert out["boxed"] == int((bnd["box"] >= 0).sum())
    assert out["checksum"] == int(np.ascontiguousarray(bnd["bounds"]).view(np.uint64).sum(dtype=np.uint64))
    assert out["valid"] == int((got["status"] == 0).sum()) and out["moved"] == int((got["waypoints"] != w).sum()) > 1000
    longest = int(np.argmax(np.diff(off)))                                   # (the first of the longest, as the example takes it)
    assert out["longest"] == fv[longest].tolist() and out["longest_ok"] == int(bnd["ok"][longest])
    assert out["longest_pos"] == got["waypoints"][off[longest]:off[longest + 1]].reshape(-1).tolist()
    m.close()
