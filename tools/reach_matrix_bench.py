#!/usr/bin/env python3
"""The reach matrix (fiesta_hip_reach_matrix_dev) on tools/reach_bench.py's map, against the route that existed before it: one
fiesta_hip_reach_field_dev call per site.

Scene (built here, nothing is read from disk): bench.py's C2-partial map -- 512^3 @ 0.1 m, 27 % of its 32^3-voxel blocks never
observed, 50 000 scattered obstacles -- and the box of 128^3 voxels around the free voxel nearest to the centre, the robot.
Sites: the robot, then the cheapest member (by travel cost from the robot, clearance 0) of each frontier cluster of the box
(connectivity 26, at least 5 voxels), the clusters in order of that cost, capped at 32 and at 64 sites.  The unobserved blocks of
this map touch one another, so its frontier is a few very large surfaces (the JSON's frontier_clusters_unsplit: 2 in this box);
like a planner that splits large frontiers before it places viewpoints, the tool cuts them on the grid of --split voxels (16: 205
clusters in this box; 32, the map's own block size, leaves 38) before clustering -- voxels on two sides of a grid plane are not
adjacent.  Connectivity 26, clearance 0
and 0.3 m, every array resident on the device.  Per case, p50 over --steps repetitions after --warmup, the three routes taken in
turn inside every repetition (each call synchronises by itself):
  matrix_ms      the square matrix in one call, max_fields = 0: one bitmap, the floods side by side
  matrix_b1_ms   the same call with max_fields = 1: one bitmap, the floods one after the other -- what the shared bitmap alone saves
  loop_ms        a loop of ReachFieldDevice calls, one per site, the sites as targets, each writing its row of the matrix
  mask_ms        the matrix call without sources: k_reach_mask and the call's fixed cost
and, counted by the calls themselves: rounds and tile visits of the matrix call and summed over the loop.
Checked: three rows of usable sites (the first, the middle, the last) equal the loop's rows, for every case.
One JSON line; with --out DIR it is also written to DIR/reach_matrix_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/reach_matrix_bench.py` (a run of its own).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
INF = 2 ** 31 - 1


def scene_and_sites(G, obstacles, split):
    """the map, the robot, the box and the sites of the docstring (also tools/tour_bench.py's): (m, robot, lo, hi, frontier voxels,
    unsplit cluster count, the clusters in order of cost, the sites)"""
    from reach_bench import build_partial
    m, _ = build_partial(G, int(round(obstacles * (G / 512.0) ** 3)))
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    c0 = max(G // 2 - 32, 0)                       # (the nearest free voxel lies well inside the central 64^3)
    free = np.argwhere((obs & ~occ)[c0:c0 + 64, c0:c0 + 64, c0:c0 + 64]) + c0
    robot = free[np.argmin(((free - G // 2) ** 2).sum(1))].astype(np.int32).reshape(1, 3)
    half = min(64, G // 2)
    lo = np.clip(robot[0] - half, 0, G - 1)
    hi = np.clip(lo + 2 * half - 1, 0, G - 1)
    # the sites: the frontier clusters of the box, each by its cheapest member, nearest cluster first
    fv, _ = m.GetFrontierVoxels(lo, hi)
    fv = np.ascontiguousarray(fv[np.lexsort((fv[:, 2], fv[:, 1], fv[:, 0]))])
    key = m.ReachField(robot, lo, hi, targets=fv, want_cost=False)["target_cost"]
    unsplit = m.ClusterVoxels(fv, connectivity=26, min_size=5)["n_clusters"]
    # (the cluster call sees coordinates only: one voxel of room per grid plane crossed makes the two sides of a plane non-adjacent)
    cl = m.ClusterVoxels(np.ascontiguousarray(fv + fv // split), key=key, connectivity=26, min_size=5)
    order = [k for k in np.lexsort((np.arange(len(cl["key_min"])), cl["key_min"])) if cl["key_argmin"][k] >= 0]
    all_sites = np.concatenate([robot, fv[[int(cl["key_argmin"][k]) for k in order]]]).astype(np.int32)
    return m, robot, lo, hi, fv, unsplit, order, all_sites


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--caps", type=int, nargs="+", default=[32, 64], help="site counts")
    ap.add_argument("--split", type=int, default=16, help="grid on which large frontier clusters are cut, voxels")
    ap.add_argument("--out", default=None, help="directory for reach_matrix_partial<grid>.json")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    G = args.grid
    m, robot, lo, hi, fv, unsplit, order, all_sites = scene_and_sites(G, args.obstacles, args.split)

    def timed_in_turn(fns):
        """p50 per function; inside every repetition each function runs once, in order"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        ts = [[] for _ in fns]
        for _ in range(args.steps):
            for k, fn in enumerate(fns):
                m.synchronize()
                t0 = time.perf_counter()
                fn()
                m.synchronize()
                ts[k].append(time.perf_counter() - t0)
        return [statistics.median(t) for t in ts]

    cases, checks = {}, {}
    for cap in args.caps:
        sites = np.ascontiguousarray(all_sites[:cap])
        n = len(sites)
        sd = torch.tensor(sites, dtype=torch.int32, device=dev)
        mat = torch.full((n * n,), -7, dtype=torch.int32, device=dev)
        mat1 = torch.full((n * n,), -7, dtype=torch.int32, device=dev)
        rows = torch.full((n * n,), -7, dtype=torch.int32, device=dev)
        status = torch.full((n,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for clearance in (0.0, 0.3):
            info, info1, loop = {}, {}, {}

            def matrix():
                info.update(m.ReachMatrixDevice(sd.data_ptr(), n, lo=lo, hi=hi, min_clearance=clearance, cost_dev_ptr=mat.data_ptr(),
                                                source_status_dev_ptr=status.data_ptr()))

            def matrix_b1():
                info1.update(m.ReachMatrixDevice(sd.data_ptr(), n, lo=lo, hi=hi, min_clearance=clearance, max_fields=1, cost_dev_ptr=mat1.data_ptr()))

            def single_calls():
                loop["rounds"] = loop["tile_visits"] = 0
                for s in range(n):
                    r = m.ReachFieldDevice(sd.data_ptr() + 12 * s, 1, lo, hi, sd.data_ptr(), n, min_clearance=clearance,
                                           target_cost_dev_ptr=rows.data_ptr() + 4 * n * s)
                    loop["rounds"] += r["rounds"]
                    loop["tile_visits"] += r["tile_visits"]

            def mask_only():
                m.ReachMatrixDevice(0, 0, lo=lo, hi=hi, min_clearance=clearance)

            t_matrix, t_loop, t_b1, t_mask = timed_in_turn([matrix, single_calls, matrix_b1, mask_only])
            a, a1, b, st = mat.cpu().numpy().reshape(n, n), mat1.cpu().numpy().reshape(n, n), rows.cpu().numpy().reshape(n, n), status.cpu().numpy()
            usable = np.flatnonzero(st == 0)
            picked = [int(usable[0]), int(usable[len(usable) // 2]), int(usable[-1])]
            name = f"sites{n}_clear{clearance}"
            checks[name + "_rows_equal_loop"] = bool(all(np.array_equal(a[s], b[s]) for s in picked))
            checks[name + "_batch_width_changes_nothing"] = bool(np.array_equal(a, a1))
            finite = (a >= 0) & (a != INF)
            cases[name] = {
                "sites": n, "sites_usable": int(len(usable)), "matrix_ms": t_matrix * 1e3, "matrix_b1_ms": t_b1 * 1e3, "loop_ms": t_loop * 1e3,
                "mask_ms": t_mask * 1e3, "matrix_over_loop": t_matrix / t_loop, "matrix_b1_over_loop": t_b1 / t_loop,
                "fields": info["fields"], "batches": info["batches"], "rounds": info["rounds"], "tile_visits": info["tile_visits"],
                "b1_rounds": info1["rounds"], "b1_tile_visits": info1["tile_visits"], "loop_rounds": loop["rounds"],
                "loop_tile_visits": loop["tile_visits"], "n_traversable": info["n_traversable"], "finite_entries": int(finite.sum()),
                "unreached_entries": int((a == INF).sum()), "checked_rows": picked, "box": [info["box_lo"], info["box_hi"]]}
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    head = cases[f"sites{min(args.caps[0], len(all_sites))}_clear0.0"]
    out = {"metric": "reach_matrix_over_single_calls", "value": head["matrix_over_loop"], "unit": "x", "scene": f"partial{G}", "grid": G,
           "revision": rev, "source_sha256": source_digest(), "robot": robot[0].tolist(), "frontier_voxels": int(len(fv)),
           "frontier_clusters_unsplit": int(unsplit), "split": args.split, "frontier_clusters": int(len(order)), "cases": cases, "steps": args.steps, "warmup": args.warmup, "checks": checks,
           "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"reach_matrix_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if out["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
