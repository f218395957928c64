#!/usr/bin/env python3
"""The site tour (fiesta_hip_site_tour_dev) on tools/reach_matrix_bench.py's scene, next to the reach matrix call that feeds it.

Scene and sites: reach_matrix_bench.py's, word for word (bench.py's C2-partial map, the 128^3 box around the robot, the robot and
one site per split frontier cluster, capped at 32 and at 64 sites), clearance 0, connectivity 26.  Per cap the matrix is computed
once by ReachMatrixDevice and stays on the device; the tour call reads it there.  Per case, p50 over --steps repetitions after
--warmup (each call synchronises by itself):
  matrix_ms            the ReachMatrixDevice call that produced the matrix
  tour_ms[R]           SiteTourDevice, open path from the robot, R = 1, 64, 1024 restarts, every output written
and, from the calls' own info: the length against nn_length (the nearest-neighbour tour) and against restart 0 alone (nearest
neighbour plus local search: the R = 1 call), the moves per restart, the capped restarts, the best restart.
Checked, for every case: order, site_status, leg_cost, every restart_length and the info equal fiesta_amd.tour_model on the
downloaded matrix.
One JSON line; with --out DIR it is also written to DIR/tour_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/tour_bench.py` (a run of its own).
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
INFO = ("n_visited", "length", "best_restart", "nn_length", "moves", "capped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--caps", type=int, nargs="+", default=[32, 64], help="site counts")
    ap.add_argument("--restarts", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--split", type=int, default=16, help="grid on which large frontier clusters are cut, voxels")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="directory for tour_partial<grid>.json")
    args = ap.parse_args()
    import torch
    from fiesta_amd import tour_model
    from reach_matrix_bench import scene_and_sites
    dev = torch.device("cuda", 0)
    G = args.grid
    m, robot, lo, hi, _, _, _, all_sites = scene_and_sites(G, args.obstacles, args.split)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.steps):
            m.synchronize()
            t0 = time.perf_counter()
            fn()
            m.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    cases, checks = {}, {}
    for cap in args.caps:
        sites = np.ascontiguousarray(all_sites[:cap])
        n = len(sites)
        sd = torch.tensor(sites, dtype=torch.int32, device=dev)
        mat = torch.full((n * n,), -7, dtype=torch.int32, device=dev)
        outs = [torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        t_matrix = timed(lambda: m.ReachMatrixDevice(sd.data_ptr(), n, lo=lo, hi=hi, cost_dev_ptr=mat.data_ptr()))
        cost = mat.cpu().numpy().reshape(n, n)
        case = {"sites": n, "matrix_ms": t_matrix * 1e3, "tour": {}}
        for R in args.restarts:
            lens = torch.full((R,), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            info = {}

            def tour():
                info.update(m.SiteTourDevice(mat.data_ptr(), n, n, restarts=R, seed=args.seed, order_dev_ptr=outs[0].data_ptr(),
                                             site_status_dev_ptr=outs[1].data_ptr(), leg_cost_dev_ptr=outs[2].data_ptr(),
                                             restart_length_dev_ptr=lens.data_ptr()))

            t_tour = timed(tour)
            want = tour_model(cost, restarts=R, seed=args.seed)
            got = dict(zip(("order", "site_status", "leg_cost", "restart_length"), [a.cpu().numpy() for a in outs + [lens]]))
            checks[f"sites{n}_R{R}_equals_model"] = bool(all(np.array_equal(got[k], want[k]) for k in got) and all(info[k] == want[k] for k in INFO))
            case["tour"][str(R)] = {"tour_ms": t_tour * 1e3, "tour_over_matrix": t_tour / t_matrix, "moves_per_restart": info["moves"] / R,
                                    "first_restart_length": int(got["restart_length"][0]), **{k: info[k] for k in INFO}}
        cases[f"sites{n}"] = case
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    head = cases[f"sites{min(args.caps[0], len(all_sites))}"]["tour"][str(args.restarts[min(1, len(args.restarts) - 1)])]
    out = {"metric": "site_tour_over_reach_matrix", "value": head["tour_over_matrix"], "unit": "x", "scene": f"partial{G}", "grid": G, "revision": rev,
           "source_sha256": source_digest(), "robot": robot[0].tolist(), "seed": args.seed, "cases": cases, "steps": args.steps, "warmup": args.warmup,
           "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"tour_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if out["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
