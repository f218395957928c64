#!/usr/bin/env python3
"""The legs of a tour (fiesta_hip_leg_paths_dev) on tools/reach_matrix_bench.py's scene, next to the two calls that feed them and
against the route that existed before: per leg one fiesta_hip_reach_field_dev plus one fiesta_hip_reach_paths_dev.

Scene and sites: those of tools/reach_matrix_bench.py (bench.py's C2-partial map, 512^3 @ 0.1 m, the box of 128^3 voxels around the
robot, the robot and the cheapest member of each frontier cluster), capped at 32 and at 64 sites; connectivity 26, clearance 0,
every array resident on the device.  The legs are those of the open tour from the robot (64 restarts), from = order, to = order + 1:
views into the order array where the tour call left it.  Per case, p50 over --steps repetitions after --warmup, every route taken in
turn inside every repetition, each timed by a host clock around work that ends in a synchronise of the map's stream:
  matrix_ms          ReachMatrixDevice, the square matrix: it leaves the batch of floods that the leg call descends
  tour_ms            SiteTourDevice on that matrix
  legs_raw_ms        LegPathsDevice, every voxel a waypoint (the serial descent alone: no visibility walk is made)
  legs_shortcut_ms   LegPathsDevice, SHORTCUT with max_span 4096 (the descent and the visibility walks)
  old_raw_ms, old_shortcut_ms   the route that existed before, with the order read on the host: per leg ReachFieldDevice(seeds = the
                     leg's source, target = the leg's target) and ReachPathsDevice on the field it retains, written at the leg's offset
A leg call is count + scan + write; the buffers are sized once, outside the timed window (the sizing call is timed on its own:
legs_size_ms, count + scan).  Checked, for every case and both modes: offsets, voxels, positions (f64 bits), status, moves and cost
of the leg call equal the per-leg route's, bit for bit; the leg costs equal the tour's leg_cost.
One JSON line; with --out DIR it is also written to DIR/leg_paths_partial<grid>.json.  --lib PATH loads another build of the
library (one compiled with -DFIESTA_LEG_PATH_WAVES=4, say) and names it in the JSON.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/leg_paths_bench.py` (a run of its own).
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
MODES = (("raw", False, 4096), ("shortcut", True, 4096))
FILL = -7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--caps", type=int, nargs="+", default=[32, 64], help="site counts")
    ap.add_argument("--split", type=int, default=16, help="grid on which large frontier clusters are cut, voxels")
    ap.add_argument("--restarts", type=int, default=64)
    ap.add_argument("--lib", default=None, help="another build of libfiesta_hip.so to measure")
    ap.add_argument("--out", default=None, help="directory for leg_paths_partial<grid>.json")
    args = ap.parse_args()
    if args.lib:
        import fiesta_amd._lib
        fiesta_amd._lib.LIB_PATH = os.path.abspath(args.lib)
    import torch
    from reach_matrix_bench import scene_and_sites
    dev = torch.device("cuda", 0)
    G = args.grid
    m, robot, lo, hi, fv, unsplit, order_of_clusters, all_sites = scene_and_sites(G, args.obstacles, args.split)

    def timed_in_turn(fns):
        """p50 per function; inside every repetition each function runs once, in order"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        m.synchronize()
        ts = [[] for _ in fns]
        for _ in range(args.steps):
            for k, fn in enumerate(fns):
                m.synchronize()
                t0 = time.perf_counter()
                fn()
                m.synchronize()
                ts[k].append(time.perf_counter() - t0)
        return [statistics.median(t) for t in ts]

    def i32(n, cols=None):
        return torch.full((n,) if cols is None else (n, cols), FILL, dtype=torch.int32, device=dev)

    cases, checks = {}, {}
    for cap in args.caps:
        sites = np.ascontiguousarray(all_sites[:cap])
        n = len(sites)
        sd = torch.tensor(sites, dtype=torch.int32, device=dev)
        mat, order, leg_cost = i32(n * n), i32(n), i32(n)
        torch.cuda.synchronize()
        info, tour = {}, {}

        def matrix():
            info.update(m.ReachMatrixDevice(sd.data_ptr(), n, lo=lo, hi=hi, cost_dev_ptr=mat.data_ptr()))

        def site_tour():
            tour.update(m.SiteTourDevice(mat.data_ptr(), n, n, start=0, restarts=args.restarts, order_dev_ptr=order.data_ptr(),
                                         leg_cost_dev_ptr=leg_cost.data_ptr()))

        matrix()
        site_tour()
        assert info["batches"] == 1, info
        legs = tour["n_visited"] - 1
        assert legs >= 1, tour
        order_h = order.cpu().numpy()
        fr_h, to_h = order_h[:legs], order_h[1:legs + 1]
        # per mode: the buffers of the leg call and of the per-leg route, sized once
        buf = {}
        for name, shortcut, span in MODES:
            off = torch.full((legs + 1,), FILL, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            m.LegPathsDevice(order.data_ptr(), legs, off.data_ptr(), to_dev_ptr=order.data_ptr() + 4, shortcut=shortcut, max_span=span)
            m.synchronize()
            offs = off.cpu().numpy()
            total = int(offs[-1])
            buf[name] = {"off": off, "offs": offs, "total": total,
                         "new": {"vox": i32(total + 1, 3), "pos": torch.full((total + 1, 3), float(FILL), dtype=torch.float64, device=dev),
                                 "status": i32(legs), "n_moves": i32(legs), "cost": i32(legs)},
                         "old": {"vox": i32(total + 1, 3), "pos": torch.full((total + 1, 3), float(FILL), dtype=torch.float64, device=dev),
                                 "status": i32(legs), "n_moves": i32(legs), "cost": i32(legs),
                                 "off": torch.full((legs, 2), FILL, dtype=torch.int64, device=dev)}}
        torch.cuda.synchronize()

        def leg_call(name, shortcut, span, size_only=False):
            b = buf[name]
            if size_only:
                return lambda: m.LegPathsDevice(order.data_ptr(), legs, b["off"].data_ptr(), to_dev_ptr=order.data_ptr() + 4, shortcut=shortcut,
                                                max_span=span)
            o = b["new"]
            return lambda: m.LegPathsDevice(order.data_ptr(), legs, b["off"].data_ptr(), to_dev_ptr=order.data_ptr() + 4, shortcut=shortcut, max_span=span,
                                            capacity=b["total"], waypoints_vox_dev_ptr=o["vox"].data_ptr(), waypoints_pos_dev_ptr=o["pos"].data_ptr(),
                                            status_dev_ptr=o["status"].data_ptr(), n_moves_dev_ptr=o["n_moves"].data_ptr(),
                                            cost_dev_ptr=o["cost"].data_ptr())

        def old_route(name, shortcut, span):
            b = buf[name]
            o = b["old"]

            def run():
                for k in range(legs):
                    s, t = int(fr_h[k]), int(to_h[k])
                    at, cnt = int(b["offs"][k]), int(b["offs"][k + 1] - b["offs"][k])
                    m.ReachFieldDevice(sd.data_ptr() + 12 * s, 1, lo, hi, sd.data_ptr() + 12 * t, 1, target_cost_dev_ptr=o["cost"].data_ptr() + 4 * k)
                    m.ReachPathsDevice(sd.data_ptr() + 12 * t, 1, o["off"].data_ptr() + 16 * k, shortcut=shortcut, max_span=span, capacity=cnt,
                                       waypoints_vox_dev_ptr=o["vox"].data_ptr() + 12 * at, waypoints_pos_dev_ptr=o["pos"].data_ptr() + 24 * at,
                                       status_dev_ptr=o["status"].data_ptr() + 4 * k, n_moves_dev_ptr=o["n_moves"].data_ptr() + 4 * k)
            return run

        fns = [matrix, site_tour] + [leg_call(*mode) for mode in MODES] + [leg_call(*mode, size_only=True) for mode in MODES] + \
              [old_route(*mode) for mode in MODES]
        t = timed_in_turn(fns)
        t_matrix, t_tour, t_new, t_size, t_old = t[0], t[1], t[2:4], t[4:6], t[6:8]
        # (the repetitions' last matrix and tour calls have rewritten `order`: the same, the calls are deterministic)
        assert np.array_equal(order.cpu().numpy(), order_h)
        name_c = f"sites{n}"
        case = {"sites": n, "legs": legs, "n_visited": tour["n_visited"], "tour_length": tour["length"], "matrix_ms": t_matrix * 1e3,
                "tour_ms": t_tour * 1e3, "fields": info["fields"], "batches": info["batches"], "box": [info["box_lo"], info["box_hi"]]}
        lc = leg_cost.cpu().numpy()
        for j, (name, shortcut, span) in enumerate(MODES):
            b = buf[name]
            new, old = b["new"], b["old"]
            total = b["total"]
            same = {k: bool(np.array_equal(new[k].cpu().numpy(), old[k].cpu().numpy())) for k in ("vox", "pos", "status", "n_moves", "cost")}
            counts = old["off"].cpu().numpy()
            same["offsets"] = bool((counts[:, 0] == 0).all() and np.array_equal(counts[:, 1], np.diff(b["offs"])) and
                                   np.array_equal(b["off"].cpu().numpy(), b["offs"]))
            same["written"] = bool((new["vox"].cpu().numpy()[:total] != FILL).all() and (new["vox"].cpu().numpy()[total:] == FILL).all())
            for k, v in same.items():
                checks[f"{name_c}_{name}_{k}_equal_per_leg_route"] = v
            checks[f"{name_c}_{name}_cost_is_the_tours_leg_cost"] = bool(np.array_equal(new["cost"].cpu().numpy(), lc[1:legs + 1]))
            checks[f"{name_c}_{name}_all_legs_ok"] = bool((new["status"].cpu().numpy() == 0).all())
            moves = new["n_moves"].cpu().numpy()
            case.update({f"legs_{name}_ms": t_new[j] * 1e3, f"legs_{name}_size_ms": t_size[j] * 1e3, f"old_{name}_ms": t_old[j] * 1e3,
                         f"legs_{name}_over_matrix": t_new[j] / t_matrix, f"legs_{name}_over_old": t_new[j] / t_old[j],
                         f"waypoints_{name}": total})
        case.update({"moves_total": int(moves.sum()), "moves_longest": int(moves.max())})
        cases[name_c] = case
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    head = cases[f"sites{min(args.caps[0], len(all_sites))}"]
    out = {"metric": "leg_paths_shortcut_over_matrix_call", "value": head["legs_shortcut_over_matrix"], "unit": "x", "scene": f"partial{G}", "grid": G,
           "revision": rev, "source_sha256": source_digest(), "lib": args.lib, "robot": robot[0].tolist(), "frontier_voxels": int(len(fv)),
           "split": args.split, "frontier_clusters": int(len(order_of_clusters)), "restarts": args.restarts, "cases": cases, "steps": args.steps,
           "warmup": args.warmup, "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"leg_paths_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if out["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
