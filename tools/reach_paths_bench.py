#!/usr/bin/env python3
"""Reach paths (fiesta_hip_reach_paths[_dev]) on reach_bench's map, against the route a user had before the call existed.

Scene (built here, nothing is read from disk): tools/reach_bench.py's partially observed 512^3 @ 0.1 m map with 50 000 scattered
obstacles; the flood runs in the box of 128^3 voxels around the seed (the free voxel nearest to the centre), connectivity 26,
clearance 0.  The targets are the frontier voxels of that box (fiesta_hip_get_frontier_voxels), resident on the device.
Measured, p50 over --steps calls after --warmup, the device variant on the retained field with every output resident on the device
(a sizing call has fixed the capacity before; each timed call is count + scan + write, then one synchronisation):
  raw        every voxel of the descent
  span32     shortcut, max_span 32
  span4096   shortcut, max_span 4096
per mode: call_ms, paths_per_s (targets with status OK per second), waypoints, and voxel_tests_per_s_est -- the voxels the sequential rule
reads for its visibility tests (fiesta_amd.reach_paths_model counts them: every test up to its first failing voxel, nothing shared
between targets; a wave tests 64 candidates at once and so reads more than that) per second of the call.
Once, for scale: the route that existed before -- fiesta_hip_reach_field's host variant with the cost field copied back
(field_copy_ms; field_only_ms is the same flood without the copy) plus fiesta_amd.reach_paths_model on the host, run on a sample of
--sample targets (all with --sample 0) and scaled to the batch (model_ms_est; so are the voxel tests).
Checked: the host variant on the sample equals the model, every array, every mode; the device batch agrees on status and counts.
One JSON line; with --out DIR it is also written to DIR/reach_paths_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/reach_paths_bench.py` (a run of its own).
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

MODES = (("raw", False, 1), ("span32", True, 32), ("span4096", True, 4096))
KEYS = ("offsets", "waypoints_vox", "waypoints_pos", "status", "n_moves")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=2000, help="targets compared with the model (0: all)")
    ap.add_argument("--out", default=None, help="directory for reach_paths_partial<grid>.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from reach_bench import build_partial
    dev = torch.device("cuda", 0)
    G = args.grid
    m, _ = build_partial(G, int(round(args.obstacles * (G / 512.0) ** 3)))
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    c0 = max(G // 2 - 32, 0)
    free = np.argwhere((obs & ~occ)[c0:c0 + 64, c0:c0 + 64, c0:c0 + 64]) + c0
    seed = free[np.argmin(((free - G // 2) ** 2).sum(1))].astype(np.int32).reshape(1, 3)
    half = min(64, G // 2)
    lo = np.clip(seed[0] - half, 0, G - 1)
    hi = np.clip(lo + 2 * half - 1, 0, G - 1)
    targets, _ = m.GetFrontierVoxels(lo, hi, want_mask=False)
    n = len(targets)

    def timed(fn, steps=args.steps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        m.synchronize()
        ts = []
        for _ in range(steps):
            m.synchronize()
            t0 = time.perf_counter()
            fn()
            m.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    # the route that existed before: the flood with its cost field copied to the host, then the descent on the host
    state = {}

    def field_copy():
        state["field"] = m.ReachField(seed, lo, hi)

    t_copy = timed(field_copy, steps=3, warmup=1)
    t_field = timed(lambda: m.ReachField(seed, lo, hi, want_cost=False), steps=3, warmup=1)   # (leaves the field retained)
    field = state["field"]
    box_lo = field["box_lo"]
    td = torch.tensor(targets, dtype=torch.int32, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    mv = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pick = np.arange(n) if args.sample <= 0 or args.sample >= n else np.sort(np.random.RandomState(1).choice(n, args.sample, replace=False))
    modes, checks = {}, {}
    for name, shortcut, span in MODES:
        kw = dict(connectivity=26, shortcut=shortcut, max_span=span)
        m.ReachPathsDevice(td.data_ptr(), n, off.data_ptr(), capacity=0, **kw)
        m.synchronize()
        total = int(off[n].item())
        vox = torch.zeros((max(total, 1), 3), dtype=torch.int32, device=dev)
        pos = torch.zeros((max(total, 1), 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def call():
            m.ReachPathsDevice(td.data_ptr(), n, off.data_ptr(), capacity=total, waypoints_vox_dev_ptr=vox.data_ptr(),
                               waypoints_pos_dev_ptr=pos.data_ptr(), status_dev_ptr=st.data_ptr(), n_moves_dev_ptr=mv.data_ptr(), **kw)

        t = timed(call)
        # the host descent (the model) on the sample; its time and its work are scaled to all targets (an estimate: the model shares
        # work between targets, so the scaled time is a lower bound of the whole batch's)
        stats = {}
        t0 = time.perf_counter()
        want = fiesta_amd.reach_paths_model(field["cost"], box_lo, targets[pick], 26, 1 if shortcut else 0, span, (0.0, 0.0, 0.0), 0.1, stats=stats)
        t_model = (time.perf_counter() - t0) * n / len(pick)
        tests = stats["voxel_tests"] * n / len(pick)
        status = st.cpu().numpy()
        n_ok = int((status == 0).sum())
        modes[name] = {"call_ms": t * 1e3, "paths_per_s": n_ok / t, "paths_ok": n_ok, "waypoints": total, "moves": int(mv.cpu().numpy()[status == 0].sum()),
                       "voxel_tests_est": tests, "voxel_tests_per_s_est": tests / t, "model_ms_est": t_model * 1e3,
                       "copy_route_ms_est": t_copy * 1e3 + t_model * 1e3, "device_route_ms": t_field * 1e3 + t * 1e3}
        # the sample against the model: the host variant on the picked targets (per-target results do not depend on the batch), and
        # the big device batch's status and waypoint counts of those targets
        got = m.ReachPaths(targets[pick], **kw)
        checks[f"{name}_sample_equals_model"] = bool(all(np.array_equal(got[k], want[k]) for k in KEYS))
        checks[f"{name}_device_batch_agrees"] = bool(np.array_equal(status[pick], want["status"]) and
                                                     np.array_equal(np.diff(off.cpu().numpy())[pick], np.diff(want["offsets"])))
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    out = {"metric": "reach_paths_copy_route_over_device_route_span4096",
           "value": modes["span4096"]["copy_route_ms_est"] / modes["span4096"]["device_route_ms"], "unit": "x", "scene": f"partial{G}", "grid": G,
           "revision": rev, "source_sha256": source_digest(), "seed": seed[0].tolist(), "box": [field["box_lo"], field["box_hi"]],
           "targets": n, "n_reached": field["n_reached"], "field_copy_ms": t_copy * 1e3, "field_only_ms": t_field * 1e3,
           "copy_alone_ms": (t_copy - t_field) * 1e3, "modes": modes, "sample": int(len(pick)), "steps": args.steps, "warmup": args.warmup,
           "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"reach_paths_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if out["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
