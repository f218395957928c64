#!/usr/bin/env python3
"""Reachability (fiesta_hip_reach_field[_dev]) on bench.py's C2-partial map, against the route a user had before and against the
calls a planner runs next to it.

Scene (built here, nothing is read from disk): 512^3 @ 0.1 m, 27 % of its 32^3-voxel blocks never observed, 50 000 scattered
obstacles.  The seed is the free voxel nearest to the centre of the map.  Two cases, each with min_clearance 0 and 0.3 m, connectivity
26, the device variant into a cost field resident on the device:
  whole   the whole array
  box128  the box of 128^3 voxels around the seed
Measured per case, p50 over --steps calls after --warmup (the call synchronises by itself):
  call_ms              the call; rounds, tile_visits, n_reached, reached_per_s = n_reached / call time
  mask_ms              the same call without seeds and without info: k_reach_mask alone (plus the call's fixed cost: two memsets, one
                       read of the counters) -- the traversability bitmap, the cost field's initialisation
Once, for scale:
  download_route_ms    the route available before: download_field (d2, occ), GetDistance of the box's voxels and
                       fiesta_amd.reach_model (numpy + a heap Dijkstra) on the 128^3 box
  frontier_count_ms    the whole-map frontier call (capacity 0): the price of one sweep of the bitmaps
  update_esdf_ms       one UpdateESDF of this map after 25 000 new obstacle voxels (half of bench.py's step), host time
Checked: on the 128^3 box the call's whole cost field and its info equal the model's, for both clearances.
One JSON line; with --out DIR it is also written to DIR/reach_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/reach_bench.py` (a run of its own).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def build_partial(G, obstacles):
    import fiesta_amd
    from bench import P_DEFAULT, Workload
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, (G * 0.1,) * 3)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    keep = np.random.RandomState(2718).rand(G // 32, G // 32, G // 32) >= 0.27
    for bx, by, bz in np.argwhere(keep):
        m.SetOccupancyBox((int(bx) * 32, int(by) * 32, int(bz) * 32), (int(bx) * 32 + 31, int(by) * 32 + 31, int(bz) * 32 + 31), 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    wl = Workload(G, obstacles, seed=12345)
    for _ in range(3):
        m.SetOccupancy(wl.initial(), 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m, wl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="directory for reach_partial<grid>.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from fiesta_amd._lib import ReachResult
    from fiesta_amd.esdf_map import _p
    dev = torch.device("cuda", 0)
    G = args.grid
    m, wl = build_partial(G, int(round(args.obstacles * (G / 512.0) ** 3)))
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    c0 = max(G // 2 - 32, 0)                       # (the nearest free voxel lies well inside the central 64^3)
    free = np.argwhere((obs & ~occ)[c0:c0 + 64, c0:c0 + 64, c0:c0 + 64]) + c0
    seed = free[np.argmin(((free - G // 2) ** 2).sum(1))].astype(np.int32).reshape(1, 3)
    half = min(64, G // 2)
    lo = np.clip(seed[0] - half, 0, G - 1)
    hi = np.clip(lo + 2 * half - 1, 0, G - 1)
    cost = torch.empty(G ** 3, dtype=torch.int32, device=dev)
    sd = torch.tensor(seed, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

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

    res = ReachResult(cost.data_ptr(), None)

    def mask_only(blo, bhi, clearance):
        st = m._lib.fiesta_hip_reach_field_dev(m._h, _p(blo), _p(bhi), None, 0, None, 0, float(clearance), 26, 0, C.byref(res), None)
        assert st == 0

    cases = {}
    for name, (blo, bhi) in (("whole", (None, None)), ("box128", (lo, hi))):
        b32 = (None, None) if blo is None else (np.ascontiguousarray(blo, np.int32), np.ascontiguousarray(bhi, np.int32))
        for clearance in (0.0, 0.3):
            info = {}

            def call():
                info.update(m.ReachFieldDevice(sd.data_ptr(), 1, blo, bhi, min_clearance=clearance, cost_dev_ptr=cost.data_ptr()))

            t = timed(call)
            t_mask = timed(lambda: mask_only(b32[0], b32[1], clearance))
            cases[f"{name}_clear{clearance}"] = {
                "call_ms": t * 1e3, "mask_ms": t_mask * 1e3, "rounds": info["rounds"], "tile_visits": info["tile_visits"],
                "n_traversable": info["n_traversable"], "n_reached": info["n_reached"], "max_cost": info["max_cost"],
                "reached_per_s": info["n_reached"] / t, "box": [info["box_lo"], info["box_hi"]]}

    # the 128^3 box against the model, and the route a user had before
    state = {}

    def download_route():
        g = m.download_field(("d2", "occ"))
        o, c = (g["d2"] >= 0).reshape(m.grid_size), g["occ"].reshape(m.grid_size) != 0
        box = tuple(slice(int(a), int(b) + 1) for a, b in zip(lo, hi))
        ext = tuple(int(b - a + 1) for a, b in zip(lo, hi))
        V = np.stack(np.meshgrid(*[np.arange(int(a), int(b) + 1) for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
        state["args"] = (o[box], c[box], m.GetDistance(V).reshape(ext))
        state["model0"] = fiesta_amd.reach_model(state["args"][0], state["args"][1], seed, origin_vox=lo)

    t_route = timed(download_route, steps=1, warmup=0)
    checks = {}
    for clearance in (0.0, 0.3):
        want = state["model0"] if clearance == 0.0 else \
            fiesta_amd.reach_model(state["args"][0], state["args"][1], seed, state["args"][2], min_clearance=clearance, origin_vox=lo)
        got = m.ReachField(seed, lo, hi, min_clearance=clearance)
        checks[f"box128_clear{clearance}_equals_model"] = bool(
            np.array_equal(got["cost"], want["cost"]) and all(got[k] == want[k] for k in ("n_traversable", "n_reached", "max_cost", "n_seeds_used")))
    n64 = C.c_int64(0)
    t_frontier = timed(lambda: m._lib.fiesta_hip_get_frontier_voxels(m._h, None, None, 0.0, None, None, 0, C.byref(n64)))
    new, _ = wl.next_step()
    for _ in range(3):
        m.SetOccupancy(new, 1, want_ret=False)
        m.UpdateOccupancy(True)
    t0 = time.perf_counter()
    st = m.UpdateESDF()
    t_esdf = time.perf_counter() - t0
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    box_ms = cases["box128_clear0.0"]["call_ms"]
    out = {"metric": "reach_box128_over_update_esdf", "value": box_ms / (t_esdf * 1e3), "unit": "x", "scene": f"partial{G}", "grid": G,
           "revision": rev, "source_sha256": source_digest(), "seed": seed[0].tolist(), "observed_fraction": float(obs.mean()),
           "cases": cases, "download_route_ms": t_route * 1e3, "download_route_over_box128_call": t_route * 1e3 / box_ms,
           "frontier_count_ms": t_frontier * 1e3, "frontier_voxels": int(n64.value), "update_esdf_ms": t_esdf * 1e3,
           "update_esdf_device_ms": st["device_ms"], "update_esdf_inserted": st["inserted"], "steps": args.steps, "warmup": args.warmup,
           "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"reach_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if out["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
