#!/usr/bin/env python3
"""Frontier extraction (fiesta_hip_get_frontier_voxels[_dev]) on two maps an exploring robot produces, against the one sweep of a
bitmap the library already had and against the route a user had before.

Scenes (built here, nothing is read from disk):
  partial512  bench.py's C2-partial map: 512^3 @ 0.1 m, 27 % of its 32^3-voxel blocks never observed, 50 000 scattered obstacles
  cones256    256^3 @ 0.1 m observed through four view cones (60 degrees half angle, 12 m range) whose last voxel of range is a hit
Measured per scene in one run, p50 over --steps calls after --warmup, a device synchronise around every call:
  frontier_dev_ms          the device variant into buffers that hold every entry, whole map, min_clearance 0 (what a planner runs per frame)
  frontier_dev_clear_ms    ... with min_clearance 0.3 m (the field is decoded for every candidate)
  frontier_dev_box_ms      ... min_clearance 0, restricted to the central box of a quarter of the extent per axis (128^3 of 512^3)
  frontier_count_ms        the host variant with capacity 0 (zero the counter, sweep, read the counter back)
  occupied_count_ms        fiesta_hip_get_occupied_voxels with capacity 0: the same shape of call over ONE bitmap -- the floor for "a
                           sweep of a bitmap plus compaction"; frontier_over_occupied = frontier_count_ms / occupied_count_ms
  download_route_ms        once, for scale, the route a user had before: download_field (d2, occ) + fiesta_amd.frontier_model in numpy
                           (no filter, so no distances are needed)
  hbm_frac*                the bytes the call must read -- two bitmaps over the swept words, plus 4 B per candidate when the filter is
                           on -- over the call time, as a fraction of the 8.0 TB/s HBM peak (a whole-call figure, launch included)
Checked: the device variant's set of (voxel, mask) rows equals frontier_model's on both scenes (filter off; the boxed call too).
One JSON line; with --out DIR it is also written to DIR/frontiers_<scene>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/frontier_bench.py` (a run of its own).
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
HBM_PEAK = 8.0e12


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
    return m


def build_cones(G):
    """four sensors looking along +x, -x, +y, -y from a quarter of the way in; inside a cone everything up to the range is free, the
    last voxel of the range is a hit"""
    import torch
    import fiesta_amd
    from bench import P_DEFAULT
    dev = torch.device("cuda", 0)
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, (G * 0.1,) * 3)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    ax = torch.arange(G, device=dev, dtype=torch.float32)
    X, Y, Z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    R = float(int(0.47 * G))   # 120 voxels at 256^3
    free = torch.zeros((G, G, G), dtype=torch.bool, device=dev)
    hit = torch.zeros_like(free)
    q, h = G // 4, G // 2
    for pos, axis, sign in (((q, h, h), 0, 1.0), ((G - q, h + 9, h - 7), 0, -1.0), ((h - 11, q, h + 5), 1, 1.0), ((h + 3, G - q, h), 1, -1.0)):
        d = (X - pos[0], Y - pos[1], Z - pos[2])
        r = torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        inside = (sign * d[axis] >= 0.5 * r) & (r <= R) & (r > 0)
        free |= inside & (r <= R - 1)
        hit |= inside & (r > R - 1)
    free &= ~hit
    for cycle in range(3):
        for mask, occ in ((free, 0), (hit, 1)):
            if cycle and not occ:
                continue
            v = torch.nonzero(mask).to(torch.int32).contiguous()
            o = torch.full((len(v),), occ, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            m.SetOccupancyDevice(v.data_ptr(), o.data_ptr(), len(v))
            m.synchronize()
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


def sorted_rows(vox, mask):
    a = np.concatenate([np.asarray(vox, np.int64).reshape(-1, 3), np.asarray(mask, np.int64).reshape(-1, 1)], 1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def measure(name, m, args):
    import torch
    import fiesta_amd
    dev = torch.device("cuda", 0)
    G = m.grid_size[0]
    lib, h = m._lib, m._h
    n64 = C.c_int64(0)

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

    c0 = G // 2 - G // 8
    box = ((c0,) * 3, (c0 + G // 4 - 1,) * 3)
    total = len(m.GetFrontierVoxels(want_mask=False)[0])
    total_clear = len(m.GetFrontierVoxels(min_clearance=0.3, want_mask=False)[0])
    total_box = len(m.GetFrontierVoxels(*box, want_mask=False)[0])
    vox = torch.empty((max(total, 1), 3), dtype=torch.int32, device=dev)
    mask = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
    count = torch.zeros((1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def dev_call(lo=None, hi=None, clearance=0.0):
        m.GetFrontierVoxelsDevice(lo, hi, clearance, vox.data_ptr(), mask.data_ptr(), total, count.data_ptr())

    t_dev = timed(dev_call)
    whole = sorted_rows(vox[:total].cpu().numpy(), mask[:total].cpu().numpy())
    t_clear = timed(lambda: dev_call(clearance=0.3))
    t_box = timed(lambda: dev_call(*box))
    boxed = sorted_rows(vox[:total_box].cpu().numpy(), mask[:total_box].cpu().numpy())
    t_count = timed(lambda: lib.fiesta_hip_get_frontier_voxels(h, None, None, 0.0, None, None, 0, C.byref(n64)))
    t_occ = timed(lambda: lib.fiesta_hip_get_occupied_voxels(h, None, 0, C.byref(n64)))
    n_occ = n64.value
    state = {}

    def download_route():
        f = m.download_field(("d2", "occ"))
        state["obs"], state["occ"] = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
        state["model"] = fiesta_amd.frontier_model(state["obs"], state["occ"])

    t_route = timed(download_route, steps=1, warmup=0)
    checks = {"whole_map_equals_model": bool(np.array_equal(whole, sorted_rows(*state["model"]))),
              "boxed_equals_model": bool(np.array_equal(boxed, sorted_rows(*fiesta_amd.frontier_model(state["obs"], state["occ"], lo=box[0], hi=box[1]))))}
    nzw = (G + 31) // 32
    words, words_box = G * G * nzw, (G // 4) * (G // 4) * ((box[1][2] >> 5) - (box[0][2] >> 5) + 1)
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    out = {"metric": "frontier_over_occupied_sweep", "value": t_count / t_occ, "unit": "x", "scene": name, "grid": G, "revision": rev,
           "source_sha256": source_digest(), "observed_fraction": float(state["obs"].mean()), "occupied_voxels": int(n_occ),
           "frontier_voxels": total, "frontier_voxels_clear_0.3": total_clear, "frontier_voxels_box": total_box, "box": [list(box[0]), list(box[1])],
           "frontier_dev_ms": t_dev * 1e3, "frontier_dev_clear_ms": t_clear * 1e3, "frontier_dev_box_ms": t_box * 1e3,
           "frontier_count_ms": t_count * 1e3, "occupied_count_ms": t_occ * 1e3, "download_route_ms": t_route * 1e3,
           "box_over_whole": t_box / t_dev, "download_route_over_frontier_dev": t_route / t_dev,
           "hbm_frac": words * 8 / t_dev / HBM_PEAK, "hbm_frac_clear": (words * 8 + total * 4) / t_clear / HBM_PEAK,
           "hbm_frac_box": words_box * 8 / t_box / HBM_PEAK, "bytes_must_read": words * 8, "steps": args.steps, "warmup": args.warmup,
           "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"frontiers_{name}.json"), "w").write(line + "\n")
    return out["all_checks"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="partial512,cones256")
    ap.add_argument("--grid", type=int, default=0, help="override both scenes' grid (a multiple of 32; a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for frontiers_<scene>.json")
    args = ap.parse_args()
    ok = True
    for name in args.scenes.split(","):
        if name == "partial512":
            G = args.grid or 512
            m = build_partial(G, int(round(args.obstacles * (G / 512.0) ** 3)))
        elif name == "cones256":
            m = build_cones(args.grid or 256)
        else:
            raise SystemExit(f"unknown scene {name}")
        ok &= measure(name, m, args)
        m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
