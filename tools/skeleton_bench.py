#!/usr/bin/env python3
"""Skeleton extraction (fiesta_hip_get_skeleton_voxels[_dev]) on the maps bench.py measures, against the sweeps the library already
had and against the route a user had before.

Scenes (built here, nothing is read from disk):
  c2          bench.py's C2 map: 512^3 @ 0.1 m, fully observed, 50 000 scattered obstacles
  c2_partial  bench.py's C2-partial map: the same with 27 % of its 32^3-voxel blocks never observed
  hash        the hash workload's map (bench.py --workload c4): the first --frames frames of the moving 6 x 6 x 3 m window @ 0.05 m
Measured per scene in one run, p50 over --steps calls after --warmup, a device synchronise around every call:
  skeleton_dev_ms          the device variant into buffers that hold every entry, whole map, min_sep2 9, min_clearance 0
  skeleton_dev_clear_ms    ... with min_clearance 0.3 m
  skeleton_dev_box_ms      ... min_clearance 0, restricted to a central box of 128^3 voxels
  frontier_count_ms        fiesta_hip_get_frontier_voxels with capacity 0: the sweep that reads the bitmaps only (dense) / the pages' words
  no_obstacle_count_ms     dense maps: fiesta_hip_count_no_obstacle, ONE pass over the field that reads every word and writes nothing --
                           the floor for "read the field once"; skeleton_over_field_read = skeleton_dev_ms / no_obstacle_count_ms
  download_ms, model_ms    once, for scale, the route a user had before: download_field (d2, coc, occ; 16 B per voxel) or
                           download_hash, and fiesta_amd.skeleton_model in numpy -- the model runs on --samples seeded boxes of 48^3
                           voxels and model_ms_extrapolated scales its time to the swept volume
  hbm_frac*                4 B per swept voxel over the call time, as a fraction of the 8.0 TB/s HBM peak (a whole-call figure, launch
                           included; dense: the voxels of the box, hash: the voxels of the pages that meet the box)
Checked: on every sampled box the device variant's set of (voxel, mask, d2, sep2) rows, restricted to the box, equals skeleton_model's
on the map's own dump (with a one-voxel halo around the box, so the neighbour test sees what the kernel sees).
One JSON line per scene; with --out DIR it is also written to DIR/skeleton_<scene>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/skeleton_bench.py` (a run of its own).
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
MIN_SEP2 = 9
NAMES = ("vox", "mask", "d2", "sep2")


def build_dense(G, obstacles, unobserved):
    import fiesta_amd
    from bench import P_DEFAULT, Workload
    m = fiesta_amd.ESDFMap((0, 0, 0), 0.1, (G * 0.1,) * 3)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    if unobserved > 0:
        keep = np.random.RandomState(2718).rand(G // 32, G // 32, G // 32) >= unobserved
        for bx, by, bz in np.argwhere(keep):
            m.SetOccupancyBox((int(bx) * 32, int(by) * 32, int(bz) * 32), (int(bx) * 32 + 31, int(by) * 32 + 31, int(bz) * 32 + 31), 0)
    else:
        m.SetOccupancyBox((0, 0, 0), (G - 1,) * 3, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    wl = Workload(G, obstacles, seed=12345)
    for _ in range(3):
        m.SetOccupancy(wl.initial(), 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    return m


def build_hash(frames):
    import fiesta_amd
    from bench import P_DEFAULT
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scenarios import c4_frame
    m = fiesta_amd.ESDFMap((0.0, 0.0, 0.0), 0.05, reserve_size=1000000, mode="hash")
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    for k in range(frames):
        lo, hi, occ = c4_frame(k)
        m.SetOccupancyBox(lo, hi, 0)
        m.SetOccupancy(np.ascontiguousarray(occ, np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)
        m.UpdateESDF()
    return m


def sorted_rows(r):
    a = np.concatenate([np.asarray(r["vox"], np.int64).reshape(-1, 3)] + [np.asarray(r[k], np.int64).reshape(-1, 1) for k in NAMES[1:]], 1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


class Dump:
    """what the map reports of itself, and the sub-arrays the model runs on"""

    def __init__(self, m, hashed):
        self.hashed = hashed
        t0 = time.perf_counter()
        if hashed:
            h = m.download_hash()
            self.vox, self.d2, self.coc, self.occ = h["vox"].astype(np.int64), h["d2"], h["coc"], h["occ"]
            self.lo, self.hi = self.vox.min(0), self.vox.max(0)
        else:
            f = m.download_field(("d2", "coc", "occ"))
            s = tuple(m.grid_size)
            self.d2, self.coc, self.occ = f["d2"].reshape(s), f["coc"].reshape(s + (3,)), f["occ"].reshape(s)
            self.lo, self.hi = np.zeros(3, np.int64), np.array(s, np.int64) - 1
        self.download_s = time.perf_counter() - t0

    def sub(self, lo, hi):
        """(d2, coc, occ) over the box [lo - 1, hi + 1]; what the map does not hold is never observed"""
        lo, hi = np.asarray(lo, np.int64) - 1, np.asarray(hi, np.int64) + 1
        shape = tuple(int(v) for v in hi - lo + 1)
        d2, coc, occ = np.full(shape, -1, np.int64), np.zeros(shape + (3,), np.int64), np.zeros(shape, bool)
        if self.hashed:
            inside = ((self.vox >= lo) & (self.vox <= hi)).all(1)
            i = tuple((self.vox[inside] - lo).T)
            d2[i], coc[i], occ[i] = self.d2[inside], self.coc[inside], self.occ[inside] != 0
        else:
            a, b = np.maximum(lo, 0), np.minimum(hi, self.hi)
            src = tuple(slice(int(p), int(q) + 1) for p, q in zip(a, b))
            dst = tuple(slice(int(p - o), int(q - o) + 1) for p, q, o in zip(a, b, lo))
            d2[dst], coc[dst], occ[dst] = self.d2[src], self.coc[src], self.occ[src] != 0
        return d2, coc, occ, lo


def measure(name, m, args, hashed):
    import torch
    import fiesta_amd
    dev = torch.device("cuda", 0)
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

    dump = Dump(m, hashed)
    mid = (dump.lo + dump.hi) // 2
    box = (tuple(int(v) for v in mid - 64), tuple(int(v) for v in mid + 63))
    total = m.GetSkeletonVoxels(min_sep2=MIN_SEP2, want=())["n"]
    total_clear = m.GetSkeletonVoxels(min_sep2=MIN_SEP2, min_clearance=0.3, want=())["n"]
    total_box = m.GetSkeletonVoxels(*box, min_sep2=MIN_SEP2, want=())["n"]
    cap = max(total, 1)
    buf = {"vox": torch.empty((cap, 3), dtype=torch.int32, device=dev), "mask": torch.empty((cap,), dtype=torch.uint8, device=dev),
           "d2": torch.empty((cap,), dtype=torch.int32, device=dev), "sep2": torch.empty((cap,), dtype=torch.int32, device=dev)}
    count = torch.zeros((1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def dev_call(lo=None, hi=None, clearance=0.0):
        m.GetSkeletonVoxelsDevice(lo, hi, MIN_SEP2, clearance, cap, count.data_ptr(), *[buf[k].data_ptr() for k in NAMES])

    t_dev = timed(dev_call)
    t_clear = timed(lambda: dev_call(clearance=0.3))
    t_box = timed(lambda: dev_call(*box))
    t_front = timed(lambda: lib.fiesta_hip_get_frontier_voxels(h, None, None, 0.0, None, None, 0, C.byref(n64)))
    t_field = None if hashed else timed(lambda: lib.fiesta_hip_count_no_obstacle(h, C.byref(n64)))
    # the seeded sample against the model, on the map's own dump
    rng = np.random.RandomState(4242)
    checks, model_s, model_vox = {}, 0.0, 0
    for s in range(args.samples):
        lo = np.array([rng.randint(int(a), max(int(b) - 46, int(a) + 1)) for a, b in zip(dump.lo, dump.hi)], np.int64)
        hi = np.minimum(lo + 47, dump.hi)
        d2, coc, occ, org = dump.sub(lo, hi)
        t0 = time.perf_counter()
        want = fiesta_amd.skeleton_model(d2, coc, occ, MIN_SEP2, lo=lo, hi=hi, origin_vox=org)
        model_s += time.perf_counter() - t0
        model_vox += int(np.prod(hi - lo + 1))
        got = m.GetSkeletonVoxels(lo, hi, MIN_SEP2)
        checks[f"sample_{s}_equals_model"] = bool(np.array_equal(sorted_rows(got), sorted_rows(want)))
        checks[f"sample_{s}_rows"] = len(want["mask"])
    if hashed:
        pages = len(dump.d2) // 8192
        swept = pages * 8192
        tiles = np.unique(np.stack([dump.vox[::8192, 0] >> 4, dump.vox[::8192, 1] >> 4, dump.vox[::8192, 2] >> 5], 1), axis=0)
        tlo, thi = tiles * (16, 16, 32), tiles * (16, 16, 32) + (15, 15, 31)
        swept_box = int(((tlo <= box[1]).all(1) & (thi >= box[0]).all(1)).sum()) * 8192
    else:
        swept, swept_box = int(np.prod(dump.hi + 1)), 128 ** 3
    ok = all(v for k, v in checks.items() if k.endswith("equals_model")) and sum(v for k, v in checks.items() if k.endswith("rows")) > 0
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    out = {"metric": "skeleton_over_field_read", "value": None if hashed else t_dev / t_field, "unit": "x", "scene": name,
           "revision": rev, "source_sha256": source_digest(), "min_sep2": MIN_SEP2, "swept_voxels": swept, "swept_voxels_box": swept_box,
           "skeleton_voxels": total, "skeleton_voxels_clear_0.3": total_clear, "skeleton_voxels_box": total_box, "box": [list(box[0]), list(box[1])],
           "skeleton_dev_ms": t_dev * 1e3, "skeleton_dev_clear_ms": t_clear * 1e3, "skeleton_dev_box_ms": t_box * 1e3,
           "frontier_count_ms": t_front * 1e3, "no_obstacle_count_ms": None if hashed else t_field * 1e3,
           "skeleton_over_frontier_sweep": t_dev / t_front, "download_ms": dump.download_s * 1e3, "model_ms_sampled": model_s * 1e3,
           "model_ms_extrapolated": model_s * 1e3 * swept / max(model_vox, 1),
           "download_route_over_skeleton_dev": (dump.download_s + model_s * swept / max(model_vox, 1)) / t_dev,
           "hbm_frac": swept * 4 / t_dev / HBM_PEAK, "hbm_frac_clear": swept * 4 / t_clear / HBM_PEAK, "hbm_frac_box": swept_box * 4 / t_box / HBM_PEAK,
           "hbm_frac_field_read": None if hashed else swept * 4 / t_field / HBM_PEAK, "steps": args.steps, "warmup": args.warmup,
           "checks": checks, "all_checks": bool(ok)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"skeleton_{name}.json"), "w").write(line + "\n")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2,c2_partial,hash")
    ap.add_argument("--grid", type=int, default=512, help="the dense scenes' grid (a multiple of 32; a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--frames", type=int, default=12, help="frames of the hash workload")
    ap.add_argument("--samples", type=int, default=3, help="boxes of 48^3 voxels checked against the model")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for skeleton_<scene>.json")
    args = ap.parse_args()
    ok = True
    for name in args.scenes.split(","):
        if name in ("c2", "c2_partial"):
            m = build_dense(args.grid, int(round(args.obstacles * (args.grid / 512.0) ** 3)), 0.27 if name == "c2_partial" else 0.0)
        elif name == "hash":
            m = build_hash(args.frames)
        else:
            raise SystemExit(f"unknown scene {name}")
        ok &= measure(name, m, args, name == "hash")
        m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
