#!/usr/bin/env python3
"""Free-space corridors (fiesta_hip_path_corridor[_dev], fiesta_hip_free_boxes[_dev]) on reach_paths_bench's workload, against the
route a user had before the calls existed.

Scene (built here, nothing is read from disk): tools/reach_bench.py's partially observed 512^3 @ 0.1 m map with 50 000 scattered
obstacles; the flood runs in the box of 128^3 voxels around the seed, connectivity 26, clearance 0; the targets are the frontier
voxels of that box and the paths are fiesta_hip_reach_paths' to them, resident on the device: raw, and shortcut with max_span 4096.
The corridors are built in that box as the window, with max_grow 16 and 64.
Measured per (path mode, max_grow), p50 over --steps rounds after --warmup; within a round the calls ALTERNATE, each timed from a
synchronised stream to the next synchronisation:
  dev_ms        fiesta_hip_path_corridor_dev with every output resident on the device (count + scan + write; a sizing call has
                fixed the capacity before)
  host_ms       fiesta_hip_path_corridor with host arrays (the class method: a sizing call and a writing call, staging included)
  paths_ms      the fiesta_hip_reach_paths_dev call that feeds it
  free_boxes_ms fiesta_hip_free_boxes_dev alone, the frontier voxels as seeds
Once, for scale: the route of today -- download_field of the map (download_ms; the call has no box) and the same rule in vectorised
numpy, one array-slice test per slab (fiesta_amd.corridor_model), run on --sample paths and scaled to the batch (model_ms_est).
Checked: on the sample every output of the host variant and of the device batch equals the model, and so does free_boxes.
One JSON line; with --out DIR it is also written to DIR/corridor_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/corridor_bench.py` (a run of its own).
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

PATH_MODES = (("raw", False, 1), ("span4096", True, 4096))
GROWS = (16, 64)
KEYS = ("offsets", "boxes", "boxes_pos", "stop", "entry", "status", "n_chain", "blocked_segment", "blocked_vox")
BOX_KEYS = ("box", "box_pos", "stop", "volume", "status")


def same(a, b):
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b))


def sub_csr(off, pick):
    """rows and offsets of the paths `pick` of a CSR"""
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in pick] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rows, np.concatenate([[0], np.cumsum(off[pick + 1] - off[pick])]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=200, help="paths compared with the model (0: all)")
    ap.add_argument("--out", default=None, help="directory for corridor_partial<grid>.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from reach_bench import build_partial
    dev = torch.device("cuda", 0)
    G = args.grid
    m, _ = build_partial(G, int(round(args.obstacles * (G / 512.0) ** 3)))

    def clock(fn):
        m.synchronize()
        t0 = time.perf_counter()
        r = fn()
        m.synchronize()
        return time.perf_counter() - t0, r

    t_down, f = clock(lambda: m.download_field(("d2", "occ")))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    c0 = max(G // 2 - 32, 0)
    free = np.argwhere((obs & ~occ)[c0:c0 + 64, c0:c0 + 64, c0:c0 + 64]) + c0
    seed = free[np.argmin(((free - G // 2) ** 2).sum(1))].astype(np.int32).reshape(1, 3)
    half = min(64, G // 2)
    lo = np.clip(seed[0] - half, 0, G - 1)
    hi = np.clip(lo + 2 * half - 1, 0, G - 1)
    targets, _ = m.GetFrontierVoxels(lo, hi, want_mask=False)
    n = len(targets)
    m.ReachField(seed, lo, hi, want_cost=False)                                  # (leaves the field retained)
    td = torch.tensor(targets, dtype=torch.int32, device=dev)
    pick = np.arange(n) if args.sample <= 0 or args.sample >= n else np.sort(np.random.RandomState(1).choice(n, args.sample, replace=False))
    sl = tuple(slice(int(a), int(b) + 1) for a, b in zip(lo, hi))
    mkw = dict(lo=lo, hi=hi, origin_vox=tuple(int(v) for v in lo), resolution=0.1)   # the model on the box's part of the dump
    results, checks = {}, {}
    for name, shortcut, span in PATH_MODES:
        pkw = dict(connectivity=26, shortcut=shortcut, max_span=span)
        poff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=0, **pkw)
        m.synchronize()
        n_wp = int(poff[n].item())
        wp = torch.zeros((max(n_wp, 1), 3), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def paths_call():
            m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=n_wp, waypoints_vox_dev_ptr=wp.data_ptr(), **pkw)

        paths_call()
        m.synchronize()
        wp_h, poff_h = wp.cpu().numpy()[:n_wp], poff.cpu().numpy()
        rows, soff = sub_csr(poff_h, pick)
        for grow in GROWS:
            ckw = dict(lo=lo, hi=hi, max_grow=grow)
            off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            per = {k: torch.zeros((n, 3) if k == "blocked_vox" else (n,), dtype=torch.int32, device=dev) for k in KEYS[5:]}
            m.PathCorridorDevice(wp.data_ptr(), n_wp, poff.data_ptr(), n, off.data_ptr(), capacity=0, **ckw)
            m.synchronize()
            total = int(off[n].item())
            box = {"boxes": torch.zeros((max(total, 1), 6), dtype=torch.int32, device=dev), "boxes_pos": torch.zeros((max(total, 1), 6), dtype=torch.float64, device=dev),
                   "stop": torch.zeros((max(total, 1), 6), dtype=torch.uint8, device=dev), "entry": torch.zeros(max(total, 1), dtype=torch.int32, device=dev)}
            torch.cuda.synchronize()

            def dev_call():
                m.PathCorridorDevice(wp.data_ptr(), n_wp, poff.data_ptr(), n, off.data_ptr(), capacity=total, boxes_dev_ptr=box["boxes"].data_ptr(),
                                     boxes_pos_dev_ptr=box["boxes_pos"].data_ptr(), stop_dev_ptr=box["stop"].data_ptr(), entry_dev_ptr=box["entry"].data_ptr(),
                                     status_dev_ptr=per["status"].data_ptr(), n_chain_dev_ptr=per["n_chain"].data_ptr(),
                                     blocked_segment_dev_ptr=per["blocked_segment"].data_ptr(), blocked_vox_dev_ptr=per["blocked_vox"].data_ptr(), **ckw)

            def host_call():
                return m.PathCorridor(wp_h, poff_h, **ckw)

            ts = {"dev_ms": [], "host_ms": [], "paths_ms": []}
            for it in range(args.warmup + args.steps):
                for key, fn in (("dev_ms", dev_call), ("host_ms", host_call), ("paths_ms", paths_call)):
                    t, _ = clock(fn)
                    if it >= args.warmup:
                        ts[key].append(t * 1e3)
            r = {k: statistics.median(v) for k, v in ts.items()}
            # the route of today on the sample, scaled to the batch
            t0 = time.perf_counter()
            want = fiesta_amd.corridor_model(obs[sl], occ[sl], wp_h[rows], soff, **ckw, **{k: v for k, v in mkw.items() if k not in ("lo", "hi")})
            r["model_ms_est"] = (time.perf_counter() - t0) * 1e3 * n / len(pick)
            r["today_route_ms_est"] = t_down * 1e3 + r["model_ms_est"]
            status = per["status"].cpu().numpy()
            boxes_h = box["boxes"].cpu().numpy()[:total].astype(np.int64)
            r.update(paths=n, waypoints=n_wp, boxes=total, corridors_ok=int((status == 0).sum()), corridors_blocked=int((status == 2).sum()),
                     volume=int(np.prod(boxes_h[:, 3:] - boxes_h[:, :3] + 1, axis=1).sum()) if total else 0, boxes_per_s=total / (r["dev_ms"] * 1e-3))
            results[f"{name}_grow{grow}"] = r
            got = m.PathCorridor(wp_h[rows], soff, **ckw)
            checks[f"{name}_grow{grow}_host_sample_equals_model"] = all(same(got[k], want[k]) for k in KEYS)
            doff = off.cpu().numpy()
            drows, _ = sub_csr(doff, pick)
            dev_out = {k: v.cpu().numpy()[:total][drows] for k, v in box.items()}
            checks[f"{name}_grow{grow}_device_batch_equals_model"] = bool(
                np.array_equal(np.diff(doff)[pick], np.diff(want["offsets"])) and all(same(dev_out[k], want[k]) for k in dev_out) and
                all(same(per[k].cpu().numpy()[pick], want[k]) for k in per))
    # free boxes alone, the frontier voxels as seeds
    fb = {}
    for grow in GROWS:
        out = {"box": torch.zeros((n, 6), dtype=torch.int32, device=dev), "box_pos": torch.zeros((n, 6), dtype=torch.float64, device=dev),
               "stop": torch.zeros((n, 6), dtype=torch.uint8, device=dev), "volume": torch.zeros(n, dtype=torch.int64, device=dev),
               "status": torch.zeros(n, dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()

        def fb_call():
            m.FreeBoxesDevice(td.data_ptr(), n, lo, hi, grow, box_dev_ptr=out["box"].data_ptr(), box_pos_dev_ptr=out["box_pos"].data_ptr(),
                              stop_dev_ptr=out["stop"].data_ptr(), volume_dev_ptr=out["volume"].data_ptr(), status_dev_ptr=out["status"].data_ptr())

        ts = [clock(fb_call)[0] * 1e3 for _ in range(args.warmup + args.steps)][args.warmup:]
        t0 = time.perf_counter()
        want = fiesta_amd.free_box_model(obs[sl], occ[sl], targets[pick], max_grow=grow, **mkw)
        t_model = (time.perf_counter() - t0) * 1e3 * n / len(pick)
        fb[f"grow{grow}"] = {"free_boxes_ms": statistics.median(ts), "seeds": n, "model_ms_est": t_model,
                             "mean_volume": float(out["volume"].cpu().numpy().mean()) if n else 0.0}
        checks[f"free_boxes_grow{grow}_sample_equals_model"] = all(same(out[k].cpu().numpy()[pick], want[k]) for k in BOX_KEYS)
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    head = results["span4096_grow16"]
    res = {"metric": "corridor_today_route_over_device_call_span4096_grow16", "value": head["today_route_ms_est"] / head["dev_ms"], "unit": "x",
           "scene": f"partial{G}", "grid": G, "revision": rev, "source_sha256": source_digest(), "seed": seed[0].tolist(),
           "box": [lo.tolist(), hi.tolist()], "download_ms": t_down * 1e3, "corridors": results, "free_boxes": fb, "sample": int(len(pick)),
           "steps": args.steps, "warmup": args.warmup, "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"corridor_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if res["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
