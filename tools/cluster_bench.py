#!/usr/bin/env python3
"""Voxel clustering (fiesta_hip_cluster_voxels[_dev]) on the whole-map frontier of two maps an exploring robot produces, against the
frontier sweep that feeds it and against the route a user had before.

Scenes (tools/frontier_bench.py's, built here, nothing is read from disk):
  partial512  bench.py's C2-partial map: 512^3 @ 0.1 m, 27 % of its 32^3-voxel blocks never observed, 50 000 scattered obstacles
  cones256    256^3 @ 0.1 m observed through four view cones whose last voxel of range is a hit
Measured per scene in one run, p50 over --steps calls after --warmup, a device synchronise around every call; per setting
(connectivity 6 and 26, min_size 1 and 10):
  cluster_dev_ms     the device variant on the frontier list resident on the device, every output written, capacities = entries
  chain_dev_ms       fiesta_hip_get_frontier_voxels_dev followed by the device variant through n_dev: no host round trip between them
  entries_per_s      frontier voxels / cluster_dev time;  K and largest: what the call found
and once per scene:
  frontier_dev_ms    the frontier sweep alone: the floor (cluster_over_frontier = cluster_dev_ms / frontier_dev_ms)
  frontier_host_ms   the host frontier call, copy-back included: the first half of the route a user had before
  copy_ms            frontier_host_ms - frontier_dev_ms: what the copy alone costs
  model_ms           fiesta_amd.cluster_model (a dict and a BFS in plain Python: the host flood fill) on a SAMPLE -- the frontier
                     voxels of a sub-box, at most --sample entries -- scaled by entries / sample entries (model_scaled_ms); the model
                     is linear in the entries.  host_route_ms = frontier_host_ms + model_scaled_ms
  saved_ms           host_route_ms - chain_dev_ms, to be compared with copy_ms
Checked: on the sample, for every setting, the device call's labels, per-cluster arrays, totals and member sets equal the model's; on
the whole list, that the chain's totals equal those of the call on the resident list.
One JSON line per scene; with --out DIR it is also written to DIR/clusters_<scene>.json.
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
SETTINGS = ((6, 1), (6, 10), (26, 1), (26, 10))
PER_CLUSTER = ("size", "root", "box_lo", "box_hi", "centroid", "mask_or", "key_min", "key_argmin")
TOTALS = ("n_clusters", "n_members", "n_invalid", "n_duplicates", "n_dropped_clusters", "largest")


def same(got, want):
    for k in TOTALS:
        if got[k] != want[k]:
            return False
    for k in ("label", "offsets") + PER_CLUSTER:
        if not np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(want[k]).view(np.uint8)):
            return False
    off = want["offsets"]
    return all(sorted(got["members"][off[k]:off[k + 1]].tolist()) == sorted(want["members"][off[k]:off[k + 1]].tolist()) for k in range(len(off) - 1))


def measure(name, m, args):
    import torch
    import fiesta_amd
    from fiesta_amd.esdf_map import CLUSTER_FIELDS
    dev = torch.device("cuda", 0)
    G = m.grid_size[0]

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

    t_host = timed(lambda: m.GetFrontierVoxels())
    hv, hm = m.GetFrontierVoxels()
    n = len(hv)
    cap = max(n, 1)
    t = {"vox": torch.empty((cap, 3), dtype=torch.int32, device=dev), "mask": torch.empty(cap, dtype=torch.uint8, device=dev),
         "label": torch.empty(cap, dtype=torch.int32, device=dev), "offsets": torch.empty(cap + 1, dtype=torch.int64, device=dev),
         "members": torch.empty(cap, dtype=torch.int64, device=dev), "head": torch.zeros(8, dtype=torch.int64, device=dev)}
    for field, dtype, shape in CLUSTER_FIELDS:
        t[field] = torch.empty((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    torch.cuda.synchronize()
    head = t["head"].data_ptr()
    outs = {k: t[k].data_ptr() for k in ("label", "offsets", "members") + PER_CLUSTER}

    def frontier():
        m.GetFrontierVoxelsDevice(None, None, 0.0, t["vox"].data_ptr(), t["mask"].data_ptr(), cap, head)

    def cluster(conn, min_size):
        m.ClusterVoxelsDevice(t["vox"].data_ptr(), cap, head + 8, mask_dev_ptr=t["mask"].data_ptr(), n_dev_ptr=head, connectivity=conn,
                              min_size=min_size, cluster_capacity=cap, member_capacity=cap, out=outs)

    def totals():
        return [int(v) for v in t["head"].cpu().numpy()[1:7]]

    t_frontier = timed(frontier)
    rows, checks = [], {}
    for conn, min_size in SETTINGS:
        frontier()
        t_cluster = timed(lambda: cluster(conn, min_size))
        alone = totals()
        t_chain = timed(lambda: (frontier(), cluster(conn, min_size)))
        checks[f"chain_totals_{conn}_{min_size}"] = totals() == alone and int(t["head"][0].item()) == n
        rows.append({"connectivity": conn, "min_size": min_size, "cluster_dev_ms": t_cluster * 1e3, "chain_dev_ms": t_chain * 1e3,
                     "entries_per_s": n / t_cluster if t_cluster > 0 else None, "K": alone[0], "largest": alone[5], "n_dropped_clusters": alone[4]})
    # the sample: the frontier voxels of a growing central sub-box, so that what is connected in it stays connected
    half = G // 2
    sample = np.zeros(len(hv), bool)
    for r in range(8, half + 1, 8):
        inside = ((hv >= half - r) & (hv < half + r)).all(axis=1)
        if inside.sum() > args.sample:
            break
        sample = inside
    sv, sm = np.ascontiguousarray(hv[sample]), np.ascontiguousarray(hm[sample])
    model_ms = {}
    for conn, min_size in SETTINGS:
        t0 = time.perf_counter()
        want = fiesta_amd.cluster_model(sv, mask=sm, connectivity=conn, min_size=min_size, resolution=m.resolution, origin=m.origin)
        model_ms[(conn, min_size)] = (time.perf_counter() - t0) * 1e3
        checks[f"sample_equals_model_{conn}_{min_size}"] = bool(same(m.ClusterVoxels(sv, mask=sm, connectivity=conn, min_size=min_size), want))
    scale = n / max(len(sv), 1)
    for row in rows:
        ms = model_ms[(row["connectivity"], row["min_size"])]
        row["model_ms"], row["model_scaled_ms"] = ms, ms * scale
        row["host_route_ms"] = t_host * 1e3 + ms * scale
        row["saved_ms"] = row["host_route_ms"] - row["chain_dev_ms"]
        row["cluster_over_frontier"] = row["cluster_dev_ms"] / (t_frontier * 1e3)
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    best = min(rows, key=lambda r: r["cluster_dev_ms"])
    out = {"metric": "cluster_entries_per_s", "value": best["entries_per_s"], "unit": "entries/s", "scene": name, "grid": G, "revision": rev,
           "source_sha256": source_digest(), "frontier_voxels": n, "sample_entries": int(len(sv)), "frontier_dev_ms": t_frontier * 1e3,
           "frontier_host_ms": t_host * 1e3, "copy_ms": (t_host - t_frontier) * 1e3, "settings": rows, "steps": args.steps, "warmup": args.warmup,
           "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"clusters_{name}.json"), "w").write(line + "\n")
    return out["all_checks"]


def main():
    from frontier_bench import build_cones, build_partial
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="partial512,cones256")
    ap.add_argument("--grid", type=int, default=0, help="override both scenes' grid (a multiple of 32; a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=30000, help="entries the host model is run on (scaled to the whole list)")
    ap.add_argument("--out", default=None, help="directory for clusters_<scene>.json")
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
