#!/usr/bin/env python3
"""View coverage (fiesta_hip_view_coverage[_dev]) on the frontier clusters of two maps an exploring robot produces, against the two
routes that existed before the call.

Scenes (tools/frontier_bench.py's, built here, nothing is read from disk):
  partial512  bench.py's C2-partial map: 512^3 @ 0.1 m, 27 % of its 32^3-voxel blocks never observed, 50 000 scattered obstacles
  cones256    256^3 @ 0.1 m observed through four view cones whose last voxel of range is a hit
Per scene: the frontier, its clusters (connectivity 26, min_size 10), a ring of 3 radii x 16 angles x 2 heights around every centroid,
a camera of 80 x 60 degrees (tan of the half angles) and 4.5 m range, block_mask OCCUPIED | UNKNOWN.  Measured in one run, p50 over
--steps calls after --warmup, a device synchronise around every call:
  fused_ms        fiesta_hip_view_coverage_dev, ring form, every output written
  pairs_per_s, surviving_per_s, walked_voxels_per_s   pairs, pairs in view and walked voxels (the ray query's n_visited over the
                  surviving segments) / fused time
  fused_cull_only_ms   the same call with max_range 1e-9: every pair generated and culled, none queued or walked; fused_minus_cull_ms is
                  what the queue, the walks and their reductions add
  route_a_ms      the device route a user had: pair generation and cull in torch (chunked), fiesta_hip_ray_query_dev on the surviving
                  segments (hit_index, hit_vox), a torch reduction per view.  It is handed the usable views for free.
  route_b_ms      fiesta_hip_ray_query_dev alone on those surviving segments, pre-built and resident (hit_index and hit_vox written);
                  route_b_all_ms: all six outputs written
Checked (the only pass / fail): the fused call's per-view counts, cover_count, first_view, best_view and best_count equal what route (a)'s
pairs give, on every view, target and cluster; on a sample of small clusters every
output equals fiesta_amd.view_coverage_model -- on every scene: of the first --sample-clusters clusters the --sample-size members nearest
the cluster's best pose, each a group of its own under the same ring, through the host variant of the call.
One JSON line per scene; with --out DIR it is also written to DIR/view_coverage_<scene>.json.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CHUNK = 1 << 25      # pairs per chunk of route (a)


def measure(name, m, args):
    import torch
    import fiesta_amd
    from fiesta_amd._lib import ViewResult
    from fiesta_amd.esdf_map import CLUSTER_FIELDS
    dev = torch.device("cuda", 0)
    res, org = m.resolution, torch.tensor(m.origin, dtype=torch.float64, device=dev)
    sensor = dict(min_range=0.0, max_range=4.5, tan_h=math.tan(math.radians(40.0)), tan_v=math.tan(math.radians(30.0)), block_mask=3, min_visible=1)
    ring = fiesta_amd.view_ring([1.0, 2.0, 3.0], 16, [0.0, 0.5])
    M = len(ring)

    def timed(fn, steps=args.steps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        m.synchronize()
        ts = []
        for _ in range(steps):
            m.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            m.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    hv, hm = m.GetFrontierVoxels()
    n = len(hv)
    cap = max(n, 1)
    t = {"vox": torch.from_numpy(hv).to(dev), "mask": torch.from_numpy(hm).to(dev), "label": torch.empty(cap, dtype=torch.int32, device=dev),
         "offsets": torch.empty(cap + 1, dtype=torch.int64, device=dev), "members": torch.empty(cap, dtype=torch.int64, device=dev),
         "head": torch.zeros(8, dtype=torch.int64, device=dev)}
    for field, dtype, shape in CLUSTER_FIELDS:
        t[field] = torch.empty((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    torch.cuda.synchronize()
    m.ClusterVoxelsDevice(t["vox"].data_ptr(), n, t["head"].data_ptr() + 8, mask_dev_ptr=t["mask"].data_ptr(), connectivity=26, min_size=10,
                          cluster_capacity=cap, member_capacity=cap, out={k: t[k].data_ptr() for k in ("label", "offsets", "members", "centroid", "size")})
    m.synchronize()
    K, n_members = int(t["head"][1].item()), int(t["head"][2].item())
    V = K * M
    ring_dev = torch.from_numpy(ring).to(dev)
    o = {"view_class": torch.empty(V, dtype=torch.uint8, device=dev), "n_in_view": torch.empty(V, dtype=torch.int32, device=dev),
         "n_visible": torch.empty(V, dtype=torch.int32, device=dev), "cover_count": torch.empty(cap, dtype=torch.int32, device=dev),
         "first_view": torch.empty(cap, dtype=torch.int32, device=dev), "best_view": torch.empty(max(K, 1), dtype=torch.int64, device=dev),
         "best_count": torch.empty(max(K, 1), dtype=torch.int32, device=dev)}
    info = torch.zeros(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def fused():
        m.ViewCoverageDevice(t["vox"].data_ptr(), n, info.data_ptr(), centroid_dev_ptr=t["centroid"].data_ptr(), ring_dev_ptr=ring_dev.data_ptr(), n_ring=M,
                             offsets_dev_ptr=t["offsets"].data_ptr(), members_dev_ptr=t["members"].data_ptr(), n_groups=K, n_members=n_members,
                             out={k: o[k].data_ptr() for k, _ in ViewResult._fields_}, **sensor)

    t_fused = timed(fused)
    n_usable, n_pairs, n_in_view, n_vis = (int(x) for x in info.cpu().numpy())
    # the same call with a range nothing lies in: every pair is generated and culled, none is queued or walked
    real = dict(sensor)
    sensor.update(max_range=1e-9)
    t_cull = timed(fused)
    culled_in_view = int(info.cpu().numpy()[2])
    sensor.clear()
    sensor.update(real)
    fused()
    m.synchronize()

    # ---- route (a): torch pair generation and cull, the ray query on the survivors, a torch reduction
    usable = o["n_visible"] >= 0                                                  # (handed to the route for free)
    pos = (t["centroid"][:K, None, :] + ring_dev[None, :, :3]).reshape(-1, 3)
    dirs = ring_dev[None, :, 3:].expand(K, M, 2).reshape(-1, 2)
    off = t["offsets"][:K + 1]
    sizes = (off[1:] - off[:-1]).repeat_interleave(M) * usable                    # pairs per view
    first = torch.cumsum(sizes, 0) - sizes
    centre = (t["vox"].to(torch.float64) + 0.5) * res + org
    keep = {}
    ends = np.cumsum(sizes.cpu().numpy())                                         # whole views per chunk of at most CHUNK pairs (or one view)
    cuts = sorted(set(np.minimum(np.searchsorted(ends, np.arange(CHUNK, int(ends[-1]) + CHUNK, CHUNK), side="right"), V).tolist() + [V])) if V else []
    cuts = [c for c in cuts if c > 0]

    def route_a(store=False):
        vin = torch.zeros(V, dtype=torch.int64, device=dev)
        vvis = torch.zeros(V, dtype=torch.int64, device=dev)
        S, E = [], []
        v0 = 0
        for v1 in cuts:
            if v1 == v0:
                continue
            sz = sizes[v0:v1]
            view = torch.repeat_interleave(torch.arange(v0, v1, device=dev), sz)
            if len(view):
                rank = torch.arange(len(view), device=dev) - torch.repeat_interleave(first[v0:v1] - first[v0], sz)
                ent = t["members"][off[view // M] + rank]
                q = centre[ent] - pos[view]
                d2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]
                fwd = q[:, 0] * dirs[view, 0] + q[:, 1] * dirs[view, 1]
                lat = q[:, 1] * dirs[view, 0] - q[:, 0] * dirs[view, 1]
                ok = (sensor["min_range"] ** 2 <= d2) & (d2 <= sensor["max_range"] ** 2) & (fwd > 0) & (lat.abs() <= sensor["tan_h"] * fwd) & \
                     (q[:, 2].abs() <= sensor["tan_v"] * fwd)
                view, ent = view[ok], ent[ok]
                s, e = pos[view].contiguous(), centre[ent].contiguous()
                k = len(view)
                if k:
                    hit = torch.empty(k, dtype=torch.int32, device=dev)
                    hvx = torch.empty((k, 3), dtype=torch.int32, device=dev)
                    torch.cuda.synchronize()                                      # (the map's stream does not wait for torch's)
                    m.RayQueryDevice(s.data_ptr(), e.data_ptr(), k, stop_mask=3, out={"hit_index": hit.data_ptr(), "hit_vox": hvx.data_ptr()})
                    m.synchronize()
                    seen = (hit == -1) | (hvx == t["vox"][ent]).all(1)
                    vin.index_add_(0, view, torch.ones_like(view))
                    vvis.index_add_(0, view, seen.to(torch.int64))
                    if store:     # (the checking pass only: the segments for route (b), the per-target outputs)
                        S.append(s), E.append(e)
                        keep["cover"].index_add_(0, ent[seen], torch.ones_like(ent[seen]))
                        keep["first"].scatter_reduce_(0, ent[seen], view[seen], "amin")
            v0 = v1
        if store:
            keep["start"], keep["end"] = torch.cat(S) if S else torch.zeros((0, 3), device=dev), torch.cat(E) if E else torch.zeros((0, 3), device=dev)
        return vin, vvis

    keep["cover"] = torch.zeros(cap, dtype=torch.int64, device=dev)
    keep["first"] = torch.full((cap,), 1 << 40, dtype=torch.int64, device=dev)
    vin, vvis = route_a(store=True)
    checks = {"in_view_equals_route_a": bool((vin[usable] == o["n_in_view"][usable]).all().item()),
              "visible_equals_route_a": bool((vvis[usable] == o["n_visible"][usable]).all().item())}
    # per target and per group out of route (a)'s pairs: cover_count, first_view; the view with most visible pairs, the lowest among equals
    checks["cover_count_equals_route_a"] = bool((keep["cover"][:n] == o["cover_count"][:n]).all().item())
    checks["first_view_equals_route_a"] = bool((torch.where(keep["first"][:n] == 1 << 40, -1, keep["first"][:n]) == o["first_view"][:n]).all().item())
    counts = torch.where(usable, vvis, torch.full_like(vvis, -1)).reshape(K, M).cpu().numpy()
    arg = counts.argmax(1)                                                        # (numpy: the first maximum)
    top = counts[np.arange(K), arg]
    good = top >= sensor["min_visible"]
    checks["best_equals_route_a"] = bool(np.array_equal(o["best_view"][:K].cpu().numpy(), np.where(good, np.arange(K) * M + arg, -1)) and
                                         np.array_equal(o["best_count"][:K].cpu().numpy(), np.where(good, top, 0)))
    t_a = timed(route_a)

    # ---- route (b): the ray query alone on the surviving segments
    ns = len(keep["start"])
    rb = {"n_visited": torch.empty(max(ns, 1), dtype=torch.int32, device=dev), "hit_index": torch.empty(max(ns, 1), dtype=torch.int32, device=dev),
          "hit_class": torch.empty(max(ns, 1), dtype=torch.uint8, device=dev), "hit_vox": torch.empty((max(ns, 1), 3), dtype=torch.int32, device=dev),
          "hit_dist": torch.empty(max(ns, 1), dtype=torch.float64, device=dev), "counts": torch.empty((max(ns, 1), 4), dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    t_b = t_b_all = None
    walked = 0
    if ns:
        two = {k: rb[k].data_ptr() for k in ("hit_index", "hit_vox")}
        t_b = timed(lambda: m.RayQueryDevice(keep["start"].data_ptr(), keep["end"].data_ptr(), ns, stop_mask=3, out=two))
        t_b_all = timed(lambda: m.RayQueryDevice(keep["start"].data_ptr(), keep["end"].data_ptr(), ns, stop_mask=3, out={k: v.data_ptr() for k, v in rb.items()}))
        walked = int(rb["n_visited"][:ns].to(torch.int64).sum().item())
    checks["survivors_equal_pairs_in_view"] = ns == n_in_view

    # ---- the model on a sample: of the first clusters, the members nearest the cluster's best pose (its centroid if it has none), each
    #      sample a group of its own under the same ring around the same centroid -- the host variant of the call against the model
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0
    offs, mem, cen = t["offsets"][:K + 1].cpu().numpy(), t["members"][:n_members].cpu().numpy(), t["centroid"][:K].cpu().numpy()
    best = o["best_view"][:K].cpu().numpy()
    pick = np.arange(min(K, args.sample_clusters))
    seg = []
    for k in pick:
        members = mem[offs[k]:offs[k + 1]]
        near = cen[k] + (ring[best[k] % M, :3] if best[k] >= 0 else 0.0)
        d = np.linalg.norm((hv[members] + 0.5) * res + np.asarray(m.origin) - near, axis=1)
        seg.append(members[np.argsort(d, kind="stable")[:args.sample_size]])
    if len(pick):
        kw = dict(centroid=cen[pick], ring=ring, offsets=np.concatenate([[0], np.cumsum([len(x) for x in seg])]), members=np.concatenate(seg), **sensor)
        want = fiesta_amd.view_coverage_model(obs, occ, m.origin, res, hv, pos_range=m.pos_range, **kw)
        got = m.ViewCoverage(hv, **kw)
        checks["sample_equals_model"] = all(np.array_equal(got[k], want[k]) for k in want)
        checks["sample_not_vacuous"] = bool(0 < want["pairs_visible"] < want["n_pairs"])
    else:
        checks["sample_equals_model"] = False        # (no cluster: nothing was checked against the model)
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    out = {"metric": "view_pairs_per_s", "value": n_pairs / t_fused if t_fused > 0 else None, "unit": "pairs/s", "scene": name, "grid": m.grid_size[0],
           "revision": rev, "source_sha256": source_digest(), "frontier_voxels": n, "clusters": K, "members": n_members, "views": V, "usable_views": n_usable,
           "pairs": n_pairs, "pairs_in_view": n_in_view, "pairs_visible": n_vis, "walked_voxels": walked, "fused_ms": t_fused * 1e3, "fused_cull_only_ms": t_cull * 1e3,
           "fused_minus_cull_ms": (t_fused - t_cull) * 1e3, "cull_only_pairs_in_view": culled_in_view,
           "route_a_ms": t_a * 1e3, "route_b_ms": None if t_b is None else t_b * 1e3, "route_b_all_ms": None if t_b_all is None else t_b_all * 1e3,
           "surviving_per_s": n_in_view / t_fused, "walked_voxels_per_s": walked / t_fused, "route_a_over_fused": t_a / t_fused,
           "route_b_over_fused": None if t_b is None else t_b / t_fused, "sample_clusters": int(len(pick)), "steps": args.steps, "warmup": args.warmup,
           "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"view_coverage_{name}.json"), "w").write(line + "\n")
    return out["all_checks"]


def main():
    from frontier_bench import build_cones, build_partial
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cones256,partial512")
    ap.add_argument("--grid", type=int, default=0, help="override both scenes' grid (a multiple of 32; a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample-clusters", type=int, default=6, help="clusters the host model is run on")
    ap.add_argument("--sample-size", type=int, default=300, help="members of each sampled cluster (those nearest its best pose)")
    ap.add_argument("--out", default=None, help="directory for view_coverage_<scene>.json")
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
