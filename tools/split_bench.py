#!/usr/bin/env python3
"""Cluster splitting (fiesta_hip_split_clusters[_dev]) on the whole-map frontier of two maps an exploring robot produces, against the
cluster call that feeds it and against the routes a user had before.

Scenes (tools/cluster_bench.py's, built here, nothing is read from disk): partial512 and cones256; the whole frontier is clustered
once at connectivity 26, min_size 1, and its CSR pair stays on the device.
Measured per scene in one run, p50 over --steps calls after --warmup, a device synchronise around every call; per setting
(max_size 256, max_size 4096, max_extent 16; max_depth 63):
  split_dev_ms       the device variant on the resident cluster outputs, every output written, part_capacity = members
  split_host_ms      the host variant on host copies of the same arrays (staging, copy-back, one synchronise)
  P, largest, depth  what the call found;  members_per_s = members / split_dev time
  numpy_ms           the parent commit's first route: a vectorised numpy statement of the rule (level by level over all parts with
                     np.minimum.reduceat / a stable sort) on host copies;  copy_back_ms: fetching offsets and members for it
  checked            on a sample of clusters (at most --sample members) every output of the host call equals fiesta_amd.split_model,
                     and the numpy route's part sizes and boxes equal the device's on the whole list
and once per scene:
  cluster_dev_ms     the cluster call that feeds the split: the yardstick next to it
  recluster_ms       the parent commit's second route, the trick of tools/reach_matrix_bench.py: the cluster call on fv + fv // 16,
                     which tears the lattice at a fixed grid (no bound on a part's size, centroids in warped coordinates)
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/split_bench.py` (a run of its own).
One JSON line per scene; with --out DIR it is also written to DIR/split_<scene>.json.
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
SETTINGS = (dict(max_size=256), dict(max_size=4096), dict(max_extent=16))
PER_PART = ("parent", "depth", "size", "root", "box_lo", "box_hi", "centroid", "mask_or", "key_min", "key_argmin")
TOTALS = ("n_parts", "n_members", "n_split_clusters", "n_oversize", "largest", "deepest", "status")


def same(got, want):
    for k in TOTALS:
        if got[k] != want[k]:
            return False
    for k in ("label", "offsets") + PER_PART:
        if not np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(want[k]).view(np.uint8)):
            return False
    off = want["offsets"]
    return all(sorted(got["members"][off[k]:off[k + 1]].tolist()) == sorted(want["members"][off[k]:off[k + 1]].tolist()) for k in range(len(off) - 1))


def numpy_split(v, off, mem, max_size=0, max_extent=0, max_depth=63):
    """the rule, vectorised over all parts of a level: returns (sizes, box_lo, box_hi) of the final parts in the rule's order"""
    keep = np.diff(off) > 0
    start = off[:-1][keep].astype(np.int64)
    end = int(off[-1])
    mem = mem.copy()
    active = np.ones(len(start), bool)                                    # parts that may still be oversize
    for _ in range(max_depth):
        P = len(start)
        if not P:
            break
        size = np.diff(np.append(start, end))
        part = np.repeat(np.arange(P), size)
        c = v[mem[start[0]:end]].astype(np.int64) if P else np.zeros((0, 3), np.int64)
        lo, hi = np.minimum.reduceat(c, start - start[0], axis=0), np.maximum.reduceat(c, start - start[0], axis=0)   # (parts are contiguous)
        ext = hi - lo + 1
        over = active & (ext.max(1) >= 2) & (((max_size > 0) & (size > max_size)) | ((max_extent > 0) & (ext.max(1) > max_extent)))
        if not over.any():
            break
        axis = ext.argmax(1)
        mid = lo[np.arange(P), axis] + ((hi[np.arange(P), axis] - lo[np.arange(P), axis]) >> 1)
        high = over[part] & (c[np.arange(len(c)), axis[part]] > mid[part])
        order = np.lexsort((high, part))                                  # stable: by part, low before high
        mem[start[0]:end] = mem[start[0]:end][order]
        n_high = np.bincount(part, weights=high, minlength=P).astype(np.int64)
        second = start + size - n_high
        new_start = np.empty(P + int(over.sum()), np.int64)
        new_active = np.zeros(len(new_start), bool)
        at = np.arange(P) + np.concatenate([[0], np.cumsum(over)[:-1]])
        new_start[at] = start
        new_start[at[over] + 1] = second[over]
        new_active[at[over]] = new_active[at[over] + 1] = True
        start, active = new_start, new_active
    P = len(start)
    size = np.diff(np.append(start, end))
    c = v[mem[start[0]:end]].astype(np.int64) if P else np.zeros((0, 3), np.int64)
    if not P:
        return size, np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    return size, np.minimum.reduceat(c, start - start[0], axis=0), np.maximum.reduceat(c, start - start[0], axis=0)


def measure(name, m, args):
    import torch
    import fiesta_amd
    from fiesta_amd._lib import ClusterResult, SplitResult
    from fiesta_amd.esdf_map import CLUSTER_FIELDS, SPLIT_FIELDS
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

    hv, hm = m.GetFrontierVoxels()
    n = len(hv)
    cap = max(n, 1)
    c = {"vox": torch.from_numpy(hv).to(dev), "mask": torch.from_numpy(hm).to(dev), "label": torch.empty(cap, dtype=torch.int32, device=dev),
         "offsets": torch.empty(cap + 1, dtype=torch.int64, device=dev), "members": torch.empty(cap, dtype=torch.int64, device=dev),
         "head": torch.zeros(8, dtype=torch.int64, device=dev)}
    for field, dtype, shape in CLUSTER_FIELDS:
        c[field] = torch.empty((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    s = {"label": torch.empty(cap, dtype=torch.int32, device=dev), "offsets": torch.empty(cap + 1, dtype=torch.int64, device=dev),
         "members": torch.empty(cap, dtype=torch.int64, device=dev), "info": torch.zeros(7, dtype=torch.int64, device=dev)}
    for field, dtype, shape in SPLIT_FIELDS:
        s[field] = torch.empty((cap,) + shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    warped = torch.from_numpy(np.ascontiguousarray(hv + hv // 16)).to(dev)
    torch.cuda.synchronize()
    head = c["head"].data_ptr()

    def cluster(vox=c["vox"]):
        m.ClusterVoxelsDevice(vox.data_ptr(), n, head + 8, mask_dev_ptr=c["mask"].data_ptr(), connectivity=26, min_size=1, cluster_capacity=cap,
                              member_capacity=cap, out={k: c[k].data_ptr() for k, _ in ClusterResult._fields_})

    def split(**kw):
        m.SplitClustersDevice(c["vox"].data_ptr(), n, c["offsets"].data_ptr(), c["members"].data_ptr(), cap, cap, s["info"].data_ptr(),
                              mask_dev_ptr=c["mask"].data_ptr(), n_clusters_dev_ptr=head + 8, part_capacity=cap,
                              out={k: s[k].data_ptr() for k, _ in SplitResult._fields_}, **kw)

    t_recluster = timed(lambda: cluster(warped))
    recl = [int(x) for x in c["head"].cpu().numpy()[1:7]]
    t_cluster = timed(cluster)
    K, M = int(c["head"][1].item()), int(c["head"][2].item())
    t_copy = timed(lambda: (c["offsets"][:K + 1].cpu(), c["members"][:M].cpu()))
    off, mem = c["offsets"][:K + 1].cpu().numpy(), c["members"][:M].cpu().numpy()
    sizes = np.diff(off)
    # the sample: whole clusters, largest first, as long as they fit into half of --sample; then, of the largest cluster, the first
    # members in (x, y, z) order that fill the other half (a slab of it: the rule does not care whether a segment is connected)
    pick, total = [], 0
    for k in np.argsort(-sizes, kind="stable"):
        if total + sizes[k] <= args.sample // 2:
            pick.append(int(k))
            total += int(sizes[k])
    pick.sort()
    segs = [mem[off[k]:off[k + 1]] for k in pick]
    if K and int(np.argmax(sizes)) not in pick:
        big = mem[off[np.argmax(sizes)]:off[np.argmax(sizes) + 1]]
        bv = hv[big]
        segs.append(big[np.lexsort((bv[:, 2], bv[:, 1], bv[:, 0]))[:args.sample // 2]])
    s_mem = np.concatenate(segs).astype(np.int64) if segs else np.zeros(0, np.int64)
    s_off = np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64)
    rows, checks = [], {}
    for kw in SETTINGS:
        tag = "_".join(f"{k}{v}" for k, v in kw.items())
        t_dev = timed(lambda: split(**kw))
        info = dict(zip(TOTALS, (int(x) for x in s["info"].cpu().numpy())))
        t_host = timed(lambda: m.SplitClusters(hv, off, mem, mask=hm, **kw), steps=max(args.steps // 4, 3), warmup=1)
        print(f"[split_bench] {name} {tag}: device {t_dev * 1e3:.3f} ms, host {t_host * 1e3:.3f} ms", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        np_size, np_lo, np_hi = numpy_split(hv, off, mem, **kw)
        t_numpy = time.perf_counter() - t0
        P = info["n_parts"]
        checks[f"numpy_route_equals_device_{tag}"] = bool(len(np_size) == P and np.array_equal(np_size, s["size"][:P].cpu().numpy())
                                                          and np.array_equal(np_lo, s["box_lo"][:P].cpu().numpy())
                                                          and np.array_equal(np_hi, s["box_hi"][:P].cpu().numpy()))
        want = fiesta_amd.split_model(hv, s_off, s_mem, mask=hm, resolution=m.resolution, origin=m.origin, **kw)
        checks[f"sample_equals_model_{tag}"] = bool(same(m.SplitClusters(hv, s_off, s_mem, mask=hm, **kw), want))
        checks[f"status_ok_{tag}"] = info["status"] == 0 and info["n_oversize"] == 0 and info["n_members"] == M
        rows.append(dict(kw, split_dev_ms=t_dev * 1e3, split_host_ms=t_host * 1e3, numpy_ms=t_numpy * 1e3, numpy_route_ms=(t_numpy + t_copy) * 1e3,
                         members_per_s=M / t_dev if t_dev > 0 else None, P=P, largest=info["largest"], depth=info["deepest"],
                         n_split_clusters=info["n_split_clusters"], split_over_cluster=t_dev / t_cluster))
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    best = min(rows, key=lambda r: r["split_dev_ms"])
    out = {"metric": "split_members_per_s", "value": best["members_per_s"], "unit": "members/s", "scene": name, "grid": G, "revision": rev,
           "source_sha256": source_digest(), "frontier_voxels": n, "clusters": K, "members": M, "largest_cluster": int(sizes.max()) if K else 0,
           "sample_members": int(len(s_mem)), "sample_clusters": len(segs), "cluster_dev_ms": t_cluster * 1e3, "copy_back_ms": t_copy * 1e3,
           "recluster_ms": t_recluster * 1e3, "recluster_K": recl[0], "recluster_largest": recl[5], "settings": rows, "steps": args.steps,
           "warmup": args.warmup, "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"split_{name}.json"), "w").write(line + "\n")
    return out["all_checks"]


def main():
    from frontier_bench import build_cones, build_partial
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="partial512,cones256")
    ap.add_argument("--grid", type=int, default=0, help="override both scenes' grid (a multiple of 32; a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=20000, help="members the host model is run on (whole clusters)")
    ap.add_argument("--out", default=None, help="directory for split_<scene>.json")
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
