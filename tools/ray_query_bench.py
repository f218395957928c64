#!/usr/bin/env python3
"""Batched ray queries (fiesta_hip_ray_query[_dev]) on the maps and ray sets a planner produces, against the route that existed
before for the same voxels.

Workloads (built here, nothing is read from disk):
  frame    bench.py's C3 map (512^3 @ 0.1 m, a box room with spheres, --frames depth frames of a yaw sweep cast and fused) and the
           rays of ONE more 640 x 480 depth frame: start = the sensor, end = the frame's end points (clipped to the ray window as the
           ray cast clips them); stop_mask 0 (the whole walk), 1 (first obstacle: expected depth) and 7 (line of sight).
           Yardstick, timed in the same run on the same points: fiesta_hip_raycast_frame[_dev] with dedup = 0 -- the same traversal,
           which additionally counts an observation per voxel.
  segments bench.py's C2-partial map (512^3, 27 % of its 32^3-voxel blocks never observed, 50 000 scattered obstacles) and
           --segments random segments of 0.5 .. 10 m inside it, stop_mask 7 (line of sight for shortcutting)
  views    the same map: 64 candidate views at frontier voxels with 0.3 m clearance (fiesta_hip_get_frontier_voxels), 4096 rays of
           5 m each in uniformly random directions per view, stop_mask 1; the gain of a view is the sum of its rays' counts[2]
Measured, p50 over --steps calls after --warmup with a synchronise around every call: the device variant (inputs and outputs
resident; what a planner on the device runs) and the host variant (stages, synchronises, copies back); rays/s and visited voxels/s
(sum of n_visited over the valid rays) from the device variant.
Checked: every output of --check rays per workload and stop mask (evenly spaced through the batch) equals fiesta_amd.ray_query_model
on the map's download_field, bit for bit; the device variant equals the host variant on the whole batch.
One JSON line per workload; with --out DIR also written to DIR/ray_queries_<workload>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/ray_query_bench.py` (a run of its own).
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
FIELDS = ("n_visited", "hit_index", "hit_class", "hit_vox", "hit_dist", "counts")


def build_c3(G, frames):
    """run_c3's map after `frames` frames; returns the map, the next frame's sensor-frame points (f32), its pose and ray window"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scenarios import INTRINSICS as intr, P_DEFAULT, depth_to_points, render_depth, yaw_pose
    import fiesta_amd
    res, half = 0.1, G * 0.1 / 2
    origin, size = (-half, -half, -half), (G * res,) * 3
    m = fiesta_amd.ESDFMap(origin, res, size)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    spheres = [((1.5, 0.5, 0.0), 0.5), ((-1.0, 2.0, 0.3), 0.7), ((0.5, -2.0, -0.5), 0.4), ((-2.0, -1.0, 0.5), 0.6), ((2.2, -1.8, 0.2), 0.3)]
    scale = min(1.0, G / 512.0)   # (a rehearsal at a small grid: the room shrinks with it)
    room = ((-3.0 * scale, -3.0 * scale, -1.5 * scale), (3.0 * scale, 3.0 * scale, 1.5 * scale))
    spheres = [(tuple(np.multiply(c, scale)), r * scale) for c, r in spheres]
    lc, rc = origin, tuple(np.add(origin, size))
    window = (0.5 * scale, 5.0 * scale)
    for f in range(frames + 1):
        T = yaw_pose(2.0 * f, (0.0, 0.0, 0.0))
        depth = render_depth(T, rows=480, cols=640, room=room, spheres=spheres, intr=intr)
        if f == frames:
            return m, depth_to_points(depth, intr), T, window, lc, rc
        m.RaycastDepth(depth, intr["fx"], intr["fy"], intr["cx"], intr["cy"], T, T[:3, 3], window[0], window[1], lc, rc, dedup=1)
        m.UpdateOccupancy(True)
        m.UpdateESDF()


def frame_rays(points, T, window):
    """start / end of the frame's rays as RaycastProcess forms them (include/Fiesta.h:202-213): transformed in f64, clipped to
    max_ray_length; a point closer than min_ray_length casts nothing and is left out"""
    p = points.astype(np.float64)
    h = p @ T[:3, :3].T + T[:3, 3]
    o = T[:3, 3]
    d = h - o
    ln = np.sqrt((d * d).sum(1))
    keep = np.isfinite(ln) & (ln >= window[0])
    far = ln > window[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(far[:, None], d / ln[:, None] * window[1] + o, h)
    return np.repeat(o[None], int(keep.sum()), 0).copy(), np.ascontiguousarray(h[keep]), keep


class Timer:
    def __init__(self, m, steps, warmup):
        self.m, self.steps, self.warmup = m, steps, warmup

    def __call__(self, fn):
        for _ in range(self.warmup):
            fn()
        self.m.synchronize()
        ts = []
        for _ in range(self.steps):
            self.m.synchronize()
            t0 = time.perf_counter()
            fn()
            self.m.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)


def same(a, b):
    for k in FIELDS:
        x, y = a[k], b[k]
        if k == "hit_dist":
            ok = ~np.isnan(y)
            if not (np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[ok].view(np.uint64), y[ok].view(np.uint64))):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


class Queries:
    """device buffers for one batch of rays, both variants of the call, the model on a sample"""

    def __init__(self, m, start, end, timer, check):
        import torch
        self.m, self.start, self.end, self.timer, self.check = m, np.ascontiguousarray(start), np.ascontiguousarray(end), timer, check
        dev = torch.device("cuda", 0)
        n = self.n = len(start)
        self.s, self.e = torch.from_numpy(self.start).to(dev), torch.from_numpy(self.end).to(dev)
        shapes = {"n_visited": ((n,), torch.int32), "hit_index": ((n,), torch.int32), "hit_class": ((n,), torch.uint8),
                  "hit_vox": ((n, 3), torch.int32), "hit_dist": ((n,), torch.float64), "counts": ((n, 4), torch.int32)}
        self.out = {k: torch.zeros(shapes[k][0], dtype=shapes[k][1], device=dev) for k in FIELDS}
        self.ptrs = {k: t.data_ptr() for k, t in self.out.items()}
        torch.cuda.synchronize()
        self.field = None

    def model_sample(self, mask, got):
        import fiesta_amd
        m = self.m
        if self.field is None:
            f = m.download_field(("d2", "occ"))
            self.field = ((f["d2"] >= 0).reshape(m.grid_size), f["occ"].reshape(m.grid_size) != 0)
        idx = np.unique(np.linspace(0, self.n - 1, min(self.check, self.n)).astype(np.int64))
        want = fiesta_amd.ray_query_model(self.field[0], self.field[1], m.origin, m.resolution, self.start[idx], self.end[idx], mask,
                                          pos_range=m.pos_range)
        return same({k: v[idx] for k, v in got.items()}, want), len(idx)

    def run(self, mask):
        m = self.m
        t_dev = self.timer(lambda: m.RayQueryDevice(self.s.data_ptr(), self.e.data_ptr(), self.n, mask, self.ptrs))
        got = {k: t.cpu().numpy() for k, t in self.out.items()}
        host = {}

        def host_call():
            host.update(m.RayQuery(self.start, self.end, mask))
        t_host = self.timer(host_call)
        ok_model, n_checked = self.model_sample(mask, got)
        valid = got["n_visited"] >= 0
        visited = int(got["n_visited"][valid].sum())
        return {"stop_mask": mask, "dev_ms": t_dev * 1e3, "host_ms": t_host * 1e3, "rays_per_s": self.n / t_dev, "visited": visited,
                "visited_voxels_per_s": visited / t_dev, "mean_visited": visited / max(int(valid.sum()), 1), "invalid_rays": int((~valid).sum()),
                "hits": int((got["hit_index"] >= 0).sum()), "unknown_before_hit": int(got["counts"][:, 2].sum()),
                "checks": {"sample_equals_model": bool(ok_model), "sample": n_checked, "device_equals_host": bool(same(got, host))}}, got


def emit(args, name, out):
    from path_query_bench import source_digest
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    out.update({"workload": name, "revision": rev, "source_sha256": source_digest(), "steps": args.steps, "warmup": args.warmup})
    out["all_checks"] = all(all(v for k, v in r["checks"].items() if k != "sample") for r in out["runs"])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"ray_queries_{name}.json"), "w").write(line + "\n")
    return out["all_checks"]


def workload_frame(args):
    import torch
    from fiesta_amd._lib import RaycastParams, check
    G = args.grid or 512
    m, points, T, window, lc, rc = build_c3(G, args.frames)
    timer = Timer(m, args.steps, args.warmup)
    start, end, keep = frame_rays(points, T, window)
    q = Queries(m, start, end, timer, args.check)
    runs = [q.run(mask)[0] for mask in (0, 1, 7)]
    # the yardstick, after the queries (it adds pending observations; the classes only change at UpdateOccupancy): the casting
    # points of the same frame through the ray cast without de-duplication, host and device variant
    pts = np.ascontiguousarray(points[keep], np.float32)
    o = np.ascontiguousarray(T[:3, 3], np.float64)
    Tf = np.ascontiguousarray(T, np.float64).reshape(16)
    prm = RaycastParams(window[0], window[1], (C.c_double * 3)(*lc), (C.c_double * 3)(*rc), 0, 0)
    dpts = torch.from_numpy(pts).to("cuda:0")
    torch.cuda.synchronize()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    t_cast_host = timer(lambda: check(m._lib.fiesta_hip_raycast_frame(m._h, vp(pts), len(pts), vp(Tf), vp(o), C.byref(prm))))
    t_cast_dev = timer(lambda: check(m._lib.fiesta_hip_raycast_frame_dev(m._h, C.c_void_p(dpts.data_ptr()), len(pts), vp(Tf), vp(o), C.byref(prm))))
    out = {"metric": "ray_query_stop0_over_raycast_frame", "value": runs[0]["dev_ms"] / (t_cast_dev * 1e3), "unit": "x", "grid": G, "rays": len(start),
           "frames_fused": args.frames, "raycast_frame_dedup0_dev_ms": t_cast_dev * 1e3, "raycast_frame_dedup0_host_ms": t_cast_host * 1e3,
           "runs": runs, "dev_over_raycast_dev": {str(r["stop_mask"]): r["dev_ms"] / (t_cast_dev * 1e3) for r in runs},
           "host_over_raycast_host": {str(r["stop_mask"]): r["host_ms"] / (t_cast_host * 1e3) for r in runs}}
    m.close()
    return emit(args, "frame", out)


def workload_partial(args, which):
    from frontier_bench import build_partial
    G = args.grid or 512
    m = build_partial(G, int(round(50000 * (G / 512.0) ** 3)))
    timer = Timer(m, args.steps, args.warmup)
    rng = np.random.RandomState(99)
    size = G * 0.1
    ok = True
    if "segments" in which:
        n = args.segments
        start = rng.rand(n, 3) * size
        d = rng.randn(n, 3)
        d /= np.linalg.norm(d, axis=1)[:, None]
        end = np.clip(start + d * rng.uniform(0.5, 10.0, (n, 1)), 0.0, size - 1e-9)
        run, _ = Queries(m, start, end, timer, args.check).run(7)
        ok &= emit(args, "segments", {"metric": "ray_query_segments_rays_per_s", "value": run["rays_per_s"], "unit": "rays/s", "grid": G, "rays": n,
                                      "runs": [run]})
    if "views" in which:
        vox, _ = m.GetFrontierVoxels(min_clearance=0.3, want_mask=False)
        views = vox[rng.choice(len(vox), 64, replace=len(vox) < 64)]
        centres = (views + 0.5) * 0.1
        d = rng.randn(64, 4096, 3)
        d /= np.linalg.norm(d, axis=2)[:, :, None]
        start = np.repeat(centres[:, None], 4096, 1).reshape(-1, 3)
        end = start + d.reshape(-1, 3) * min(5.0, size / 4)
        run, got = Queries(m, start, end, timer, args.check).run(1)
        gain = got["counts"][:, 2].reshape(64, 4096).sum(1)
        ok &= emit(args, "views", {"metric": "ray_query_views_rays_per_s", "value": run["rays_per_s"], "unit": "rays/s", "grid": G, "rays": len(start),
                                   "views": 64, "frontier_voxels_clear_0.3": int(len(vox)), "gain_min_median_max": [int(gain.min()), int(np.median(gain)), int(gain.max())],
                                   "runs": [run]})
    m.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="frame,segments,views")
    ap.add_argument("--grid", type=int, default=0, help="override the maps' grid (a multiple of 32; a rehearsal at a small size)")
    ap.add_argument("--frames", type=int, default=8, help="frame: depth frames cast and fused before the measured one")
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=2000, help="rays per run compared with the model")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for ray_queries_<workload>.json")
    args = ap.parse_args()
    which = args.workloads.split(",")
    ok = True
    if "frame" in which:
        ok &= workload_frame(args)
    if "segments" in which or "views" in which:
        ok &= workload_partial(args, which)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
