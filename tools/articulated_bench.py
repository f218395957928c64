#!/usr/bin/env python3
"""Articulated body queries against the route that exists without them, on the map and planner batch of tools/body_query_bench.py.

Config 2's map (512^3 @ 0.1 m, 50 000 scattered obstacles, fully observed).  100 000 configurations: base positions drawn (seeded)
from that batch's waypoints; every frame within 0.5 m of the base on every axis, with a seeded random quaternion of norm 0.5 .. 2.
Bodies of (K spheres, F frames) = (8, 2), (64, 7), (105, 7), (512, 16), the spheres dealt evenly over the frames, each inside a ball
0.5 m wide about its frame's origin.  Per body, over IDENTICAL configurations:
  articulated  (a) fiesta_hip_articulated_query_dev, all ten outputs
  per_frame    (b) the route that exists without it: one fiesta_hip_body_query_dev per frame with that frame's spheres and poses
               (all eight outputs each), then torch: the minimum and arg-minimum across the frames, the sums of the counts and costs
  rigid        (c) fiesta_hip_body_query_dev of a rigid body of the same K spheres at N poses, all eight outputs: the floor
p50 of each (device synchronise around every call, warm-up first; fewer repetitions for the large K, whose calls are long), the
first 500 configurations checked against fiesta_amd.articulated_query_model (exact outputs by bits, the sums within the header's
bound), the minimum and the count checked against route (b) on all configurations, one JSON line, also written to
DIR/articulated_query.json.  `source_sha256` identifies the measured sources independently of git.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/articulated_bench.py` (a run of its own).
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

BODIES = ((8, 2), (64, 7), (105, 7), (512, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--configs", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="directory for articulated_query.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from bench import P_DEFAULT, Workload
    from fiesta_amd.esdf_map import ARTICULATED_FIELDS, BODY_FIELDS
    from path_query_bench import planner_polylines, source_digest
    G, res, dev = args.grid, 0.1, torch.device("cuda", 0)
    m = fiesta_amd.ESDFMap((0, 0, 0), res, (G * res,) * 3)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((0, 0, 0), (G - 1,) * 3, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    wl = Workload(G, args.obstacles, seed=12345)
    for _ in range(3):
        m.SetOccupancy(wl.initial(), 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    w, _ = planner_polylines(G, res, dev)
    rng = np.random.RandomState(2025)
    N, margin = args.configs, args.margin
    base = w[torch.from_numpy(rng.choice(len(w), N, replace=False)).to(dev)].cpu().numpy()

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    def tensors(fields, dims):
        outs = {name: torch.empty((N,) + tuple(dims.get(d, d) for d in shape), dtype=torch.float64 if dt == np.float64 else torch.int32,
                                  device=dev) for name, dt, shape in fields}
        return outs, {k: v.data_ptr() for k, v in outs.items()}

    rows, ok = [], True
    for K, F in BODIES:
        frm = np.sort(np.arange(K) % F).astype(np.int32)
        c = rng.randn(K, 3)
        c *= (0.25 * rng.rand(K) ** (1 / 3) / np.linalg.norm(c, axis=1))[:, None]
        sph = np.ascontiguousarray(np.concatenate([c, rng.rand(K, 1) * 0.15], 1))
        quat = rng.randn(N, F, 4)
        quat *= (2.0 ** rng.uniform(-1, 1, (N, F)) / np.linalg.norm(quat, axis=2))[:, :, None]
        poses_np = np.ascontiguousarray(np.concatenate([base[:, None, :] + rng.uniform(-0.5, 0.5, (N, F, 3)), quat], 2))
        poses = torch.from_numpy(poses_np).to(dev)
        outs, ptrs = tensors(ARTICULATED_FIELDS, {"K": K, "F": F})
        # route (b): the frame's own spheres, its poses gathered once (not timed: a caller's kinematics would write them per frame)
        first = np.searchsorted(frm, np.arange(F + 1))
        first_t = torch.from_numpy(first[:-1].astype(np.int32)).to(dev)
        per_frame = []
        for f in range(F):
            k_f = int(first[f + 1] - first[f])
            o, p = tensors(BODY_FIELDS, {"K": k_f})
            per_frame.append((np.ascontiguousarray(sph[first[f]:first[f + 1]]), poses[:, f].contiguous(), o, p))
        rigid_out, rigid_ptrs = tensors(BODY_FIELDS, {"K": K})
        rigid_poses = poses[:, 0].contiguous()
        torch.cuda.synchronize()
        steps = args.steps if K <= 64 else max(5, args.steps // 4)
        state = {}

        def route_b():
            for s_f, p_f, _, ptr_f in per_frame:
                m.BodyQueryDevice(s_f, p_f.data_ptr(), N, margin, ptr_f)
            m.synchronize()          # the map's stream -> torch's reductions: the streams do not wait for each other
            mins = torch.stack([o["min_clearance"] for _, _, o, _ in per_frame], 1)
            best, frame = mins.min(1)
            local = torch.stack([o["min_sphere"] for _, _, o, _ in per_frame], 1).gather(1, frame[:, None])[:, 0]
            state["out"] = {"min_clearance": best, "min_sphere": local + first_t[frame],
                            "n_below": torch.stack([o["n_below"] for _, _, o, _ in per_frame], 1).sum(1),
                            "cost": torch.stack([o["cost"] for _, _, o, _ in per_frame], 1).sum(1)}

        t_a = timed(lambda: m.ArticulatedQueryDevice(sph, frm, F, poses.data_ptr(), N, margin, ptrs), steps)
        t_b = timed(route_b, steps)
        t_c = timed(lambda: m.BodyQueryDevice(sph, rigid_poses.data_ptr(), N, margin, rigid_ptrs), steps)
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        want = fiesta_amd.articulated_query_model(m.GetDistWithGradTrilinear, sph, frm, F, poses_np[:500], margin)
        tr = {k: v.cpu().numpy() for k, v in state["out"].items()}
        bits = lambda a: np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a   # noqa: E731
        checks = {k: bool(np.array_equal(bits(got[k][:500]), bits(want[k])))
                  for k in ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "frame_clearance", "sphere_clearance")}
        for k in ("cost", "frame_cost", "frame_grad"):
            n = want[k + "_n"]
            lim = ((n[:, :, None] if k == "frame_grad" else n) + 16.0) * 2.0 ** -52 * want[k + "_abs"]
            checks[k + "_within_bound"] = bool(np.all(np.abs(got[k][:500] - want[k]) <= lim))
        checks["per_frame_route_min_clearance"] = bool(np.array_equal(got["min_clearance"], tr["min_clearance"]))
        checks["per_frame_route_n_below"] = bool(np.array_equal(got["n_below"], tr["n_below"]))
        checks["per_frame_route_cost_close"] = bool(np.allclose(got["cost"], tr["cost"], rtol=1e-12, atol=1e-12))
        ok = ok and all(checks.values())
        rows.append({"n_spheres": K, "n_frames": F, "steps": steps, "articulated_ms": t_a * 1e3, "per_frame_route_ms": t_b * 1e3,
                     "rigid_same_k_ms": t_c * 1e3, "configs_per_s": N / t_a, "spheres_per_s": N * K / t_a,
                     "speedup_vs_per_frame_route": t_b / t_a, "ratio_to_rigid_same_k": t_a / t_c,
                     "configs_below_margin": int((got["n_below"] > 0).sum()), "equal": checks})
        del outs, per_frame, rigid_out, state, tr, poses
        torch.cuda.empty_cache()
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    out = {"metric": "articulated_query_speedup_vs_per_frame_route_min_over_bodies", "value": min(r["speedup_vs_per_frame_route"] for r in rows),
           "unit": "x", "revision": rev, "source_sha256": source_digest(),
           "batch": f"{N} configurations based on the waypoints of bench.py's planner batch, frames within 0.5 m of the base with random "
                    f"quaternions, margin {margin:g}, spheres inside a ball 0.5 m wide about their frame, map {G}^3 @ {res} m with "
                    f"{args.obstacles} obstacles",
           "warmup": args.warmup, "by_body": rows, "all_equal": ok}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, "articulated_query.json"), "w").write(line + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
