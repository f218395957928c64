#!/usr/bin/env python3
"""Body sweeps against the route that exists without them, on the map and planner batch of tools/body_query_bench.py.

Config 2's map (512^3 @ 0.1 m, 50 000 scattered obstacles, fully observed).  8192 polylines of 9 poses: the first nine waypoints of
that batch's polylines, seeded random quaternions of norm 0.5 .. 2, each within 90 degrees of its predecessor.  Bodies of K = 1, 8,
64, 512 spheres inside a ball 1 m wide, step 0.1 m.  Per K, over IDENTICAL waypoint poses:
  sweep   fiesta_hip_body_sweep_dev, all eleven outputs
  torch   the route of the parent commit: the sample poses built in torch on the device from the header's rule (one elementwise
          kernel per operation), fiesta_hip_body_query_dev on them, then torch segmented reductions per path
  body    fiesta_hip_body_query_dev ALONE on the same pre-built sample poses: the price of the samples themselves
p50 of each (device synchronise around every call, warm-up first; fewer repetitions for the large K, whose calls are long), the
first 500 paths checked against fiesta_amd.body_sweep_model by bits, the minimum and the first contact of ALL paths against the
torch route, one JSON line, also written to DIR/body_sweep.json.  `source_sha256` identifies the measured sources independently
of git.  Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/body_sweep_bench.py` (a run of its own).
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


def torch_sample_poses(poses, n_wp, step, reach):
    """the header's sample rule in torch for paths of n_wp poses each: (sample poses (M, 7), each sample's path, samples per path)"""
    import torch
    T = len(poses) // n_wp
    P = poses.reshape(T, n_wp, 7)
    q = P[:, :, 3:]
    s = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    u = q / torch.sqrt(s)[..., None]
    a, u0, u1 = P[:, :-1, :3], u[:, :-1], u[:, 1:]
    d = P[:, 1:, :3] - a
    L = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    dot = ((u0[..., 0] * u1[..., 0] + u0[..., 1] * u1[..., 1]) + u0[..., 2] * u1[..., 2]) + u0[..., 3] * u1[..., 3]
    v = torch.where((dot >= 0)[..., None], u1, -u1)
    e = v - u0
    ch = torch.sqrt(((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) + e[..., 3] * e[..., 3])
    S = torch.clamp(torch.ceil((L + (2.25 * reach) * ch) / step), min=1).to(torch.int64)             # (T, n_wp - 1)
    S1 = torch.cat([S, torch.ones((T, 1), dtype=torch.int64, device=S.device)], 1).reshape(-1)       # the final sample of every path
    seg = torch.repeat_interleave(torch.arange(len(S1), device=S.device), S1)                         # (reads the total back)
    k = torch.arange(len(seg), device=S.device) - (torch.cumsum(S1, 0) - S1)[seg]
    t = k.to(torch.float64) / S1[seg].to(torch.float64)
    r = 1.0 - t
    pad = lambda x: torch.cat([x, torch.zeros_like(x[:, :1])], 1).reshape(len(S1), -1)   # noqa: E731  (no segment starts at the last pose)
    pos = P[..., :3].reshape(-1, 3)[seg] + pad(d)[seg] * t[:, None]
    rot = r[:, None] * u.reshape(-1, 4)[seg] + t[:, None] * pad(v)[seg]                  # (t = 0 at the final sample: its own u, exactly)
    path = seg // n_wp
    return torch.cat([pos, rot], 1).contiguous(), path, S1.reshape(T, n_wp).sum(1)


def torch_route(m, sph, poses, n_wp, step, margin, reach, outs, state=None):
    """the four steps a caller takes today; returns the per-path minimum, its sample, the first contact and the contact count"""
    import torch
    samples, path, n = torch_sample_poses(poses, n_wp, step, reach)
    M, T = len(samples), len(n)
    mc, nb = outs["min_clearance"][:M], outs["n_below"][:M]
    torch.cuda.synchronize()   # torch's poses -> the map's stream -> torch's reductions: the streams do not wait for each other
    m.BodyQueryDevice(sph, samples.data_ptr(), M, margin, {"min_clearance": mc.data_ptr(), "min_sphere": outs["min_sphere"].data_ptr(),
                                                           "n_below": nb.data_ptr()})
    m.synchronize()
    first = torch.cumsum(n, 0) - n
    idx = torch.arange(M, device=samples.device) - first[path]
    big = torch.iinfo(torch.int64).max
    mins = torch.full((T,), float("inf"), dtype=torch.float64, device=samples.device).scatter_reduce(0, path, mc, "amin")
    arg = torch.full((T,), big, dtype=torch.int64, device=samples.device).scatter_reduce(
        0, path, torch.where(mc == mins[path], idx, torch.full_like(idx, big)), "amin")
    below = nb > 0
    fb = torch.full((T,), big, dtype=torch.int64, device=samples.device).scatter_reduce(0, path, torch.where(below, idx, torch.full_like(idx, big)), "amin")
    count = torch.zeros(T, dtype=torch.int64, device=samples.device).scatter_add(0, path, below.to(torch.int64))
    if state is not None:
        state["samples"] = samples
    return {"min_clearance": mins, "min_sample": arg, "first_below": torch.where(fb == big, torch.full_like(fb, -1), fb), "n_below": count,
            "n_samples": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--paths", type=int, default=8192)
    ap.add_argument("--poses", type=int, default=9, help="waypoint poses per polyline")
    ap.add_argument("--step", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin", type=float, default=0.3)
    ap.add_argument("--check", type=int, default=500, help="paths checked against the model")
    ap.add_argument("--out", default=None, help="directory for body_sweep.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from bench import P_DEFAULT, Workload
    from fiesta_amd.esdf_map import BODY_FIELDS, SWEEP_FIELDS
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
    w, w_off = planner_polylines(G, res, dev)
    T, W, step, margin = args.paths, args.poses, args.step, args.margin
    per = int(w_off[1] - w_off[0])
    pos = w.reshape(-1, per, 3)[:T, :W].cpu().numpy()
    rng = np.random.RandomState(2025)
    quat = np.empty((T, W, 4))
    q = rng.randn(T, 4)
    q /= np.linalg.norm(q, axis=1)[:, None]
    for j in range(W):                                       # each within 90 degrees of its predecessor: dq * q, dq about a random axis
        if j:
            ang = np.radians(rng.uniform(0, 90, T))
            axis = rng.randn(T, 3)
            axis /= np.linalg.norm(axis, axis=1)[:, None]
            dw, dv = np.cos(ang / 2), np.sin(ang / 2)[:, None] * axis
            q = np.concatenate([(dw * q[:, 0] - np.sum(dv * q[:, 1:], 1))[:, None], dw[:, None] * q[:, 1:] + q[:, :1] * dv + np.cross(dv, q[:, 1:])], 1)
        quat[:, j] = q * (2.0 ** rng.uniform(-1, 1, T))[:, None]
    poses_np = np.ascontiguousarray(np.concatenate([pos, quat], 2).reshape(-1, 7))
    off_np = np.arange(0, T * W + 1, W, dtype=np.int64)
    poses, off = torch.from_numpy(poses_np).to(dev), torch.from_numpy(off_np).to(dev)
    kinds = {np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32}

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

    bits = lambda a: np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a   # noqa: E731
    rows, ok = [], True
    for K in (1, 8, 64, 512):
        c = rng.randn(K, 3)
        c *= (0.5 * rng.rand(K) ** (1 / 3) / np.linalg.norm(c, axis=1))[:, None]
        sph = np.ascontiguousarray(np.concatenate([c, rng.rand(K, 1) * 0.15], 1))
        reach = fiesta_amd.body_reach(sph)
        outs = {name: torch.empty((T,) + shape, dtype=kinds[dt], device=dev) for name, dt, shape in SWEEP_FIELDS}
        ptrs = {k: v.data_ptr() for k, v in outs.items()}
        M = int(torch_sample_poses(poses, W, step, reach)[2].sum())
        body_outs = {name: torch.empty((M,) + tuple(K if d == "K" else d for d in shape), dtype=kinds[dt], device=dev)
                     for name, dt, shape in BODY_FIELDS if name in ("min_clearance", "min_sphere", "n_below")}
        torch.cuda.synchronize()
        steps = args.steps if K <= 64 else max(5, args.steps // 4)
        state = {}
        t_sweep = timed(lambda: (m.BodySweepDevice(sph, poses.data_ptr(), T * W, off.data_ptr(), T, step, margin, ptrs), m.synchronize()), steps)
        t_torch = timed(lambda: state.update(out=torch_route(m, sph, poses, W, step, margin, reach, body_outs, state)), steps)
        samples = state["samples"]
        body_ptrs = {k: v.data_ptr() for k, v in body_outs.items()}
        t_body = timed(lambda: (m.BodyQueryDevice(sph, samples.data_ptr(), M, margin, body_ptrs), m.synchronize()), steps)
        # the call against the model on the first paths (in chunks: the model holds every sphere of every sample), and against the
        # torch route on all of them
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        n_chk = min(args.check, T)
        checks = {name: True for name, _, _ in SWEEP_FIELDS}
        for lo in range(0, n_chk, 25):
            hi = min(lo + 25, n_chk)
            want = fiesta_amd.body_sweep_model(m.GetDistWithGradTrilinear, sph, poses_np[lo * W:hi * W], off_np[lo:hi + 1] - lo * W, step, margin)
            for name in checks:
                checks[name] = checks[name] and bool(np.array_equal(bits(got[name][lo:hi]), bits(want[name])))
        tr = {k: v.cpu().numpy() for k, v in state["out"].items()}
        for name in ("min_clearance", "min_sample", "first_below", "n_below", "n_samples"):
            checks["torch_route_" + name] = bool(np.array_equal(bits(got[name]), bits(tr[name])))
        ok = ok and all(checks.values())
        rows.append({"n_spheres": K, "steps": steps, "samples": M, "sweep_ms": t_sweep * 1e3, "torch_route_ms": t_torch * 1e3,
                     "body_query_only_ms": t_body * 1e3, "paths_per_s": T / t_sweep, "samples_per_s": M / t_sweep, "spheres_per_s": M * K / t_sweep,
                     "speedup_vs_torch_route": t_torch / t_sweep, "ratio_to_body_query_only": t_sweep / t_body,
                     "paths_in_contact": int((got["first_below"] >= 0).sum()), "equal": checks})
        del outs, body_outs, state, samples, tr
        torch.cuda.empty_cache()
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    out = {"metric": "body_sweep_speedup_vs_torch_route_min_over_K", "value": min(r["speedup_vs_torch_route"] for r in rows), "unit": "x",
           "revision": rev, "source_sha256": source_digest(),
           "batch": f"{T} polylines of {W} poses on the first waypoints of bench.py's planner batch, random quaternions within 90 degrees of their "
                    f"predecessor, step {step:g}, margin {margin:g}, bodies inside a ball 1 m wide, map {G}^3 @ {res} m with {args.obstacles} obstacles",
           "warmup": args.warmup, "by_n_spheres": rows, "all_equal": ok}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, "body_sweep.json"), "w").write(line + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
