#!/usr/bin/env python3
"""Body queries against the route that exists without them, on the map and planner batch of tools/path_query_bench.py.

Config 2's map (512^3 @ 0.1 m, 50 000 scattered obstacles, fully observed).  100 000 poses: positions drawn (seeded) from that
batch's waypoints, seeded random quaternions of norm 0.5 .. 2.  Bodies of K = 1, 8, 64, 512 spheres inside a ball 1 m wide.  Per K,
over IDENTICAL poses:
  body    fiesta_hip_body_query_dev, all eight outputs
  torch   the rotation and the N x K sphere centres built in torch, GetDistWithGradTrilinearDevice over all of them, then the
          penalty, the cross products and the per-pose reductions in torch
  points  GetDistWithGradTrilinearDevice ALONE on the same pre-built N x K points: the price of the samples themselves
p50 of each (device synchronise around every call, warm-up first; fewer repetitions for the large K, whose calls are long), the
first 500 poses checked against fiesta_amd.body_query_model (exact outputs by bits, cost and grad within the header's bound), one
JSON line, also written to DIR/body_query.json.  `source_sha256` identifies the measured sources independently of git.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/body_query_bench.py` (a run of its own).
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


def torch_route(m, sph_t, poses, margin, state=None):
    """the four steps a caller takes today, in torch around the device point query; returns the per-pose outputs"""
    import torch
    p, q = poses[:, :3], poses[:, 3:]
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    k = 2.0 / (((qw * qw + qx * qx) + qy * qy) + qz * qz)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
    R = torch.stack([1.0 - k * (yy + zz), k * (xy - wz), k * (xz + wy), k * (xy + wz), 1.0 - k * (xx + zz), k * (yz - wx),
                     k * (xz - wy), k * (yz + wx), 1.0 - k * (xx + yy)], 1).reshape(-1, 3, 3)
    c, r = sph_t[:, :3], sph_t[:, 3]
    a = (R[:, None, :, 0] * c[None, :, 0, None] + R[:, None, :, 1] * c[None, :, 1, None]) + R[:, None, :, 2] * c[None, :, 2, None]   # (N, K, 3)
    x = (p[:, None, :] + a).reshape(-1, 3).contiguous()
    n = len(x)
    dist = torch.empty(n, dtype=torch.float64, device=x.device)
    grad = torch.empty((n, 3), dtype=torch.float64, device=x.device)
    torch.cuda.synchronize()   # torch's centres -> the map's stream -> torch's reductions: the streams do not wait for each other
    m.GetDistWithGradTrilinearDevice(x.data_ptr(), n, dist.data_ptr(), grad.data_ptr())
    torch.cuda.synchronize()
    N, K = len(poses), len(sph_t)
    s = dist.reshape(N, K) - r[None]
    below = s < margin
    e = torch.where(below, margin - s, torch.zeros_like(s))
    gam = torch.where(below[:, :, None], (-2.0 * e)[:, :, None] * grad.reshape(N, K, 3), torch.zeros((), dtype=torch.float64, device=x.device))
    t = torch.cross(a, gam, dim=2)
    mins, arg = s.min(1)
    out = {"min_clearance": mins, "min_sphere": arg, "n_below": below.sum(1), "cost": (e * e).sum(1), "grad": torch.cat([gam.sum(1), t.sum(1)], 1),
           "sphere_clearance": s}
    if state is not None:
        state["x"] = x
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--poses", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="directory for body_query.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from bench import P_DEFAULT, Workload
    from fiesta_amd.esdf_map import BODY_FIELDS
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
    rng = np.random.RandomState(2024)
    N, margin = args.poses, args.margin
    pick = torch.from_numpy(rng.choice(len(w), N, replace=False)).to(dev)
    quat = rng.randn(N, 4)
    quat *= (2.0 ** rng.uniform(-1, 1, N) / np.linalg.norm(quat, axis=1))[:, None]
    poses = torch.cat([w[pick], torch.from_numpy(quat).to(dev)], 1).contiguous()
    poses_np = poses.cpu().numpy()

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

    rows, ok = [], True
    for K in (1, 8, 64, 512):
        c = rng.randn(K, 3)
        c *= (0.5 * rng.rand(K) ** (1 / 3) / np.linalg.norm(c, axis=1))[:, None]
        sph = np.ascontiguousarray(np.concatenate([c, rng.rand(K, 1) * 0.15], 1))
        sph_t = torch.from_numpy(sph).to(dev)
        outs = {name: torch.empty((N,) + tuple(K if d == "K" else d for d in shape), dtype=torch.float64 if dt == np.float64 else torch.int32,
                                  device=dev) for name, dt, shape in BODY_FIELDS}
        ptrs = {k: v.data_ptr() for k, v in outs.items()}
        torch.cuda.synchronize()
        steps = args.steps if K <= 64 else max(5, args.steps // 4)
        state = {}
        t_body = timed(lambda: m.BodyQueryDevice(sph, poses.data_ptr(), N, margin, ptrs), steps)
        t_torch = timed(lambda: state.update(out=torch_route(m, sph_t, poses, margin, state)), steps)
        x = state["x"]
        dist = torch.empty(len(x), dtype=torch.float64, device=dev)
        grad = torch.empty((len(x), 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t_points = timed(lambda: m.GetDistWithGradTrilinearDevice(x.data_ptr(), len(x), dist.data_ptr(), grad.data_ptr()), steps)
        # the call against the model on the first 500 poses, and against the torch route on all of them
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        want = fiesta_amd.body_query_model(m.GetDistWithGradTrilinear, sph, poses_np[:500], margin)
        tr = {k: v.cpu().numpy() for k, v in state["out"].items()}
        bits = lambda a: np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a   # noqa: E731
        checks = {k: bool(np.array_equal(bits(got[k][:500]), bits(want[k]))) for k in ("min_clearance", "min_sphere", "min_pos", "min_grad", "n_below", "sphere_clearance")}
        for k in ("cost", "grad"):
            lim = (K + 16.0) * 2.0 ** -52 * want[k + "_abs"]
            checks[k + "_within_bound"] = bool(np.all(np.abs(got[k][:500] - want[k]) <= lim))
        checks["torch_route_min_clearance"] = bool(np.array_equal(got["min_clearance"], tr["min_clearance"]))
        checks["torch_route_n_below"] = bool(np.array_equal(got["n_below"], tr["n_below"]))
        checks["torch_route_cost_close"] = bool(np.allclose(got["cost"], tr["cost"], rtol=1e-12, atol=1e-12))
        ok = ok and all(checks.values())
        rows.append({"n_spheres": K, "steps": steps, "body_ms": t_body * 1e3, "torch_route_ms": t_torch * 1e3, "point_query_only_ms": t_points * 1e3,
                     "poses_per_s": N / t_body, "spheres_per_s": N * K / t_body, "speedup_vs_torch_route": t_torch / t_body,
                     "ratio_to_point_query_only": t_body / t_points, "poses_below_margin": int((got["n_below"] > 0).sum()), "equal": checks})
        del outs, state, x, dist, grad, tr
        torch.cuda.empty_cache()
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    out = {"metric": "body_query_speedup_vs_torch_route_min_over_K", "value": min(r["speedup_vs_torch_route"] for r in rows), "unit": "x",
           "revision": rev, "source_sha256": source_digest(),
           "batch": f"{N} poses on the waypoints of bench.py's planner batch, random quaternions, margin {margin:g}, bodies inside a ball 1 m wide, "
                    f"map {G}^3 @ {res} m with {args.obstacles} obstacles",
           "warmup": args.warmup, "by_n_spheres": rows, "all_equal": ok}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, "body_query.json"), "w").write(line + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
