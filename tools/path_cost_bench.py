#!/usr/bin/env python3
"""Batched path cost + waypoint gradients against the point route, on bench.py's planner batch (`--workload queries`).

The map and the batch of tools/path_query_bench.py: config 2's map (512^3 @ 0.1 m, 50 000 scattered obstacles, fully observed), 8192
polylines of 123 waypoints, step = 0.4 * res, ~8.0 M samples.  Measured in one run, p50 with warm-up, device synchronise around
every call:
  (a) cost       fiesta_hip_path_cost_dev: cost, length, n_below, n_samples per path, the gradient of every waypoint
  (b) clearance  fiesta_hip_path_clearance_dev on the same batch (reads the same eight corners per sample, no gradient)
  (c) kernel     the point query kernel alone WITH gradients over the pre-generated samples: no generation, no reduction -- the
                 floor of any point route; (a) reads what (c) reads and writes almost nothing, so (a) / (c) should stay <= 1.25
  (d) points     the full point route in torch: the samples by the header's rule, GetDistWithGradTrilinearDevice over all of them,
                 penalty, chain rule, index_add_ into the segments' sums, the per-segment formulas, per-path sums; target (d) / (a) >= 3
(a) is checked against fiesta_amd.path_cost_model (numpy over the host point query) and (d) against (a), both within the
header's summation bound (n + 16) * 2^-52 * A.  One JSON line; `source_sha256` identifies the measured sources.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/path_cost_bench.py` (a run of its own).
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


def torch_point_route(m, w, off, step, margin):
    """what an optimiser does today, on the device: returns cost (T), grad (T * K, 3), and the pre-generated samples"""
    import torch
    dev = w.device
    T = len(off) - 1
    K = len(w) // T                     # (every path has the same number of waypoints here)
    W = w.reshape(T, K, 3)
    d = W[:, 1:] - W[:, :-1]
    L = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    S = torch.clamp(torch.ceil(L / step), min=1).to(torch.int64)          # (T, K - 1)
    S_ext = torch.cat([S, torch.ones((T, 1), dtype=torch.int64, device=dev)], 1).reshape(-1)
    idx = torch.repeat_interleave(torch.arange(T * K, device=dev), S_ext)
    first = torch.cumsum(S_ext, 0) - S_ext
    k = torch.arange(len(idx), device=dev) - first[idx]
    dd = torch.cat([d, torch.zeros((T, 1, 3), dtype=w.dtype, device=dev)], 1).reshape(-1, 3)
    t = k.to(torch.float64) / S_ext[idx].to(torch.float64)
    pos = (w[idx] + dd[idx] * t[:, None]).contiguous()     # (the last waypoint: dd = 0, t = 0)
    n = len(pos)
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    grad = torch.empty((n, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()   # torch's samples -> the map's stream -> torch's reductions: the streams do not wait for each other
    m.GetDistWithGradTrilinearDevice(pos.data_ptr(), n, dist.data_ptr(), grad.data_ptr())
    torch.cuda.synchronize()
    below = dist < margin
    e = torch.where(below, margin - dist, torch.zeros_like(dist))
    phi = e * e
    gam = torch.where(below[:, None], (-2.0 * e)[:, None] * grad, torch.zeros_like(grad))
    inner = (k > 0).to(torch.float64)
    r = 1.0 - t
    P = torch.zeros(T * K, dtype=torch.float64, device=dev).index_add_(0, idx, phi * inner)
    A = torch.zeros((T * K, 3), dtype=torch.float64, device=dev).index_add_(0, idx, (r * inner)[:, None] * gam)
    B = torch.zeros((T * K, 3), dtype=torch.float64, device=dev).index_add_(0, idx, (t * inner)[:, None] * gam)
    phi_w, gam_w = phi[first].reshape(T, K), gam[first].reshape(T, K, 3)
    P, A, B = P.reshape(T, K)[:, :-1], A.reshape(T, K, 3)[:, :-1], B.reshape(T, K, 3)[:, :-1]
    Sd = S.to(torch.float64)
    h = L / Sd
    Q = (phi_w[:, :-1] * 0.5 + P) + phi_w[:, 1:] * 0.5
    qs = Q / Sd
    u = d / L[..., None]
    ok = (L > 0)[..., None]
    N = torch.where(ok, h[..., None] * (gam_w[:, :-1] * 0.5 + A) - qs[..., None] * u, torch.zeros_like(u))
    E = torch.where(ok, h[..., None] * (B + gam_w[:, 1:] * 0.5) + qs[..., None] * u, torch.zeros_like(u))
    cost = torch.where(L > 0, h * Q, torch.zeros_like(Q)).sum(1)
    g = torch.zeros((T, K, 3), dtype=torch.float64, device=dev)
    g[:, :-1] += N
    g[:, 1:] += E
    return cost, g.reshape(-1, 3), pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from bench import P_DEFAULT, Workload
    from fiesta_amd.esdf_map import PATH_COST_FIELDS, PATH_FIELDS
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
    w, off = planner_polylines(G, res, dev)
    T, step, margin = len(off) - 1, 0.4 * res, args.margin
    f64 = lambda dt: torch.float64 if dt == np.float64 else torch.int64   # noqa: E731
    couts = {name: torch.empty((T if per == "path" else len(w),) + shape, dtype=f64(dt), device=dev) for name, dt, per, shape in PATH_COST_FIELDS}
    pouts = {name: torch.empty((T,) + shape, dtype=f64(dt), device=dev) for name, dt, shape in PATH_FIELDS}
    cptrs, pptrs = {k: v.data_ptr() for k, v in couts.items()}, {k: v.data_ptr() for k, v in pouts.items()}
    state = {}

    def cost():
        m.PathCostDevice(w.data_ptr(), len(w), off.data_ptr(), T, step, margin, cptrs)

    def clearance():
        m.PathClearanceDevice(w.data_ptr(), len(w), off.data_ptr(), T, step, margin, pptrs)

    def points():
        state["cost"], state["grad"], state["pos"] = torch_point_route(m, w, off, step, margin)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    t_cost = timed(cost)
    t_clear = timed(clearance)
    t_points = timed(points)
    pos = state["pos"]
    dist_k = torch.empty(len(pos), dtype=torch.float64, device=dev)
    grad_k = torch.empty((len(pos), 3), dtype=torch.float64, device=dev)
    t_kernel = timed(lambda: m.GetDistWithGradTrilinearDevice(pos.data_ptr(), len(pos), dist_k.data_ptr(), grad_k.data_ptr()))
    # (a) against the numpy model over the host point query, (d) against (a): the header's summation bound
    got = {k: v.cpu().numpy() for k, v in couts.items()}
    model = fiesta_amd.path_cost_model(m.GetDistWithGradTrilinear, w.cpu().numpy(), off.cpu().numpy(), step, margin)
    lim = lambda n, a: (n + 16.0) * 2.0 ** -52 * a   # noqa: E731
    lim_cost, lim_grad = lim(model["cost_n"], model["cost_abs"]), lim(model["grad_n"][:, None], model["grad_abs"])
    pc, pg = state["cost"].cpu().numpy(), state["grad"].cpu().numpy()
    checks = {
        "n_samples": bool(np.array_equal(got["n_samples"], model["n_samples"])),
        "n_below": bool(np.array_equal(got["n_below"], model["n_below"])),
        "cost_vs_model": bool((np.abs(got["cost"] - model["cost"]) <= lim_cost).all()),
        "grad_vs_model": bool((np.abs(got["grad"] - model["grad"]) <= lim_grad).all()),
        "length_vs_model": bool((np.abs(got["length"] - model["length"]) <= lim(model["length_n"], model["length_abs"])).all()),
        "point_route_cost_vs_fused": bool((np.abs(pc - got["cost"]) <= lim_cost).all()),
        "point_route_grad_vs_fused": bool((np.abs(pg - got["grad"]) <= lim_grad).all()),
    }
    n_samp = int(model["n_samples"].sum())
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    out = {"metric": "path_cost_speedup_vs_point_route", "value": t_points / t_cost, "unit": "x", "target": 3.0,
           "met": bool(t_points / t_cost >= 3.0), "revision": rev, "source_sha256": source_digest(),
           "batch": f"bench.py --workload queries planner batch: {T} paths, {len(w) // T} waypoints each (every 8th sample), "
                    f"step {step:g} m, {n_samp} samples, margin {margin:g}, map {G}^3 @ {res} m with {args.obstacles} obstacles",
           "path_cost_ms": t_cost * 1e3, "path_clearance_ms": t_clear * 1e3, "point_query_kernel_with_grad_ms": t_kernel * 1e3,
           "point_route_ms": t_points * 1e3, "cost_over_point_query_kernel": t_cost / t_kernel, "cost_over_kernel_expected_max": 1.25,
           "cost_over_kernel_met": bool(t_cost / t_kernel <= 1.25), "cost_over_clearance": t_cost / t_clear,
           "cost_samples_per_s": n_samp / t_cost, "paths_with_cost": int(np.count_nonzero(model["cost"] > 0)),
           "samples_below_margin": int(model["n_below"].sum()),
           "cost_io_bytes": len(w) * 24 + (T + 1) * 8 + T * 32 + len(w) * 24, "point_route_io_bytes_min": n_samp * (24 + 8 + 24),
           "steps": args.steps, "warmup": args.warmup, "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    m.close()
    return 0 if out["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
