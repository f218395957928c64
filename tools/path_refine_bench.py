#!/usr/bin/env python3
"""Path refinement (fiesta_hip_path_refine_dev) on corridor_bench's workload, against the route a user had before the call existed.

Scene (built here, nothing is read from disk): tools/reach_bench.py's partially observed 512^3 @ 0.1 m map with 50 000 scattered
obstacles; the flood runs in the box of 128^3 voxels around the seed, connectivity 26; the targets are the frontier voxels of that
box, the paths are fiesta_hip_reach_paths' RAW paths to them (one waypoint per move), the corridors fiesta_hip_path_corridor's with
max_grow 16 in that box, the bounds fiesta_amd.corridor_bounds' (host numpy, once, not timed).
Measured at 8 and at 32 iterations, p50 over --steps rounds after --warmup; within a round the calls ALTERNATE, each timed from a
synchronised device to the next synchronisation:
  refine_ms   fiesta_hip_path_refine_dev, every array resident on the device, out of place (row copy, offset check, both kernels)
  torch_ms    the route of today with everything on the device: per iteration fiesta_hip_get_dist_grad_dev on ALL waypoints, then
              torch element-wise ops for the penalty, the five-point stencil, the step and the two clamps (the two streams do not
              wait for each other: a synchronisation on either side of the query, as any caller of the two libraries needs)
and once: corridor_ms, the fiesta_hip_path_corridor_dev call that feeds the refinement.
Checked: on --sample paths every output of the device batch equals fiesta_amd.path_refine_model over the host point query (cost
within the header's summation bound); the torch route's waypoints are compared with the fused call's and the largest difference is
reported (torch's element-wise kernels round every operation once, as the header does: it is expected to be 0).
One JSON line; with --out DIR it is also written to DIR/path_refine_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/path_refine_bench.py` (a run of its own).
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

PAR = dict(margin=0.5, w_obstacle=1.0, w_smooth=1.0, alpha=0.02, max_step=0.05, tolerance=0.0)
ITERATIONS = (8, 32)


def torch_route(m, w, inner, bounds, iterations):
    """`iterations` Jacobi steps of the header's rule on every waypoint at once; inner: the mask of the waypoints that move"""
    import torch
    n = len(w)
    dist = torch.empty(n, dtype=torch.float64, device=w.device)
    grad = torch.empty((n, 3), dtype=torch.float64, device=w.device)
    zero = torch.zeros((1, 3), dtype=torch.float64, device=w.device)
    lo, hi = bounds[:, :3], bounds[:, 3:]
    im = inner[:, None]

    def second(x):   # a_j, zero at the ends
        a = torch.cat([zero, (x[:-2] - 2.0 * x[1:-1]) + x[2:], zero])
        return torch.where(im, a, torch.zeros_like(a))

    for _ in range(iterations):
        w = w.contiguous()
        torch.cuda.synchronize()
        m.GetDistWithGradTrilinearDevice(w.data_ptr(), n, dist.data_ptr(), grad.data_ptr())
        m.synchronize()
        below = dist < PAR["margin"]
        e = torch.where(below, PAR["margin"] - dist, torch.zeros_like(dist))
        gam = torch.where(below[:, None], (-2.0 * e)[:, None] * grad, torch.zeros_like(grad))
        a = second(w)
        s = torch.cat([zero, (a[:-2] - 2.0 * a[1:-1]) + a[2:], zero])
        delta = PAR["alpha"] * (PAR["w_obstacle"] * gam + (2.0 * PAR["w_smooth"]) * s)
        delta = torch.where(delta > PAR["max_step"], torch.full_like(delta, PAR["max_step"]), delta)
        delta = torch.where(delta < -PAR["max_step"], torch.full_like(delta, -PAR["max_step"]), delta)
        x = w - delta
        x = torch.where(x < lo, lo, x)
        x = torch.where(x > hi, hi, x)
        w = torch.where(im, x, w)
    torch.cuda.synchronize()
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=200, help="paths compared with the model (0: all)")
    ap.add_argument("--out", default=None, help="directory for path_refine_partial<grid>.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from fiesta_amd.esdf_map import REFINE_FIELDS
    from corridor_bench import sub_csr
    from reach_bench import build_partial
    dev = torch.device("cuda", 0)
    G = args.grid
    m, _ = build_partial(G, int(round(args.obstacles * (G / 512.0) ** 3)))

    def clock(fn):
        torch.cuda.synchronize()
        m.synchronize()
        t0 = time.perf_counter()
        r = fn()
        m.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    f = m.download_field(("d2", "occ"))
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
    poff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=0, connectivity=26)
    m.synchronize()
    n_wp = int(poff[n].item())
    wv = torch.zeros((max(n_wp, 1), 3), dtype=torch.int32, device=dev)
    wp = torch.zeros((max(n_wp, 1), 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=n_wp, connectivity=26, waypoints_vox_dev_ptr=wv.data_ptr(),
                       waypoints_pos_dev_ptr=wp.data_ptr())
    m.synchronize()
    # the corridors: a sizing call, then the call that is timed once
    ckw = dict(lo=lo, hi=hi, max_grow=16)
    coff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    m.PathCorridorDevice(wv.data_ptr(), n_wp, poff.data_ptr(), n, coff.data_ptr(), capacity=0, **ckw)
    m.synchronize()
    total = int(coff[n].item())
    box = {"boxes": torch.zeros((max(total, 1), 6), dtype=torch.int32, device=dev), "boxes_pos": torch.zeros((max(total, 1), 6), dtype=torch.float64, device=dev),
           "entry": torch.zeros(max(total, 1), dtype=torch.int32, device=dev), "status": torch.zeros(n, dtype=torch.int32, device=dev)}
    t_corridor, _ = clock(lambda: m.PathCorridorDevice(wv.data_ptr(), n_wp, poff.data_ptr(), n, coff.data_ptr(), capacity=total,
                                                       boxes_dev_ptr=box["boxes"].data_ptr(), boxes_pos_dev_ptr=box["boxes_pos"].data_ptr(),
                                                       entry_dev_ptr=box["entry"].data_ptr(), status_dev_ptr=box["status"].data_ptr(), **ckw))
    wv_h, wp_h, off_h = wv.cpu().numpy()[:n_wp], wp.cpu().numpy()[:n_wp], poff.cpu().numpy()
    cor = {"offsets": coff.cpu().numpy(), "boxes": box["boxes"].cpu().numpy()[:total], "boxes_pos": box["boxes_pos"].cpu().numpy()[:total],
           "entry": box["entry"].cpu().numpy()[:total], "status": box["status"].cpu().numpy()}
    t0 = time.perf_counter()
    bounds_h, ok = fiesta_amd.corridor_bounds(wv_h, off_h, cor)
    t_bounds = time.perf_counter() - t0
    bt = torch.from_numpy(bounds_h).to(dev)
    w0 = wp[:n_wp].contiguous()
    lens = np.diff(off_h)
    k = np.arange(n_wp) - np.repeat(off_h[:-1], lens)
    inner_h = (k >= 1) & (k <= np.repeat(lens, lens) - 2)
    inner = torch.from_numpy(inner_h).to(dev)
    tdt = {np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32}
    outs = {name: torch.zeros((n if per == "path" else n_wp,) + shape, dtype=tdt[dt], device=dev) for name, dt, per, shape in REFINE_FIELDS}
    ptrs = {kk: v.data_ptr() for kk, v in outs.items()}
    torch.cuda.synchronize()
    results, checks, state = {}, {}, {}
    pick = np.arange(n) if args.sample <= 0 or args.sample >= n else np.sort(np.random.RandomState(1).choice(n, args.sample, replace=False))
    rows, soff = sub_csr(off_h, pick)
    for its in ITERATIONS:
        par = dict(PAR, iterations=its)

        def refine():
            m.PathRefineDevice(w0.data_ptr(), n_wp, poff.data_ptr(), n, bt.data_ptr(), out=ptrs, **par)

        def route():
            state["w"] = torch_route(m, w0, inner, bt, its)

        ts = {"refine_ms": [], "torch_ms": []}
        for it in range(args.warmup + args.steps):
            for key, fn in (("refine_ms", refine), ("torch_ms", route)):
                t, _ = clock(fn)
                if it >= args.warmup:
                    ts[key].append(t * 1e3)
        r = {kk: statistics.median(v) for kk, v in ts.items()}
        got = {kk: v.cpu().numpy() for kk, v in outs.items()}
        valid = got["status"] == 0
        r.update(torch_over_refine=r["torch_ms"] / r["refine_ms"], waypoint_iterations_per_s=float(inner_h.sum()) * its / (r["refine_ms"] * 1e-3),
                 paths_invalid=int((~valid).sum()), iterations_run=int(got["iterations"][valid].sum()),
                 paths_stopped_early=int((got["iterations"][valid & (lens > 2)] < its).sum()),
                 cost_before=float(got["cost"][valid, 0].sum()), cost_after=float(got["cost"][valid, 1].sum()),
                 n_below=int(got["n_below"][valid].sum()), largest_move_m=float(np.abs(got["waypoints"] - wp_h).max()),
                 torch_route_max_abs_diff=float(np.abs(state["w"].cpu().numpy() - got["waypoints"])[np.repeat(valid, lens)].max()))
        results[f"iterations{its}"] = r
        want = fiesta_amd.path_refine_model(m.GetDistWithGradTrilinear, wp_h[rows], soff, bounds_h[rows], **par)
        same = lambda a, b: bool(np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b))  # noqa: E731
        lim = (want["cost_n"] + 16.0) * 2.0 ** -52 * want["cost_abs"]
        gc, wc = got["cost"][pick], want["cost"]
        checks[f"iterations{its}_sample_equals_model"] = bool(
            same(got["waypoints"][rows], want["waypoints"]) and all(same(got[kk][pick], want[kk]) for kk in ("last_move", "iterations", "n_below", "min_dist", "status"))
            and np.array_equal(np.isnan(gc), np.isnan(wc)) and (np.where(np.isnan(wc), 0.0, np.abs(gc - wc)) <= lim).all())
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    head = results["iterations32"]
    res = {"metric": "path_refine_torch_route_over_device_call_32_iterations", "value": head["torch_over_refine"], "unit": "x",
           "scene": f"partial{G}", "grid": G, "revision": rev, "source_sha256": source_digest(), "seed": seed[0].tolist(),
           "box": [lo.tolist(), hi.tolist()], "params": PAR, "paths": n, "waypoints": n_wp, "interior_waypoints": int(inner_h.sum()),
           "longest_path": int(lens.max()) if n else 0, "paths_above_wave_class": int((lens > 128).sum()), "boxes": total,
           "corridors_whole": int(ok.sum()), "corridor_ms": t_corridor * 1e3, "corridor_bounds_host_ms": t_bounds * 1e3, "refine": results,
           "sample": int(len(pick)), "steps": args.steps, "warmup": args.warmup, "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"path_refine_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if res["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
