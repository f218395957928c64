#!/usr/bin/env python3
"""Batched path clearance against the point route, on bench.py's planner batch (`--workload queries`).

Config 2's map (512^3 @ 0.1 m, 50 000 scattered obstacles, fully observed).  bench.py's planner batch -- the same seeds: 8192
smooth trajectories of N // 8192 = 976 samples 0.4 voxels apart, reflected at the map's faces -- becomes 8192 polylines with a
waypoint every 8 samples (and the last one), asked with step = 0.4 * res.  Two routes over IDENTICAL samples:
  fused   fiesta_hip_path_clearance_dev: min, argmin + gradient, first sample below the margin, per path
  points  the samples generated in torch by the header's rule, GetDistWithGradTrilinearDevice over all of them, then the min,
          argmin and first-below reduced in torch
p50 of each (device synchronise around every call, warm-up first), both results checked equal, one JSON line.  Beside it the
point query kernel ALONE over the same pre-generated samples (no generation, no reduction): the floor of any point route, so the
fused call's ratio to it says what the fusion itself gains (most of the full point route's time is torch's own generation and
scatter reductions).  `source_sha256` identifies the measured sources (fiesta_amd/csrc, include) independently of git.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/path_query_bench.py` (a run of its own).
"""
import argparse
import glob
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def planner_polylines(G, res, dev, T=8192, N=8_000_000):
    """bench.py run_queries' planner batch (same generator, same seeds), every 8th sample kept as a waypoint"""
    import torch
    L = N // T
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    torch.rand((N, 3), generator=gen, device=dev, dtype=torch.float64)   # (the random batch bench.py draws first)
    gen.manual_seed(11)
    start = torch.rand((T, 1, 3), generator=gen, device=dev, dtype=torch.float64) * (G * res - 4.0) + 2.0
    head = torch.randn((T, 1, 3), generator=gen, device=dev, dtype=torch.float64)
    turn = torch.randn((T, L, 3), generator=gen, device=dev, dtype=torch.float64) * 0.05
    dirs = head + torch.cumsum(turn, 1)
    dirs = dirs / dirs.norm(dim=2, keepdim=True)
    path = start + torch.cumsum(dirs * (0.4 * res), 1)
    lo_b, span = 0.3, G * res - 0.6
    path = lo_b + span - (torch.remainder(path - lo_b, 2 * span) - span).abs()
    keep = sorted(set(range(0, L, 8)) | {L - 1})
    w = path[:, keep, :].reshape(-1, 3).contiguous()
    off = torch.arange(0, T * len(keep) + 1, len(keep), device=dev, dtype=torch.int64)
    torch.cuda.synchronize()   # (the map works on a stream of its own that does not wait for torch's)
    return w, off


def torch_samples(w, off, step):
    """the header's sample rule in torch (one elementwise kernel per operation: nothing is contracted); returns the samples and
    each sample's path"""
    import torch
    T = len(off) - 1
    K = int(off[1] - off[0])           # (every path has the same number of waypoints here)
    W = w.reshape(T, K, 3)
    d = W[:, 1:] - W[:, :-1]
    L = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    S = torch.clamp(torch.ceil(L / step), min=1).to(torch.int64)          # (T, K - 1)
    S_ext = torch.cat([S, torch.ones((T, 1), dtype=torch.int64, device=w.device)], 1).reshape(-1)
    idx = torch.repeat_interleave(torch.arange(T * K, device=w.device), S_ext)
    first = torch.cumsum(S_ext, 0) - S_ext
    k = torch.arange(len(idx), device=w.device) - first[idx]
    dd = torch.cat([d, torch.zeros((T, 1, 3), dtype=w.dtype, device=w.device)], 1).reshape(-1, 3)
    t = k.to(torch.float64) / S_ext[idx].to(torch.float64)
    pos = w[idx] + dd[idx] * t[:, None]
    is_last = (idx % K) == K - 1
    pos = torch.where(is_last[:, None], w[idx], pos)
    return pos.contiguous(), torch.div(idx, K, rounding_mode="floor")


def source_digest():
    """sha256 over the native sources (path and bytes of fiesta_amd/csrc/* and include/**), in sorted path order"""
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "fiesta_amd", "csrc", "*.h*")) + glob.glob(os.path.join(ROOT, "include", "**", "*.h"),
                                                                                      recursive=True))
    for f in files:
        h.update(os.path.relpath(f, ROOT).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()


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
    from fiesta_amd.esdf_map import PATH_FIELDS
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
    outs = {name: torch.empty((T,) + shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=dev)
            for name, dt, shape in PATH_FIELDS}
    ptrs = {k: v.data_ptr() for k, v in outs.items()}

    def fused():
        m.PathClearanceDevice(w.data_ptr(), len(w), off.data_ptr(), T, step, margin, ptrs)

    state = {}

    def points():
        pos, seg = torch_samples(w, off, step)
        n = len(pos)
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        grad = torch.empty((n, 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()   # torch's samples -> the map's stream -> torch's reductions: the streams do not wait for each other
        m.GetDistWithGradTrilinearDevice(pos.data_ptr(), n, dist.data_ptr(), grad.data_ptr())
        torch.cuda.synchronize()
        mins = torch.full((T,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, seg, dist, "amin")
        ar = torch.arange(n, device=dev)
        big = torch.full((T,), n, dtype=torch.int64, device=dev)
        arg = big.scatter_reduce(0, seg, torch.where(dist == mins[seg], ar, n), "amin")
        fb = big.scatter_reduce(0, seg, torch.where(dist < margin, ar, n), "amin")
        state.update(pos=pos, seg=seg, dist=dist, grad=grad, mins=mins, arg=arg, fb=fb)

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

    t_fused = timed(fused)
    t_points = timed(points)
    pos_pre = state["pos"]
    dist_k = torch.empty(len(pos_pre), dtype=torch.float64, device=dev)
    grad_k = torch.empty((len(pos_pre), 3), dtype=torch.float64, device=dev)
    t_kernel = timed(lambda: m.GetDistWithGradTrilinearDevice(pos_pre.data_ptr(), len(pos_pre), dist_k.data_ptr(), grad_k.data_ptr()))
    # the two routes agree, and the torch samples are the header's rule (numpy) bit for bit
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    pos_np, ns = fiesta_amd.path_samples(w.cpu().numpy(), off.cpu().numpy(), step)
    s = state
    first = torch.cumsum(torch.bincount(s["seg"], minlength=T), 0).cpu().numpy() - ns
    arg, fb = s["arg"].cpu().numpy(), s["fb"].cpu().numpy()
    checks = {
        "torch_samples_equal_rule": bool(np.array_equal(s["pos"].cpu().numpy().view(np.int64), pos_np.view(np.int64))),
        "n_samples": bool(np.array_equal(got["n_samples"], ns)),
        "min_dist": bool(np.array_equal(got["min_dist"], s["mins"].cpu().numpy())),
        "min_index": bool(np.array_equal(got["min_index"], arg - first)),
        "min_grad": bool(np.array_equal(got["min_grad"].view(np.int64), s["grad"].cpu().numpy()[arg].view(np.int64))),
        "first_below": bool(np.array_equal(got["first_below"], np.where(fb < len(pos_np), fb - first, -1))),
    }
    n_samp = int(ns.sum())
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    io_bytes = len(w) * 24 + (T + 1) * 8 + T * (8 + 8 + 24 + 24 + 8 + 24 + 8)
    out = {"metric": "path_clearance_speedup_vs_point_route", "value": t_points / t_fused, "unit": "x", "target": 3.0,
           "met": bool(t_points / t_fused >= 3.0), "revision": rev, "source_sha256": source_digest(),
           "batch": f"bench.py --workload queries planner batch: {T} paths, {len(w) // T} waypoints each (every 8th sample), "
                    f"step {step:g} m, {n_samp} samples, margin {margin:g}, map {G}^3 @ {res} m with {args.obstacles} obstacles",
           "fused_ms": t_fused * 1e3, "point_route_ms": t_points * 1e3, "fused_samples_per_s": n_samp / t_fused,
           "point_route_samples_per_s": n_samp / t_points,
           "point_query_kernel_only_ms": t_kernel * 1e3, "speedup_vs_point_query_kernel_only": t_kernel / t_fused,
           "ratio_note": "the point route's time is mostly torch's: sample generation (repeat_interleave synchronises with the host) "
                         "and three scatter_reduce passes; against the point query kernel alone on pre-generated samples -- the "
                         "floor of any point route, with no generation and no reduction -- see speedup_vs_point_query_kernel_only",
           "fused_io_bytes": io_bytes, "point_route_io_bytes_min": n_samp * (24 + 8 + 24),
           "io_note": "fused: waypoints + offsets in, the seven per-path outputs out; point route: at least the samples' positions "
                      "written and read back (24 B) and value + gradient (32 B) per sample, before the reductions",
           "steps": args.steps, "warmup": args.warmup, "equal": checks, "all_equal": all(checks.values())}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    m.close()
    return 0 if out["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
