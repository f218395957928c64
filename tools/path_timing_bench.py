#!/usr/bin/env python3
"""Path timing (fiesta_hip_path_timing_dev) on path_refine_bench's workload, against the route a user had before the call existed.

Scene (built here, nothing is read from disk): tools/reach_bench.py's partially observed 512^3 @ 0.1 m map with 50 000 scattered
obstacles; the flood runs in the box of 128^3 voxels around the seed, connectivity 26; the targets are the frontier voxels of that
box.  Two batches, both timed at step = one voxel: fiesta_hip_reach_paths' RAW paths to them (one waypoint per move) and the same
paths pulled tight (SHORTCUT, max_span 4096).
Measured per batch, p50 over --steps rounds after --warmup; within a round the calls ALTERNATE, each timed from a synchronised
device to the next synchronisation:
  timing_ms     fiesta_hip_path_timing_dev, every array resident on the device (two memsets, the offset check, both kernels)
  torch_ms      the route of today with everything on the device: the samples built by torch from the waypoints
                (repeat_interleave over S), ONE fiesta_hip_get_dist_grad_dev call on all of them, the limits element-wise, the two
                prefix minima by torch.cummin over padded [n_paths, max_samples] tensors (forward, and flipped for the backward one),
                the intervals element-wise, index_add_ for the durations (the two streams do not wait for each other: a
                synchronisation on either side of the query, as any caller of the two libraries needs)
  clearance_ms  fiesta_hip_path_clearance_dev on the same batch: what the samples alone cost
Checked: on --sample paths every output of the device batch equals fiesta_amd.path_timing_model over the host point query (duration
and time within the header's summation bound); the torch route's durations are compared with the fused call's and the largest
relative difference is reported (its arc lengths come from one global cumsum, so it is close, not bit-equal).
One JSON line; with --out DIR it is also written to DIR/path_timing_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/path_timing_bench.py` (a run of its own).
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

PAR = dict(step=0.1, margin=0.3, v_max=2.0, v_min=0.1, a_max=2.0, corner_dev=0.05, v_start=0.0, v_end=0.0)


def torch_route(m, w, off, par):
    """the header's rule on every path of a valid batch at once, in torch; returns duration, min_speed per path, time, speed per
    waypoint and the number of samples"""
    import torch
    dev, f64 = w.device, torch.float64
    n, N = len(off) - 1, len(w)
    A, Vq, Mq = 2.0 * par["a_max"], par["v_max"] ** 2, par["v_min"] ** 2
    lens = off[1:] - off[:-1]
    path_of = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    ar = torch.arange(N, device=dev)
    last = ar == off[1:][path_of] - 1
    d = torch.zeros_like(w)
    d[:-1] = w[1:] - w[:-1]
    d = torch.where(last[:, None], torch.zeros_like(d), d)
    L = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    S = torch.where(last, torch.ones_like(ar), torch.clamp(torch.ceil(L / par["step"]), min=1.0).to(torch.int64))
    idx = torch.repeat_interleave(ar, S)                                  # the waypoint every sample starts from
    T = len(idx)
    first = torch.cumsum(S, 0) - S                                        # the sample of every waypoint
    k = torch.arange(T, device=dev) - first[idx]
    t = k.to(f64) / S[idx].to(f64)
    pos = (w[idx] + d[idx] * t[:, None]).contiguous()
    dist = torch.empty(T, dtype=f64, device=dev)
    torch.cuda.synchronize()
    m.GetDistWithGradTrilinearDevice(pos.data_ptr(), T, dist.data_ptr(), 0)
    m.synchronize()
    Wg = torch.cumsum(L, 0) - L
    W = Wg - Wg[off[:-1][path_of]]
    s = W[idx] + L[idx] * t
    lq = torch.clamp(A * (dist - par["margin"]), min=Mq, max=Vq)
    lq = torch.where(dist < par["margin"], torch.full_like(lq, Mq), lq)
    if np.isfinite(par["corner_dev"]):
        inner = ~last & (ar != off[:-1][path_of])
        Lp, dp = torch.roll(L, 1), torch.roll(d, 1, 0)
        ok = inner & (Lp > 0) & (L > 0)
        u, v = dp / Lp[:, None], d / L[:, None]
        c = torch.clamp((u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2], min=-1.0, max=1.0)
        sh = torch.sqrt(0.5 * (1.0 + c))
        den = 1.0 - sh
        cq = torch.where(ok & (den > 0), ((par["a_max"] * par["corner_dev"]) * sh) / den, torch.full_like(sh, float("inf")))
        lq = torch.minimum(lq, torch.full_like(lq, float("inf")).scatter(0, first, cq))
    ps = path_of[idx]
    ns = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, path_of, S)
    sfirst = torch.cumsum(ns, 0) - ns
    j = torch.arange(T, device=dev) - sfirst[ps]
    lq = torch.where(j == 0, torch.clamp(lq, max=par["v_start"] ** 2), lq)
    lq = torch.where(j == ns[ps] - 1, torch.clamp(lq, max=par["v_end"] ** 2), lq)
    P = A * s
    width = int(ns.max().item()) if n else 0
    pad = torch.full((n, max(width, 1)), float("inf"), dtype=f64, device=dev)
    X = pad.clone()
    X[ps, j] = lq - P
    f = torch.cummin(X, 1).values[ps, j] + P
    Y = pad
    Y[ps, j] = lq + P
    b = torch.flip(torch.cummin(torch.flip(Y, [1]), 1).values, [1])[ps, j] - P
    vel = torch.sqrt(torch.minimum(lq, torch.minimum(f, b)))
    h = (L / S.to(f64))[idx]
    sv = vel + torch.roll(vel, -1)
    dt = torch.where(sv > 0, (2.0 * h) / sv, 2.0 * torch.sqrt(h / par["a_max"]))
    dt = torch.where((h == 0) | (j == ns[ps] - 1), torch.zeros_like(dt), dt)
    duration = torch.zeros(n, dtype=f64, device=dev).index_add_(0, ps, dt)
    ce = torch.cumsum(dt, 0) - dt
    time_wp = ce[first] - ce[sfirst[path_of]]
    min_speed = torch.full((n,), float("inf"), dtype=f64, device=dev).scatter_reduce_(0, ps, vel, "amin")
    torch.cuda.synchronize()
    return duration, min_speed, time_wp, vel[first], T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=200, help="paths compared with the model (0: all)")
    ap.add_argument("--out", default=None, help="directory for path_timing_partial<grid>.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from fiesta_amd.esdf_map import TIMING_FIELDS
    from corridor_bench import sub_csr
    from reach_bench import build_partial
    dev = torch.device("cuda", 0)
    G = args.grid
    m, _ = build_partial(G, int(round(args.obstacles * (G / 512.0) ** 3)))
    par = dict(PAR, step=0.1)

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
    tdt = {np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32}
    batches, checks = {}, {}
    for name, shortcut in (("raw", False), ("shortcut4096", True)):
        poff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=0, connectivity=26, shortcut=shortcut, max_span=4096)
        m.synchronize()
        n_wp = int(poff[n].item())
        wp = torch.zeros((max(n_wp, 1), 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=n_wp, connectivity=26, shortcut=shortcut, max_span=4096,
                           waypoints_pos_dev_ptr=wp.data_ptr())
        m.synchronize()
        w0 = wp[:n_wp].contiguous()
        outs = {k: torch.zeros(n if per == "path" else n_wp, dtype=tdt[dt], device=dev) for k, dt, per, _ in TIMING_FIELDS}
        ptrs = {k: v.data_ptr() for k, v in outs.items()}
        md = torch.zeros(n, dtype=torch.float64, device=dev)
        state = {}
        torch.cuda.synchronize()

        def timing():
            m.PathTimingDevice(w0.data_ptr(), n_wp, poff.data_ptr(), n, out=ptrs, **par)

        def route():
            state["r"] = torch_route(m, w0, poff, par)

        def clearance():
            m.PathClearanceDevice(w0.data_ptr(), n_wp, poff.data_ptr(), n, par["step"], par["margin"], out={"min_dist": md.data_ptr()})

        ts = {"timing_ms": [], "torch_ms": [], "clearance_ms": []}
        for it in range(args.warmup + args.steps):
            for key, fn in (("timing_ms", timing), ("torch_ms", route), ("clearance_ms", clearance)):
                t, _ = clock(fn)
                if it >= args.warmup:
                    ts[key].append(t * 1e3)
        r = {k: statistics.median(v) for k, v in ts.items()}
        r.update({k.replace("_ms", "_min_ms"): min(v) for k, v in ts.items()})
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        off_h, wp_h = poff.cpu().numpy(), w0.cpu().numpy()
        valid = got["status"] == 0
        tdur = state["r"][0].cpu().numpy()
        samples = int(got["n_samples"][valid].sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(tdur - got["duration"])[valid] / np.maximum(got["duration"][valid], 1e-300)
        r.update(torch_over_timing=r["torch_ms"] / r["timing_ms"], timing_over_clearance=r["timing_ms"] / r["clearance_ms"],
                 samples_per_s=samples / (r["timing_ms"] * 1e-3), waypoints=n_wp, samples=samples, torch_route_samples=int(state["r"][4]),
                 longest_path_samples=int(got["n_samples"].max()) if n else 0, paths_not_timed=int((~valid).sum()),
                 paths_above_wave_class=int((got["n_samples"] > 256).sum()), paths_below_margin=int((got["n_below"][valid] > 0).sum()),
                 duration_total_s=float(got["duration"][valid].sum()), length_total_m=float(got["length"][valid].sum()),
                 torch_route_max_rel_diff=float(rel[got["n_samples"][valid] > 1].max()) if (got["n_samples"][valid] > 1).any() else 0.0)
        batches[name] = r
        pick = np.arange(n) if args.sample <= 0 or args.sample >= n else np.sort(np.random.RandomState(1).choice(n, args.sample, replace=False))
        rows, soff = sub_csr(off_h, pick)
        want = fiesta_amd.path_timing_model(m.GetDistWithGradTrilinear, wp_h[rows], soff, **par)

        def same(a, b):
            if a.dtype != np.float64:
                return bool(np.array_equal(a, b))
            return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.int64)[~np.isnan(a)], b.view(np.int64)[~np.isnan(b)]))

        def close(a, b, cnt, mag):
            lim = (cnt + 16.0) * 2.0 ** -52 * mag
            return bool(np.array_equal(np.isnan(a), np.isnan(b)) and (np.where(np.isnan(b), 0.0, np.abs(a - b)) <= lim).all())

        checks[f"{name}_sample_equals_model"] = bool(
            all(same(got[k][pick], want[k]) for k in ("length", "n_samples", "n_below", "min_speed", "min_index", "status"))
            and same(got["speed"][rows], want["speed"]) and close(got["duration"][pick], want["duration"], want["duration_n"], want["duration_abs"])
            and close(got["time"][rows], want["time"], want["time_n"], want["time_abs"]))
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    res = {"metric": "path_timing_torch_route_over_device_call_raw_paths", "value": batches["raw"]["torch_over_timing"], "unit": "x",
           "scene": f"partial{G}", "grid": G, "revision": rev, "source_sha256": source_digest(), "seed": seed[0].tolist(),
           "box": [lo.tolist(), hi.tolist()], "params": par, "paths": n, "batches": batches, "sample": int(args.sample), "steps": args.steps,
           "warmup": args.warmup, "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"path_timing_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if res["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
