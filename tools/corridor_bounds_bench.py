#!/usr/bin/env python3
"""Corridor bounds (fiesta_hip_corridor_bounds[_dev]) on corridor_bench's and path_refine_bench's workload, against the host function
it replaces and next to the two calls it sits between.

Scene (built here, nothing is read from disk): tools/reach_bench.py's partially observed 512^3 @ 0.1 m map with 50 000 scattered
obstacles; the flood runs in the box of 128^3 voxels around the seed, connectivity 26; the targets are the frontier voxels of that
box, the paths are fiesta_hip_reach_paths' RAW paths to them (one waypoint per move), the corridors fiesta_hip_path_corridor's with
max_grow 16 in that box.
Measured, p50 over --steps rounds after --warmup; within a round the calls ALTERNATE, each timed from a synchronised device to the
next synchronisation:
  bounds_dev_ms          fiesta_hip_corridor_bounds_dev with VOID_BROKEN, every array resident on the device, all three outputs
  bounds_dev_no_box_ms   the same without the `box` output (what the refinement needs)
  bounds_host_ms         fiesta_hip_corridor_bounds on host arrays (stages, runs the same kernels, copies back)
  numpy_ms               fiesta_amd.corridor_bounds on arrays already on the host: the parent's route, as DESIGN.md 6l timed it
  numpy_with_copy_ms     the same plus the copy-back of the waypoints, offsets, boxes, entries and status it needs
  bounds_upload_ms       ... and the upload of its bounds, which the refinement on the device needs next
  corridor_ms            fiesta_hip_path_corridor_dev, the call before
  refine8_ms, refine32_ms  fiesta_hip_path_refine_dev inside those bounds, the call after
Checked on the WHOLE batch: `bounds` (as int64 views) and `ok` of the device call and of the host call equal
fiesta_amd.corridor_bounds with the same explicit inset; with VOID_BROKEN exactly the rows of the paths that are not ok are NaN; the
refined waypoints (32 iterations) of the chain that never leaves the device equal, on the ok paths, those of the chain whose bounds
come from the host function, and every other path comes back unmoved.
One JSON line; with --out DIR it is also written to DIR/corridor_bounds_partial<grid>.json.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/corridor_bounds_bench.py` (a run of its own).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512, help="a multiple of 32 (a rehearsal at a small size)")
    ap.add_argument("--obstacles", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="directory for corridor_bounds_partial<grid>.json")
    args = ap.parse_args()
    import torch
    import fiesta_amd
    from reach_bench import build_partial
    dev = torch.device("cuda", 0)
    G = args.grid
    m, _ = build_partial(G, int(round(args.obstacles * (G / 512.0) ** 3)))
    inset = m.resolution * 2.0 ** -20

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
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    td = torch.tensor(targets, dtype=torch.int32, device=dev)
    poff = z(n + 1, torch.int64)
    torch.cuda.synchronize()
    m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=0, connectivity=26)
    m.synchronize()
    n_wp = int(poff[n].item())
    wv, wp = z((max(n_wp, 1), 3), torch.int32), z((max(n_wp, 1), 3), torch.float64)
    torch.cuda.synchronize()
    m.ReachPathsDevice(td.data_ptr(), n, poff.data_ptr(), capacity=n_wp, connectivity=26, waypoints_vox_dev_ptr=wv.data_ptr(),
                       waypoints_pos_dev_ptr=wp.data_ptr())
    m.synchronize()
    ckw = dict(lo=lo, hi=hi, max_grow=16)
    coff = z(n + 1, torch.int64)
    torch.cuda.synchronize()
    m.PathCorridorDevice(wv.data_ptr(), n_wp, poff.data_ptr(), n, coff.data_ptr(), capacity=0, **ckw)
    m.synchronize()
    total = int(coff[n].item())
    box = {"boxes": z((max(total, 1), 6), torch.int32), "boxes_pos": z((max(total, 1), 6), torch.float64), "entry": z(max(total, 1), torch.int32),
           "status": z(n, torch.int32)}
    d_bounds, d_ok, d_box = z((max(n_wp, 1), 6), torch.float64), z(n, torch.int32), z(max(n_wp, 1), torch.int64)
    d_bounds_up = z((max(n_wp, 1), 6), torch.float64)
    d_out = z((max(n_wp, 1), 3), torch.float64)
    d_rstatus = z(n, torch.int32)
    torch.cuda.synchronize()
    state = {}

    def corridor():
        m.PathCorridorDevice(wv.data_ptr(), n_wp, poff.data_ptr(), n, coff.data_ptr(), capacity=total, boxes_dev_ptr=box["boxes"].data_ptr(),
                             boxes_pos_dev_ptr=box["boxes_pos"].data_ptr(), entry_dev_ptr=box["entry"].data_ptr(),
                             status_dev_ptr=box["status"].data_ptr(), **ckw)

    def bounds_dev(void_broken=True, with_box=True, out=None):
        m.CorridorBoundsDevice(wv.data_ptr(), n_wp, poff.data_ptr(), n, coff.data_ptr(), box["boxes"].data_ptr(), box["boxes_pos"].data_ptr(),
                               box["entry"].data_ptr(), box["status"].data_ptr(), total, inset=inset, void_broken=void_broken,
                               bounds_dev_ptr=(out if out is not None else d_bounds).data_ptr(), ok_dev_ptr=d_ok.data_ptr(),
                               box_dev_ptr=d_box.data_ptr() if with_box else 0)

    def copy_back():
        state["host"] = (wv.cpu().numpy()[:n_wp], poff.cpu().numpy(),
                         {"offsets": coff.cpu().numpy(), "boxes": box["boxes"].cpu().numpy()[:total], "boxes_pos": box["boxes_pos"].cpu().numpy()[:total],
                          "entry": box["entry"].cpu().numpy()[:total], "status": box["status"].cpu().numpy()})

    def numpy_route():
        wv_h, off_h, cor = state["host"]
        state["numpy"] = fiesta_amd.corridor_bounds(wv_h, off_h, cor, inset=inset)

    def numpy_with_copy():
        copy_back()
        numpy_route()

    def upload():
        d_bounds_up[:n_wp].copy_(torch.from_numpy(state["numpy"][0]))

    def bounds_host():
        wv_h, off_h, cor = state["host"]
        state["host_call"] = m.CorridorBounds(wv_h, off_h, cor, inset=inset)

    def refine(its, bounds):
        m.PathRefineDevice(wp.data_ptr(), n_wp, poff.data_ptr(), n, bounds.data_ptr(), out={"waypoints": d_out.data_ptr(), "status": d_rstatus.data_ptr()},
                           iterations=its, **PAR)

    corridor()
    m.synchronize()
    copy_back()
    numpy_route()
    calls = (("corridor_ms", corridor), ("bounds_dev_ms", bounds_dev), ("bounds_dev_no_box_ms", lambda: bounds_dev(with_box=False)),
             ("bounds_host_ms", bounds_host), ("numpy_ms", numpy_route), ("numpy_with_copy_ms", numpy_with_copy), ("bounds_upload_ms", upload),
             ("refine8_ms", lambda: refine(8, d_bounds)), ("refine32_ms", lambda: refine(32, d_bounds)))
    ts = {k: [] for k, _ in calls}
    for it in range(args.warmup + args.steps):
        for key, fn in calls:
            t, _ = clock(fn)
            if it >= args.warmup:
                ts[key].append(t * 1e3)
    r = {k: statistics.median(v) for k, v in ts.items()}
    # ---- the checks, on the whole batch ----
    same = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64)))  # noqa: E731
    wv_h, off_h, cor = state["host"]
    want_b, want_ok = state["numpy"]
    lens = np.diff(off_h)
    rows_ok = np.repeat(want_ok, lens)
    checks = {"no_negative_zero": not bool(np.signbit(cor["boxes_pos"][cor["boxes_pos"] == 0]).any())}
    clock(lambda: bounds_dev(void_broken=False))
    checks["dev_bounds_equal_corridor_bounds"] = same(d_bounds.cpu().numpy()[:n_wp], want_b)
    checks["dev_ok_equals_corridor_bounds"] = bool(np.array_equal(d_ok.cpu().numpy() != 0, want_ok))
    checks["host_bounds_equal_corridor_bounds"] = same(state["host_call"]["bounds"], want_b)
    checks["host_ok_equals_corridor_bounds"] = bool(np.array_equal(state["host_call"]["ok"] != 0, want_ok))
    has_box = d_box.cpu().numpy()[:n_wp] >= 0
    checks["box_is_set_where_bounds_are"] = bool(np.array_equal(has_box, ~np.isnan(want_b[:, 0])))
    clock(bounds_dev)                                                            # VOID_BROKEN: what the all-device chain refines in
    void = d_bounds.cpu().numpy()[:n_wp]
    checks["void_rows_are_the_broken_paths"] = bool(np.array_equal(np.isnan(void[:, 0]), ~rows_ok | np.isnan(want_b[:, 0])) and same(void[rows_ok], want_b[rows_ok]))
    clock(lambda: refine(32, d_bounds))
    chain_dev, chain_status = d_out.cpu().numpy()[:n_wp].copy(), d_rstatus.cpu().numpy().copy()
    upload()
    clock(lambda: refine(32, d_bounds_up))
    chain_host = d_out.cpu().numpy()[:n_wp]
    wp_h = wp.cpu().numpy()[:n_wp]
    checks["device_chain_equals_host_bounds_chain_on_ok_paths"] = same(chain_dev[rows_ok], chain_host[rows_ok])
    checks["device_chain_leaves_broken_paths_alone"] = bool(same(chain_dev[~rows_ok], wp_h[~rows_ok]) and (chain_status[~want_ok & (lens > 2)] == 1).all()
                                                            and (chain_status[want_ok] == 0).all())
    rev = open(os.path.join(ROOT, ".fiesta_rev")).read().strip() if os.path.exists(os.path.join(ROOT, ".fiesta_rev")) else None
    from path_query_bench import source_digest
    out_bytes = n_wp * 56 + n * 4
    r.update(numpy_with_copy_over_dev=r["numpy_with_copy_ms"] / r["bounds_dev_ms"], numpy_over_dev=r["numpy_ms"] / r["bounds_dev_ms"],
             dev_output_gb_per_s=out_bytes / (r["bounds_dev_ms"] * 1e-3) / 1e9,
             dev_below_corridor_and_refine8=bool(r["bounds_dev_ms"] < r["corridor_ms"] and r["bounds_dev_ms"] < r["refine8_ms"]))
    res = {"metric": "corridor_bounds_numpy_route_with_copy_over_device_call", "value": r["numpy_with_copy_over_dev"], "unit": "x",
           "scene": f"partial{G}", "grid": G, "revision": rev, "source_sha256": source_digest(), "seed": seed[0].tolist(),
           "box": [lo.tolist(), hi.tolist()], "command": f"python tools/corridor_bounds_bench.py --grid {G} --obstacles {args.obstacles} --steps {args.steps} --warmup {args.warmup}", "inset": inset,
           "refine_params": PAR, "paths": n, "waypoints": n_wp, "longest_path": int(lens.max()) if n else 0,
           "paths_above_one_chunk": int((lens > 64).sum()), "boxes": total, "corridors_whole": int(want_ok.sum()),
           "waypoints_moved_by_refine32": int((chain_dev != wp_h).any(axis=1).sum()), "output_bytes": out_bytes, "times": r, "steps": args.steps,
           "warmup": args.warmup, "checks": checks, "all_checks": all(checks.values())}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        open(os.path.join(args.out, f"corridor_bounds_partial{G}.json"), "w").write(line + "\n")
    m.close()
    return 0 if res["all_checks"] else 1


if __name__ == "__main__":
    sys.exit(main())
