#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X-native incremental ESDF engine.

Metric (BASELINE.json): ESDF updated-voxels/sec (+ UpdateESDF p50 latency) on the 512^3 dense grid with a
50k-voxel insert+delete delta.  A *step* is one full pass of the hot path over one synthetic batch whose
inputs are already resident in HBM:

    2 x { SetOccupancy(new 25k, hit) ; UpdateOccupancy }                       (log-odds need 3 hits)
    1 x { SetOccupancy(new 25k, hit) + SetOccupancy(oldest 25k, miss) ; UpdateOccupancy }   -> 25k inserts + 25k deletes
    UpdateESDF()                                                               <- the 50k-voxel delta lands here

on top of a fully observed 512^3 map that holds 50k scattered obstacle voxels (scene A of SURVEY.md 8d);
the obstacle population is stationary (oldest 25k leave, 25k new arrive each step).  `value` = voxels
whose (d^2, closest obstacle) changed, summed over the K timed steps, divided by the wall time of the K
steps (barrier + synchronize on both sides, max over ranks).  The updated-voxel counts come from an
identical *untimed* replay of the same K steps from a device snapshot (the diff kernel would otherwise sit
inside the timed region).

A plain run sets up, warms up, times the K steps, replays them for the count and prints the line.  --full adds what the
headline does not need (scatter_full_update, verify, parity, cpu_baseline); --dump-outputs DIR writes the last timed step's
field (a seeded sample, dump_outputs()).

Extra objects on the JSON line:
  roofline      algorithmic bytes (16 B per updated voxel) over the SUM of the durations of every kernel
                of UpdateESDF (bulk path: k_ft_rows + k_ft_plane + k_ft_x; frontier rounds: the k_relax_q launches),
                measured live with HIP events on the map's own stream; `dominant_kernel` quotes k_ft_x alone.
  cpu_baseline  (--full) the CPU oracle (verbatim-compiled reference when oracle/_ref is present, else the pinned
                restatement) timed on one host core on a bounded sample of the same workload (same obstacle
                density on a 224^3 grid, --cpu-grid); rank 0, N=1 only.  The one-off measurement of the reference
                at the full 512^3 size (profiles/r02_cpu_512.json, ~2 min per UpdateESDF) is quoted beside it.
                A reported baseline, not the target.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P_DEFAULT = (0.70, 0.35, 0.12, 0.97, 0.80)  # src/parameters.cpp:28-32
HBM_PEAK_GBS = 8000.0                       # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
ALGO_BYTES_PER_UPDATED_VOXEL = 16           # read 8 B + write 8 B of {d^2:int32, coc:int32}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=None,
                    help="voxels per axis OWNED by each rank (default: 512 on one GPU = config 2; 1024 with --gpus N > 1, i.e. "
                         "2048^3 as 2x2x2 shards at N = 8 = config 5)")
    ap.add_argument("--obstacles", type=int, default=None,
                    help="live obstacle voxels per rank (default: config 2's density, 50000 per 512^3)")
    ap.add_argument("--engine", default="auto", choices=["auto", "rounds", "bulk", "levels", "envelope", "cells", "masked"],
                    help="UpdateESDF engine: chosen per update (default), frontier rounds only, or the bulk feature "
                         "transform whenever the map state allows it")
    ap.add_argument("--unobserved", type=float, default=0.0,
                    help="C2-partial: fraction of the 32^3-voxel blocks of the grid that are NEVER observed (0.27 = SURVEY.md appendix "
                         "B's checkerboard); the bulk transform's gate stays shut, the line measures the general engine")
    ap.add_argument("--scene", default="scatter", choices=["scatter", "surfaces"],
                    help="C2 obstacle distribution: uniform scatter (headline) or depth-sensor-like shells (scene C)")
    ap.add_argument("--pin-depth", action="store_true",
                    help="C3: the host depth images live in pinned memory (what a node that owns its image buffers can do: "
                         "the upload inside the timed region becomes one DMA instead of the runtime's staging copy)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-grid", type=int, default=224)
    ap.add_argument("--no-cpu-full", action="store_true",
                    help="skip the full-size leg of cpu_baseline (the verbatim reference on the SAME 512^3 step, one host core, "
                         "about 4 minutes and 7.4 GB; default on at N = 1 when oracle/_ref is present)")
    ap.add_argument("--delta", type=int, default=None,
                    help="voxels replaced per step (inserts + deletes; default: the whole obstacle count = config 2's 50k delta)")
    ap.add_argument("--delta-sweep", action="store_true",
                    help="engine crossover table instead of the headline: UpdateESDF p50 for deltas 100 ... 50k on every engine")
    ap.add_argument("--verify-samples", type=int, default=20000,
                    help="owned voxels per rank checked after the timed region against a k-d tree over the GLOBAL obstacle list")
    ap.add_argument("--workload", default="c2", choices=["c2", "c3", "c4", "queries"],
                    help="c2 = the headline metric; c3 = depth-frame pipeline; c4 = hash-block map, streaming window")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for smoke tests)")
    ap.add_argument("--force-sharded", action="store_true", help="run the sharded driver even with one rank (smoke test)")
    ap.add_argument("--replicas", action="store_true",
                    help="with --gpus N: N independent maps instead of one spatially sharded map")
    ap.add_argument("--full", action="store_true",
                    help="also what the headline does not need: the scatter insert's own figures, the k-d tree self-check (verify), "
                         "the parity quote of the committed fixtures and the CPU baseline (off: set up, warm up, time the steps, "
                         "print the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32 / float64): "
                         "distances and occupancy of a fixed seeded sample of voxels, and the distances of the middle z-plane")
    return ap.parse_args()


class Workload:
    """Deterministic stationary workload: `n_obs` live obstacle voxels, half replaced per step.  scene "scatter":
    uniform voxels (SURVEY.md 8d, C2 scenes A/B); "surfaces": voxels sampled on 3 axis-aligned planes and 20 spheres
    of radius 8-40 voxels, the shells a depth sensor produces (C2 scene C)."""

    def __init__(self, grid, n_obs, seed=12345, scene="scatter", delta=None):
        self.grid, self.n_obs, self.scene = grid, n_obs, scene
        self.half = (n_obs if delta is None else min(delta, n_obs)) // 2   # inserts (= deletes) per step
        self.rng = np.random.RandomState(seed)
        g = grid
        srng = np.random.RandomState(4242)  # the surfaces themselves are the same for every rank / step
        self.planes = [(int(a), int(srng.randint(g // 8, g - g // 8))) for a in range(3)]
        self.spheres = [(srng.randint(g // 8, g - g // 8, 3), float(srng.uniform(8, 40))) for _ in range(20)]
        self.live = self._fresh(n_obs, np.empty((0, 3), np.int64))
        self.step_id = 0

    def _sample(self, k):
        if self.scene == "scatter":
            return self.rng.randint(0, self.grid, (k, 3))
        g, out = self.grid, np.empty((k, 3), np.int64)
        which = self.rng.randint(0, 23, k)  # 3 planes + 20 spheres, equally likely
        for i in range(k):
            w = which[i]
            if w < 3:
                ax, pos = self.planes[w]
                v = self.rng.randint(0, g, 3)
                v[ax] = pos
            else:
                c, r = self.spheres[w - 3]
                d = self.rng.normal(size=3)
                v = np.rint(c + r * d / np.linalg.norm(d)).astype(np.int64)
            out[i] = np.clip(v, 0, g - 1)
        return out

    def _fresh(self, k, taken):
        """k voxels not in `taken` and distinct from each other: the draws in order, a voxel kept at its first occurrence
        unless taken, more drawn until k are kept (array operations: the stage of a long run is not a Python loop per voxel)."""
        g = self.grid
        lin = lambda c: (c[:, 0].astype(np.int64) * g + c[:, 1]) * g + c[:, 2]   # noqa: E731
        seen = np.sort(lin(np.asarray(taken).reshape(-1, 3)))
        shift = max(1, int(k).bit_length())
        assert (g ** 3 - 1).bit_length() + shift < 63
        out, n = [], 0
        while n < k:
            c = self._sample(k - n)
            key = np.sort((lin(c) << shift) | np.arange(len(c)))    # by voxel, then by draw order
            code, idx = key >> shift, key & ((1 << shift) - 1)
            first = np.ones(len(c), bool)
            first[1:] = code[1:] != code[:-1]                        # first occurrence within the draw
            if len(seen):
                pos = np.minimum(np.searchsorted(seen, code), len(seen) - 1)
                first &= seen[pos] != code                           # not taken
            keep = np.zeros(len(c), bool)
            keep[idx[first]] = True
            out.append(c[keep])
            n += int(keep.sum())
            if n < k:
                seen = np.sort(np.concatenate([seen, code[first]]))
        return np.concatenate(out).astype(np.int32) if out else np.empty((0, 3), np.int32)

    def initial(self):
        return self.live.copy()

    def next_step(self):
        """(new voxels to occupy, old voxels to free); the oldest half leaves."""
        old = self.live[: self.half]
        keep = self.live[self.half:]
        new = self._fresh(self.half, self.live)
        self.live = np.concatenate([keep, new])
        self.step_id += 1
        return new, old.copy()


def run_cpu_baseline(args, grid=None):
    """The oracle on one host core: same obstacle density on `grid`^3 (default: the --cpu-grid sample), one steady-state
    step timed.  grid = args.grid is the SAME step the GPU ran (same seeds, same voxels): the full-size leg."""
    from oracle import pyoracle
    pyoracle.build("port")
    kind = "ref" if pyoracle.available("ref", "array") else "port"
    g = args.cpu_grid if grid is None else grid
    n_obs = max(2, int(round(args.obstacles * (g / args.grid) ** 3)))
    res = 0.1
    t_all = time.perf_counter()
    m = pyoracle.OracleMap((0, 0, 0), res, ((g - 0.5) * res,) * 3, kind=kind)  # ceil() rounding, SURVEY 7.3-G
    assert m.grid_total_size == g ** 3
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    for x0 in range(0, g, 64):      # observe everything free, in slabs (the coordinate list of 512^3 would be 1.6 GB)
        xs = np.arange(x0, min(g, x0 + 64))
        allv = np.stack(np.meshgrid(xs, np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
        if args.unobserved > 0:   # the same never-observed 32^3 blocks as on the GPU (grids that hold whole blocks)
            keep = np.random.RandomState(2718).rand(args.grid // 32, args.grid // 32, args.grid // 32) >= args.unobserved
            blk = allv // 32
            ok = np.all(blk < np.array(keep.shape), axis=1)
            allv = allv[ok][keep[blk[ok, 0], blk[ok, 1], blk[ok, 2]]]
        m.SetOccupancyVox(allv, 0)
    del allv
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    w = Workload(g, n_obs, scene=args.scene, delta=args.delta)
    for _ in range(3):
        m.SetOccupancyVox(w.initial(), 1)
        m.UpdateOccupancy(True)
    st_scatter = m.UpdateESDF()
    before = m.dump_dense(("dist", "coc", "occ"))
    new, old = w.next_step()
    for c in range(3):
        m.SetOccupancyVox(new, 1)
        if c == 2:
            m.SetOccupancyVox(old, 0)
        m.UpdateOccupancy(True)
    st = m.UpdateESDF()
    after = m.dump_dense(("dist", "coc", "occ"))
    changed = before["dist"] != after["dist"]
    bc = before["coc"].astype(np.int64)
    has = bc[:, 0] >= 0
    lin = (bc[:, 0] * g + bc[:, 1]) * g + bc[:, 2]
    gone = np.zeros(len(lin), bool)
    gone[has] = after["occ"][lin[has]] == 0
    updated = int((changed | gone).sum())
    m.close()
    return {
        "value": updated / st["seconds"], "unit": "voxels/s", "cores": 1, "kind": "reference" if kind == "ref" else "port",
        "sample": f"{g}^3 grid at the same obstacle density ({n_obs} obstacles), one steady-state UpdateESDF "
                  f"({st['inserted']} inserts + {st['deleted']} deletes, {updated} updated voxels, {st['seconds']:.3f} s); "
                  f"full scatter insert of the sample: {g ** 3} voxels in {st_scatter['seconds']:.3f} s",
        "update_esdf_s": st["seconds"], "updated_voxels": updated, "host_cpus": os.cpu_count(), "cpu_model": cpu_model(),
        "wall_s": time.perf_counter() - t_all,
    }


def revision():
    """the commit the library was built from (__graft_entry__.build() stamps it; the GPU box has no .git)"""
    try:
        return open(os.path.join(ROOT, ".fiesta_rev")).read().strip()
    except OSError:
        return None


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def free_host_gb():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable"):
                return int(line.split()[1]) / 1e6
    except OSError:
        pass
    return 0.0


def verify_against_kdtree(query_d2, owned_lo, owned_size, obstacles, n_samples, seed, wrap):
    """Self-check of a run (N = 1 and every rank of N > 1): n_samples voxels of this rank's owned box -- a third of them
    within 3 voxels of the box faces, where shards meet -- against the exact nearest obstacle of the GLOBAL list (k-d tree;
    squared distances recomputed in integers).  wrap: on grids beyond 1024 voxels per axis an id reaches 512 voxels
    (d^2 < 2^18), farther voxels read "no obstacle".  Returns (sampled, mismatches)."""
    from scipy.spatial import cKDTree
    rng = np.random.RandomState(seed)
    lo, size = np.asarray(owned_lo, np.int64), np.asarray(owned_size, np.int64)
    v = lo + (rng.rand(n_samples, 3) * size).astype(np.int64)
    k = n_samples // 3
    ax = rng.randint(0, 3, k)
    side = rng.randint(0, 2, k)
    off = rng.randint(0, 3, k)
    v[np.arange(k), ax] = np.where(side == 0, lo[ax] + off, lo[ax] + size[ax] - 1 - off)
    obs = np.asarray(obstacles, np.int64)
    _, nn = cKDTree(obs.astype(np.float64)).query(v.astype(np.float64), k=4)   # (ties / float rounding: best of 4 in integers)
    want = ((v[:, None, :] - obs[nn]) ** 2).sum(-1).min(1)
    if wrap:
        want = np.where(want >= (1 << 18), 0x7FFFFFFF, want)
    got = np.asarray(query_d2(v.astype(np.int32)), np.int64)
    return int(len(v)), int((got != want).sum())


def esdf_summary(stats):
    """What the timed UpdateESDF calls were: medians of the engine's own counters (fiesta_hip_stats)."""
    if not stats:
        return None
    med = lambda k: float(statistics.median([st[k] for st in stats]))   # noqa: E731
    out = {k: med(k) for k in ("inserted", "deleted", "rounds", "relax_launches", "voxel_writes", "device_ms", "relax_ms")}
    out["engine"] = {"levels": sum(int(st.get("levels", 0)) for st in stats), "bulk": sum(int(st.get("bulk", 0)) for st in stats), "calls": len(stats)}
    if any(st.get("levels") for st in stats):   # level engine: time inside its one-work-group kernel, entries processed, largest frontier
        lv = [st for st in stats if st.get("levels")]
        out["level_kernel_us"] = float(statistics.median([st["prof"][0] for st in lv])) / 1e3
        out["frontier_entries"] = float(statistics.median([st["prof"][6] for st in lv]))
        out["frontier_peak"] = float(statistics.median([st["prof"][7] for st in lv]))
        # thread 0's view of the one-work-group kernel: fetch + pull, barrier, push, append + barriers (us per update)
        out["level_phases_us"] = [float(statistics.median([st["prof"][k] for st in lv])) / 1e3 for k in (2, 3, 4, 5)]
    return out


def run_c3(args):
    """BASELINE config 3 (`--workload c3`): 512^3 @0.1 m fed by 640x480 synthetic depth frames through the HIP ray cast
    (fiesta_hip_raycast_depth) -> UpdateOccupancy -> UpdateESDF on one MI355X.  Scene: 6x6x3 m box
    room with 5 spheres, sensor at the grid centre, yaw sweep 2 deg/frame, ray window 0.5-5.0 m, the reference's
    de-duplication semantics.  One JSON line: rays/s, per-stage p50 ms, frame p50; cpu_baseline = the oracle on the
    first frames (whose hit/miss counters must be bit-identical to the GPU's)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scenarios import depth_to_points, render_depth, yaw_pose
    import fiesta_amd
    from scenarios import INTRINSICS as intr  # the reference's defaults, src/parameters.cpp:21-24
    G, res = args.grid, 0.1
    half = G * res / 2
    origin, size = (-half, -half, -half), (G * res,) * 3
    m = fiesta_amd.ESDFMap(origin, res, size, update_engine=args.engine)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    cpu, cpu_frames = None, 0 if args.no_cpu_baseline else 2
    if cpu_frames:
        from oracle import pyoracle
        pyoracle.build("port")
        kind = "ref" if pyoracle.available("ref", "array") else "port"
        cpu = pyoracle.OracleMap(origin, res, size, kind=kind)
        cpu.SetParameters(*P_DEFAULT)
        cpu.SetOriginalRange()
    spheres = [((1.5, 0.5, 0.0), 0.5), ((-1.0, 2.0, 0.3), 0.7), ((0.5, -2.0, -0.5), 0.4), ((-2.0, -1.0, 0.5), 0.6),
               ((2.2, -1.8, 0.2), 0.3)]
    nframes = args.warmup + args.steps
    frames, pins = [], []
    for f in range(nframes):
        T = yaw_pose(2.0 * f, (0.0, 0.0, 0.0))
        depth = render_depth(T, rows=480, cols=640, spheres=spheres, intr=intr)
        if args.pin_depth:
            import torch
            pinned = torch.from_numpy(np.ascontiguousarray(depth)).pin_memory()
            pins.append(pinned)            # (keeps the pinned storage alive)
            depth = pinned.numpy()
        frames.append((T, depth))
    lc, rc = origin, tuple(np.add(origin, size))
    t_ray, t_fuse, t_esdf, t_all, cpu_t, esdf_stats, updated, parity, traces = [], [], [], [], [], [], [], None, []
    for f, (T, depth) in enumerate(frames):
        checked = cpu is not None and f < cpu_frames
        t0 = time.perf_counter()
        m.RaycastDepth(depth, intr["fx"], intr["fy"], intr["cx"], intr["cy"], T, T[:3, 3], 0.5, 5.0, lc, rc, dedup=1)
        m.synchronize()
        t1 = time.perf_counter()
        if checked:
            pts = depth_to_points(depth, intr)
            c0 = time.perf_counter()
            cpu.raycast_frame(pts, T, T[:3, 3], 0.5, 5.0, lc, rc)
            c1 = time.perf_counter()
            gh, gm = m.download_counts()
            ch, cm = cpu.dump_counts()
            assert np.array_equal(gm, cm) and np.array_equal(gh, ch), "hit/miss counters differ from the oracle"
        t1b = time.perf_counter()
        m.UpdateOccupancy(True)
        m.synchronize()
        t2a = time.perf_counter()
        if not checked:
            m.snapshot_save(0)       # (the benchmark's unit: voxels whose (d^2, obstacle) changes -- outside the timers)
            m.synchronize()
        t2 = time.perf_counter()
        st = m.UpdateESDF()
        t3 = time.perf_counter()
        if not checked and f >= args.warmup:
            updated.append(m.snapshot_count_updated(0))
            if st.get("levels"):
                traces.append(m.level_trace()[0])
        if checked:
            c2 = time.perf_counter()
            cpu.UpdateOccupancy(True)
            c3 = time.perf_counter()
            sc = cpu.UpdateESDF()
            c4 = time.perf_counter()
            assert (st["inserted"], st["deleted"]) == (sc["inserted"], sc["deleted"])
            cpu_t.append({"raycast_ms": (c1 - c0) * 1e3, "fuse_ms": (c3 - c2) * 1e3, "esdf_ms": (c4 - c3) * 1e3})
            if f == cpu_frames - 1:  # the field after the checked frames against the reference's, voxel by voxel
                from scenarios import D2_INF, d2_from_dist
                gd2 = m.download_field(("d2",))["d2"].astype(np.int64)
                od2 = d2_from_dist(cpu.dump_dense(("dist",))["dist"], res)
                fin = (od2 >= 0) & (od2 != D2_INF)
                parity = {"frames": cpu_frames, "voxels": int(len(od2)), "finite": int(fin.sum()), "observed_sets_equal": bool(np.array_equal(gd2 < 0, od2 < 0)),
                          "d2_differs_from_this_reference_run": int((gd2 != od2).sum()), "closer": int((gd2 < od2).sum()), "farther": int((gd2 > od2).sum()),
                          "note": "a partially observed map: the reference's own distances depend on its queue order there; the same "
                                  "frames (the first three, level engine pinned) are judged against the envelope of 4 reference runs in shuffled order in "
                                  "tests/test_gpu_raycast_parity.py (test_config3_full_size_distances_inside_the_reference_envelope); counters, queues "
                                  "and occupancy of the frames bit-exact in test_config3_640x480_frames_reference_intrinsics"}
        if f >= args.warmup and not checked:
            t_ray.append((t1 - t0) * 1e3)
            t_fuse.append((t2a - t1b) * 1e3)
            t_esdf.append((t3 - t2) * 1e3)
            t_all.append((t1 - t0 + t2a - t1b + t3 - t2) * 1e3)
            esdf_stats.append(st)
    p50 = statistics.median
    out = {
        "metric": "c3_depth_frames_per_sec", "value": 1e3 / p50(t_all), "unit": "frames/s", "n_gpus": 1, "steps": len(t_all),
        "warmup": args.warmup, "ms_per_step": p50(t_all), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64 ray arithmetic, u32 voxel words", "data": "synthetic",
        "config": {"workload": f"C3: {G}^3 @0.1 m, 640x480 depth frames (307200 rays), yaw 2 deg/frame, dedup=1; host "
                               "uint16 image uploaded inside the timed ray cast (PCIe-inclusive)"
                               + (", from PINNED host memory" if args.pin_depth else ", from pageable host memory"),
                   "update_engine": args.engine},
        "raycast_p50_ms": p50(t_ray), "rays_per_sec": 307200 / (p50(t_ray) * 1e-3),
        "update_occupancy_p50_ms": p50(t_fuse), "update_esdf_p50_ms": p50(t_esdf),
        "update_esdf": esdf_summary(esdf_stats),
        "updated_voxels_per_frame": (sum(updated) / len(updated)) if updated else None,
        # one frame's update level by level: (frontier entries, us inside the kernel) -- the frame with the median level count
        "level_trace_of_a_median_frame": sorted(traces, key=len)[len(traces) // 2] if traces else None,
        # UpdateESDF of a sensor frame: a few thousand voxels change -- latency-bound by construction (levels x memory round
        # trips), reported against the same roofline as the headline for completeness
        "roofline": {"bound": "hbm", "kernel": "k_level_run (level engine, one work-group)" if esdf_stats and all(st_.get("levels") for st_ in esdf_stats) else "k_relax_q",
                     "achieved": 16.0 * sum(updated) / max(sum(t_esdf) * 1e-3, 1e-12) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": 16.0 * sum(updated) / max(sum(t_esdf) * 1e-3, 1e-12) / 8e12, "traffic": None,
                     "frac_definition": "16 B x updated voxels / wall time of the UpdateESDF calls / 8 TB/s"} if updated else None,
        "parity": parity,
        "cpu_baseline": {"kind": "reference" if cpu is not None and cpu.describe.startswith("reference") else "port",
                         "cores": 1, "unit": "ms per stage", "sample": "the first frames of the same sequence",
                         "frames": cpu_t, "counters_bit_identical": bool(cpu_t)} if cpu_t else None,
    }
    print(json.dumps(out), flush=True)
    m.close()


def run_c4(args):
    """BASELINE config 4 (`--workload c4`): hash-block map @0.05 m, streaming insert/delete: a
    6 x 6 x 3 m observation window (864 000 voxels) moving through a 40 m volume, per frame: observe the window free
    (fiesta_hip_set_occupancy_box), observe ~16 k surface voxels occupied (device batch), UpdateOccupancy, UpdateESDF
    (tests/scenarios.py: c4_frame).  Inputs are generated before the clock starts and are resident in HBM.  value =
    updated voxels (SURVEY.md 8d unit, counted on the device outside the timed segments) / time of the timed frames.
    cpu_baseline = the reference built with -DHASH_TABLE on the first frames of the same stream."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scenarios import box_voxels, c4_frame
    import fiesta_amd
    res = 0.05
    m = fiesta_amd.ESDFMap((0.0, 0.0, 0.0), res, reserve_size=1000000, mode="hash", update_engine=args.engine)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    nframes = args.warmup + args.steps
    dev = torch.device("cuda", 0)
    frames = []
    for k in range(nframes):
        lo, hi, occ = c4_frame(k)
        v = torch.from_numpy(occ).to(dev)
        frames.append((lo, hi, occ, v, torch.ones(len(occ), dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    t_obs, t_fuse, t_esdf, upd, relax_ms, launches, esdf_stats = [], [], [], [], [], [], []
    for k, (lo, hi, occ, v, o) in enumerate(frames):
        t0 = time.perf_counter()
        m.SetOccupancyBox(lo, hi, 0)
        m.SetOccupancyDevice(v.data_ptr(), o.data_ptr(), len(occ))
        m.synchronize()
        t1 = time.perf_counter()
        m.UpdateOccupancy(True)
        m.synchronize()
        t2 = time.perf_counter()
        m.snapshot_save(0)
        t3 = time.perf_counter()
        st = m.UpdateESDF()
        t4 = time.perf_counter()
        n_upd = m.snapshot_count_updated(0)
        if k >= args.warmup:
            t_obs.append(t1 - t0), t_fuse.append(t2 - t1), t_esdf.append(t4 - t3), upd.append(n_upd)
            relax_ms.append(st["relax_ms"]), launches.append(st["relax_launches"])
            esdf_stats.append(st)
    total_s = sum(t_obs) + sum(t_fuse) + sum(t_esdf)
    pages = m.grid_total_size_ // 8192
    cpu, parity = None, None
    if not args.no_cpu_baseline:
        from oracle import pyoracle
        pyoracle.build("port")
        kind = "ref" if pyoracle.available("ref", "hash") else "port"
        c = pyoracle.OracleMap((0.0, 0.0, 0.0), res, reserve_size=1000000, mode="hash", kind=kind)
        c.SetParameters(*P_DEFAULT)
        c.SetOriginalRange()
        cu, ct, ce = 0, 0.0, 0.0
        ncpu = 0
        # a second HIP map takes the same frames in lockstep (untimed): the two fields are compared voxel by voxel at the end
        g2 = fiesta_amd.ESDFMap((0.0, 0.0, 0.0), res, reserve_size=1000000, mode="hash", update_engine=args.engine)
        g2.SetParameters(*P_DEFAULT)
        g2.SetOriginalRange()
        for k in range(nframes):
            lo, hi, occ = c4_frame(k)
            bv = box_voxels(lo, hi)
            g2.SetOccupancyBox(lo, hi, 0)
            g2.SetOccupancy(occ, 1, want_ret=False)
            g2.UpdateOccupancy(True)
            g2.UpdateESDF()
            c0 = time.perf_counter()
            c.SetOccupancyVox(bv, 0)
            c.SetOccupancyVox(occ, 1)
            c.UpdateOccupancy(True)
            c1 = time.perf_counter()
            before = c.dump_hash()
            c2 = time.perf_counter()
            sc = c.UpdateESDF()
            c3 = time.perf_counter()
            after = c.dump_hash()
            nb = len(before["dist"])
            ch = (after["dist"][:nb] != before["dist"]) | np.any(after["coc"][:nb] != before["coc"], axis=1)
            cu += int(ch.sum()) + int((after["dist"][nb:] != -10000).sum())
            ct += (c1 - c0) + (c3 - c2)
            ce += c3 - c2
            ncpu += 1
            if ct > 20.0:
                break
        from scenarios import D2_INF, d2_from_dist, hash_key
        gd, cd = g2.download_hash(), c.dump_hash()
        okc = cd["vox"][:, 0] != -10000
        ck, cdd = hash_key(cd["vox"][okc]), d2_from_dist(cd["dist"][okc], res)
        gk, gdd = hash_key(gd["vox"]), gd["d2"].astype(np.int64)
        # (the reference also allocates the blocks its neighbour reads touch: pristine forever; compared over the observed voxels)
        co, go = np.argsort(ck), np.argsort(gk)
        ck, cdd, gk, gdd = ck[co], cdd[co], gk[go], gdd[go]
        cobs, gobs = ck[cdd >= 0], gk[gdd >= 0]
        same_sets = bool(np.array_equal(cobs, gobs))
        both = np.intersect1d(cobs, gobs)
        cv, gv = cdd[np.searchsorted(ck, both)], gdd[np.searchsorted(gk, both)]
        parity = {"frames": ncpu, "observed_voxels": int(len(cobs)), "observed_sets_equal": same_sets,
                  "finite": int(((cv >= 0) & (cv != D2_INF)).sum()), "d2_differs_from_this_reference_run": int((cv != gv).sum()),
                  "closer": int((gv < cv).sum()), "farther": int((gv > cv).sum()),
                  "note": "a partially observed, streaming map: judged against the envelope of shuffled reference runs in "
                          "tests/test_gpu_hash_parity.py (test_hash_c4_stream_box_observe: the first 4 frames of this stream, no deletes yet)"}
        g2.close()
        cpu = {"value": cu / ct, "unit": "voxels/s", "cores": 1, "kind": "reference" if c.describe.startswith("reference") else "port",
               "sample": f"the first {ncpu} frames of the same stream (ingest + UpdateOccupancy + UpdateESDF, {ct:.1f} s; changed "
                         f"(distance, obstacle) entries {cu}); UpdateESDF alone {ce:.1f} s", "update_esdf_voxels_per_sec": cu / max(ce, 1e-9)}
    sum_relax_s = sum(relax_ms) * 1e-3
    n_launch = max(1, int(sum(launches)))
    out = {
        "metric": "c4_hash_updated_voxels_per_sec", "value": sum(upd) / total_s, "unit": "voxels/s", "n_gpus": 1,
        "steps": len(upd), "warmup": args.warmup, "ms_per_step": 1e3 * total_s / len(upd), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u32", "data": "synthetic",
        "config": {"workload": "C4: hash-block map (16x16x32-voxel pages behind a dense directory) @0.05 m, reserve 1e6, a "
                               "120x120x60-voxel observation window streaming 3 voxels/frame through a 40 m volume: per frame "
                               "864000 free + ~16400 occupied observations, UpdateOccupancy, UpdateESDF; inputs resident in HBM"},
        "observe_p50_ms": 1e3 * statistics.median(t_obs), "update_occupancy_p50_ms": 1e3 * statistics.median(t_fuse),
        "update_esdf_p50_ms": 1e3 * statistics.median(t_esdf), "updated_voxels_per_frame": sum(upd) / len(upd),
        "update_esdf_voxels_per_sec": sum(upd) / sum(t_esdf), "allocated_pages": int(pages),
        "allocated_voxels": int(m.grid_total_size_), "update_esdf": esdf_summary(esdf_stats),
        "roofline": {"bound": "hbm", "kernel": "k_level_run / k_level_pull+push<PagedSpace>" if any(st.get("levels") for st in esdf_stats) else "k_relax_q<16,16,1024,PAGED>", "achieved": 16.0 * sum(upd) / max(sum_relax_s, 1e-12) / 1e9,
                     "peak": 8000.0, "unit": "GB/s", "frac": 16.0 * sum(upd) / max(sum_relax_s, 1e-12) / 8e12, "traffic": None,
                     "launches": n_launch, "avg_launch_us": 1e6 * sum_relax_s / n_launch},
        "parity": parity,
        "cpu_baseline": cpu,
    }
    print(json.dumps(out), flush=True)
    m.close()


def run_queries(args):
    """`--workload queries`: the consumer side of the path (src/ESDFMap.cpp:467-540).  Config 2's map
    (512^3, 50 000 scattered obstacles, fully observed), then
      batch   N device-resident positions through fiesta_hip_get_dist_grad_dev (GetDistWithGradTrilinear: 8 corner words, f64
              value + gradient), queries/s and the fraction of the HBM roofline at SURVEY.md 8d's 64 B per query;
      scalar  ONE position per call through the drop-in C++ class (examples/query_latency.cpp, compiled here): a random walk,
              uniformly random positions, the first call after an update -- the host-side brick cache;
      cpu     the verbatim reference's GetDistWithGradTrilinear in a loop on one host core, a bounded sample (256^3 map of the
              same obstacle density, 2 M positions)."""
    import subprocess
    import tempfile
    import torch
    import fiesta_amd
    G, res = args.grid, 0.1
    dev = torch.device("cuda", 0)
    m = fiesta_amd.ESDFMap((0, 0, 0), res, (G * res,) * 3, update_engine=args.engine)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((0, 0, 0), (G - 1,) * 3, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    w = Workload(G, args.obstacles, seed=12345)
    for _ in range(3):
        m.SetOccupancy(w.initial(), 1, want_ret=False)
        m.UpdateOccupancy(True)
    st = m.UpdateESDF()
    N = 8_000_000
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    pos = (torch.rand((N, 3), generator=gen, device=dev, dtype=torch.float64) * (G * res - 0.6) + 0.3).contiguous()
    dist = torch.empty(N, device=dev, dtype=torch.float64)
    grad = torch.empty((N, 3), device=dev, dtype=torch.float64)
    for _ in range(args.warmup):
        m.GetDistWithGradTrilinearDevice(pos.data_ptr(), N, dist.data_ptr(), grad.data_ptr())
    m.synchronize()
    ts = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        m.GetDistWithGradTrilinearDevice(pos.data_ptr(), N, dist.data_ptr(), grad.data_ptr())
        m.synchronize()
        ts.append(time.perf_counter() - t0)
    t = statistics.median(ts)
    # a PLANNER's batch: trajectories, not white noise -- 8192 smooth paths of 1024 samples each, 0.4 voxels
    # apart, stored path by path: neighbouring lanes ask about neighbouring positions (the 8 corner words of consecutive
    # queries share their 128-byte lines)
    T_, L_ = 8192, N // 8192
    gen.manual_seed(11)
    start = torch.rand((T_, 1, 3), generator=gen, device=dev, dtype=torch.float64) * (G * res - 4.0) + 2.0
    head = torch.randn((T_, 1, 3), generator=gen, device=dev, dtype=torch.float64)
    turn = torch.randn((T_, L_, 3), generator=gen, device=dev, dtype=torch.float64) * 0.05
    dirs = head + torch.cumsum(turn, 1)
    dirs = dirs / dirs.norm(dim=2, keepdim=True)
    path = start + torch.cumsum(dirs * (0.4 * res), 1)
    lo_b, span = 0.3, G * res - 0.6
    path = lo_b + span - (torch.remainder(path - lo_b, 2 * span) - span).abs()   # (reflected at the map's faces)
    ppos = path.reshape(-1, 3).contiguous()
    del start, head, turn, dirs, path
    for _ in range(args.warmup):
        m.GetDistWithGradTrilinearDevice(ppos.data_ptr(), N, dist.data_ptr(), grad.data_ptr())
    m.synchronize()
    tp = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        m.GetDistWithGradTrilinearDevice(ppos.data_ptr(), N, dist.data_ptr(), grad.data_ptr())
        m.synchronize()
        tp.append(time.perf_counter() - t0)
    tpl = statistics.median(tp)
    m.GetDistWithGradTrilinearDevice(pos.data_ptr(), N, dist.data_ptr(), grad.data_ptr())   # (the check below reads the random batch's results)
    m.synchronize()
    # check a sample against the exact transform (k-d tree) -- trilinear of exact corner distances, recomputed in numpy f64
    from scipy.spatial import cKDTree
    occ = np.ascontiguousarray(m.GetOccupiedVoxels(), dtype=np.int64)
    tree = cKDTree(occ)
    ps = pos[:20000].cpu().numpy()
    b = np.floor((ps - 0.5 * res) / res).astype(np.int64)
    f = (ps - (b + 0.5) * res) / res
    corner = np.stack([b + np.array(o) for o in [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]], 1)   # n x 8 x 3
    dcorner = tree.query(corner.reshape(-1, 3))[0].reshape(-1, 8) * res
    wts = np.stack([(f[:, 0] if i else 1 - f[:, 0]) * (f[:, 1] if j else 1 - f[:, 1]) * (f[:, 2] if k else 1 - f[:, 2])
                    for i in (0, 1) for j in (0, 1) for k in (0, 1)], 1)
    want = (wts * dcorner).sum(1)
    err = float(np.abs(dist[:20000].cpu().numpy() - want).max())
    # scalar calls through the C++ class
    scalar = None
    try:
        exe = os.path.join(tempfile.mkdtemp(), "query_latency")
        subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "query_latency.cpp"),
                        "-L" + os.path.join(ROOT, "fiesta_amd"), "-lfiesta_hip", "-Wl,-rpath," + os.path.join(ROOT, "fiesta_amd"), "-o", exe], check=True)
        scalar = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
    except Exception as e:   # (no host compiler on the box: the batch line stands on its own)
        scalar = {"error": str(e)}
    cpu = None
    if not args.no_cpu_baseline:
        from oracle import pyoracle
        pyoracle.build("port")
        kind = "ref" if pyoracle.available("ref", "array") else "port"
        g2 = 256
        c = pyoracle.OracleMap((0, 0, 0), res, (g2 * res,) * 3, kind=kind)
        c.SetParameters(*P_DEFAULT)
        c.SetOriginalRange()
        c.SetOccupancyVox(np.ascontiguousarray(np.stack(np.meshgrid(*[np.arange(g2, dtype=np.int32)] * 3, indexing="ij"), -1).reshape(-1, 3)), 0)
        c.UpdateOccupancy(True)
        c.UpdateESDF()
        w2 = Workload(g2, int(round(50000 * (g2 / 512.0) ** 3)), seed=12345)
        for _ in range(3):
            c.SetOccupancyVox(w2.initial(), 1)
            c.UpdateOccupancy(True)
        c.UpdateESDF()
        pc = np.random.RandomState(7).rand(2_000_000, 3) * (g2 * res - 0.6) + 0.3
        t0 = time.perf_counter()
        c.GetDistWithGradTrilinear(pc)
        tc = time.perf_counter() - t0
        cpu = {"value": len(pc) / tc, "unit": "queries/s", "cores": 1, "kind": "reference" if c.describe.startswith("reference") else "port",
               "sample": f"2 000 000 uniformly random GetDistWithGradTrilinear calls on a {g2}^3 map of the same obstacle density "
                         f"({tc:.2f} s; cpu: {cpu_model()}, {os.cpu_count()} cores, 1 used)"}
        c.close()
    bytes_q = 64.0
    out = {"metric": "esdf_trilinear_queries_per_sec", "value": N / t, "unit": "queries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": t * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": f"queries: {N} device-resident uniformly random GetDistWithGradTrilinear positions per step on config 2's map "
                                  f"({G}^3 @0.1 m, {args.obstacles} scattered obstacles, fully observed)", "grid": [G, G, G]},
           "roofline": {"bound": "hbm", "kernel": "k_query_trilinear", "achieved": N * bytes_q / t / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": N * bytes_q / t / 1e9 / HBM_PEAK_GBS, "traffic": None,
                        "frac_definition": "64 B per query (SURVEY.md 8d: 8 corner keys x 8 B) x queries / p50 of the call / 8 TB/s; the engine reads 8 x 4 B "
                                           "words and moves 24 B of position in and 32 B of value + gradient out per query"},
           "planner_batch": {"what": f"{T_} smooth trajectories x {L_} samples 0.4 voxels apart, stored path by path (the same kernel, the same {N} queries per call)",
                             "queries_per_sec": N / tpl, "ms_per_call": tpl * 1e3, "roofline_frac_at_64B_per_query": N * bytes_q / tpl / 1e9 / HBM_PEAK_GBS,
                             "io_bytes_actually_moved_per_query": 24 + 32 + 8, "frac_of_peak_on_position_in_plus_result_out_alone": N * 56.0 / tpl / 1e9 / HBM_PEAK_GBS},
           "verify": {"sampled": 20000, "max_abs_error_m_vs_trilinear_of_exact_corner_distances": err},
           "scalar_calls_through_the_cpp_class": scalar, "cpu_baseline": cpu, "map_update": esdf_summary([st])}
    print(json.dumps(out), flush=True)
    m.close()


def run_delta_sweep(args):
    """`--delta-sweep`: where do the two UpdateESDF engines cross?  C2's map (512^3, 50k obstacles, fully observed), both
    scenes; per step `delta` voxels are replaced (delta/2 inserts + delta/2 deletes in one UpdateESDF); every delta on
    every engine setting (rounds / bulk-whenever-valid / auto).  One JSON line with the table and, per point, how much
    slower `auto` is than the better fixed engine (the engine choice is right when that never exceeds a few percent)."""
    import torch
    import fiesta_amd
    G, res = args.grid, 0.1
    dev = torch.device("cuda", 0)
    deltas = [100, 500, 2000, 5000, 10000, 25000, 50000]
    table = []
    for scene in ("scatter", "surfaces"):
        for engine in ("rounds", "bulk", "auto"):
            m = fiesta_amd.ESDFMap((0, 0, 0), res, (G * res,) * 3, update_engine=engine)
            m.SetParameters(*P_DEFAULT)
            m.SetOriginalRange()
            m.SetOccupancyBox((0, 0, 0), (G - 1, G - 1, G - 1), 0)
            m.UpdateOccupancy(True)
            m.UpdateESDF()
            w = Workload(G, args.obstacles, scene=scene)

            def observe(vox, occ):
                v = torch.from_numpy(np.ascontiguousarray(vox, dtype=np.int32)).to(dev)
                o = torch.from_numpy(np.ascontiguousarray(occ, dtype=np.int32)).to(dev)
                m.SetOccupancyDevice(v.data_ptr(), o.data_ptr(), v.shape[0])
                m.synchronize()
            for _ in range(3):
                observe(w.initial(), np.ones(args.obstacles, np.int32))
                m.UpdateOccupancy(True)
            m.UpdateESDF()
            for delta in deltas:
                w.half = delta // 2
                host, devms, bulk = [], [], []
                for r in range(1 + args.steps):
                    new, old = w.next_step()
                    for c in range(3):
                        if c < 2:
                            observe(new, np.ones(len(new), np.int32))
                        else:
                            observe(np.concatenate([new, old]), np.concatenate([np.ones(len(new), np.int32), np.zeros(len(old), np.int32)]))
                        m.UpdateOccupancy(True)
                    m.synchronize()
                    t0 = time.perf_counter()
                    st = m.UpdateESDF()
                    t1 = time.perf_counter()
                    if r:
                        host.append((t1 - t0) * 1e3), devms.append(st["device_ms"]), bulk.append(int(st["bulk"]))
                table.append({"scene": scene, "engine": engine, "delta": delta, "update_esdf_p50_ms": statistics.median(host),
                              "device_p50_ms": statistics.median(devms), "bulk_updates": int(sum(bulk)), "updates": len(bulk),
                              "last_inserted": int(st["inserted"]), "last_deleted": int(st["deleted"])})
            m.close()
    worst = 0.0
    for scene in ("scatter", "surfaces"):
        for delta in deltas:
            t = {e["engine"]: e["update_esdf_p50_ms"] for e in table if e["scene"] == scene and e["delta"] == delta}
            slow = t["auto"] / min(t["rounds"], t["bulk"]) - 1.0
            worst = max(worst, slow)
            for e in table:
                if e["scene"] == scene and e["delta"] == delta and e["engine"] == "auto":
                    e["auto_slower_than_best_fixed"] = slow
    print(json.dumps({"metric": "esdf_engine_crossover", "value": worst, "unit": "worst relative slowdown of auto vs the better fixed engine",
                      "n_gpus": 1, "steps": args.steps, "higher_is_better": False,
                      "config": {"workload": f"C2 map {G}^3, {args.obstacles} obstacles, scenes scatter + surfaces, deltas {deltas}"},
                      "table": table}), flush=True)


def main():
    args = parse()
    if args.grid is None:
        args.grid = 512 if int(os.environ.get("WORLD_SIZE", "1")) == 1 else 1024
    if args.obstacles is None:
        args.obstacles = int(round(50000 * (args.grid / 512.0) ** 3))
    if args.dump_outputs and (args.delta_sweep or args.workload != "c2"):
        raise SystemExit("bench.py --dump-outputs: the headline workload (c2) only")
    if args.delta_sweep:
        args.steps = min(args.steps, 5)
        return run_delta_sweep(args)
    if args.workload == "c3":
        import torch  # noqa: F401  (one HIP runtime per process: torch first)
        return run_c3(args)
    if args.workload == "c4":
        return run_c4(args)
    if args.workload == "queries":
        import torch  # noqa: F401
        return run_queries(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    import torch
    import fiesta_amd

    if not torch.cuda.is_available() or fiesta_amd.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    if args.backend != "nccl" or os.environ.get("FIESTA_BENCH_ALL_RANKS_ON_GPU0"):
        local_rank = 0  # smoke tests: every rank uses the one visible GPU (with nccl: RCCL refuses)
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or args.force_sharded:
        import torch.distributed as dist_mod
        dist = dist_mod
        if world == 1:  # single-rank smoke test of the sharded driver (no launcher): rendezvous on loopback
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:  # debugging only: several ranks on ONE GPU, messages through host buffers
            dist.init_process_group(args.backend)
    dev = torch.device("cuda", local_rank)
    cdev = dev if args.backend == "nccl" else torch.device("cpu")  # where collective payloads live

    G, res = args.grid, 0.1
    sharded_map = None
    if (world > 1 and not args.replicas) or args.force_sharded:
        # ONE map, spatially sharded: every rank owns a G^3 box of a (layout * G)^3 grid -> weak scaling
        from fiesta_amd.sharded import DistTransport, ShardedESDFMap, rank_coords, shard_layout
        layout = shard_layout(world)
        gg = tuple(G * l for l in layout)
        # native=True: the C++ protocol over RCCL (shard_group.hip) or nothing -- a benchmark must not degrade to the Python
        # spelling of the protocol behind a warning; the line says which protocol ran and the run fails further
        # down if the communicator does not see every rank
        sharded_map = ShardedESDFMap((0, 0, 0), res, gg, world, transport=DistTransport(cdev), devices=(local_rank,),
                                     update_engine=args.engine, native=True if args.backend == "nccl" else None)
        m = sharded_map.shards[rank]
        box_lo = np.array(rank_coords(rank, layout)) * G
        sharded_map.SetParameters(*P_DEFAULT)
        sharded_map.SetOriginalRange()
    else:
        m = fiesta_amd.ESDFMap((0, 0, 0), res, (G * res,) * 3, device=local_rank, update_engine=args.engine)
        assert m.grid_total_size_ == G ** 3, "grid rounding (SURVEY.md 7.3-G)"
        box_lo = np.zeros(3, int)
        m.SetParameters(*P_DEFAULT)
        m.SetOriginalRange()
    top = sharded_map if sharded_map is not None else m   # UpdateOccupancy / UpdateESDF go through the driver

    def dev_batch(vox, occ):
        v = torch.from_numpy(np.ascontiguousarray(vox, dtype=np.int32)).to(dev)
        o = torch.from_numpy(np.ascontiguousarray(occ, dtype=np.int32)).to(dev)
        return v, o

    def observe(batch):
        v, o = batch
        m.SetOccupancyDevice(v.data_ptr(), o.data_ptr(), v.shape[0])

    # ---- prologue: observe every voxel free once (nothing propagates through unobserved voxels)
    if args.unobserved > 0:
        # "C2-partial" (SURVEY.md appendix B's checkerboard of unobserved blocks): 32^3-voxel blocks, a seeded fraction of
        # them never observed -- what every sensor-built map looks like.  The transform's gate stays shut (the map is not
        # fully observed): this is the general engine's headline.
        assert sharded_map is None and G % 32 == 0
        keep = np.random.RandomState(2718).rand(G // 32, G // 32, G // 32) >= args.unobserved
        for bx, by, bz in np.argwhere(keep):
            m.SetOccupancyBox((int(bx) * 32, int(by) * 32, int(bz) * 32), (int(bx) * 32 + 31, int(by) * 32 + 31, int(bz) * 32 + 31), 0)
    else:
        m.SetOccupancyBox(tuple(int(v) for v in box_lo), tuple(int(v) for v in box_lo + G - 1), 0)
    top.UpdateOccupancy(True)
    top.UpdateESDF()

    # ---- scene A: scatter insert of all obstacles into the empty observed grid (reported, not the step)
    w = Workload(G, args.obstacles, seed=12345 + 1000 * rank, scene=args.scene, delta=args.delta)
    init = dev_batch(w.initial() + box_lo.astype(np.int32), np.ones(args.obstacles, np.int32))
    for _ in range(3):
        observe(init)
        top.UpdateOccupancy(True)
    if args.full:
        m.snapshot_save(0)
    t_sc = time.perf_counter()
    st_scatter = top.UpdateESDF()
    st_scatter.setdefault("host_ms", (time.perf_counter() - t_sc) * 1e3)
    st_scatter.setdefault("device_ms", st_scatter["host_ms"])
    scatter_updated = m.snapshot_count_updated(0) if args.full else None

    # ---- pre-stage every step's input in HBM
    nsteps = args.warmup + args.steps
    staged = []
    for _ in range(nsteps):
        new, old = w.next_step()
        new, old = new + box_lo.astype(np.int32), old + box_lo.astype(np.int32)
        hits = dev_batch(new, np.ones(len(new), np.int32))
        both = dev_batch(np.concatenate([new, old]), np.concatenate([np.ones(len(new), np.int32), np.zeros(len(old), np.int32)]))
        staged.append((hits, both))
    torch.cuda.synchronize()

    def step(k, account=False):
        hits, both = staged[k]
        observe(hits)
        top.UpdateOccupancy(True)
        observe(hits)
        top.UpdateOccupancy(True)
        observe(both)
        top.UpdateOccupancy(True)
        if account:
            m.snapshot_save(2)
        t_up = time.perf_counter()
        st = top.UpdateESDF()
        st.setdefault("host_ms", (time.perf_counter() - t_up) * 1e3)
        st.setdefault("device_ms", st["host_ms"])
        st.setdefault("relax_launches", st.get("rounds", 0))
        if account:
            st["updated"] = m.snapshot_count_updated(2)
        return st

    for k in range(args.warmup):
        step(k)
    m.snapshot_save(1)

    # ---- timed region: exactly K steps
    m.synchronize()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    timed = [step(args.warmup + k) for k in range(args.steps)]
    m.synchronize()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs:   # the field the last timed step left, before the replay below touches the map
        dump_outputs(args.dump_outputs, m, box_lo, G, rank if world > 1 else None)

    # ---- untimed accounting replay of the same K steps
    m.snapshot_restore(1)
    replay = [step(args.warmup + k, account=True) for k in range(args.steps)]
    updated = [r["updated"] for r in replay]
    total_updated = float(sum(updated))
    if dist:
        t = torch.tensor([total_updated], device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        total_updated = float(t.item())

    # ---- self-check of the run (every rank): sampled owned voxels against a k-d tree over the GLOBAL obstacle list --
    # what makes an N > 1 line evidence, not just a number (the field now is the one the K timed steps produced)
    verify = None
    if args.full and args.verify_samples > 0 and args.unobserved <= 0:   # (a partially observed map is not the exact transform: SURVEY.md 7.3-B)
        # the occupied set as the map holds it (the workload's own list is not it: a voxel that left and was drawn again
        # carries more log-odds than a fresh one and survives the single miss that frees the others)
        mine = np.ascontiguousarray(m.GetOccupiedVoxels(), dtype=np.int32)
        if dist:
            cnt = torch.tensor([len(mine)], device=cdev, dtype=torch.int64)
            cnts = [torch.zeros_like(cnt) for _ in range(world)]
            dist.all_gather(cnts, cnt)
            cap = int(max(int(c.item()) for c in cnts))
            pad = np.zeros((cap, 3), np.int32)
            pad[: len(mine)] = mine
            parts = [torch.empty((cap, 3), dtype=torch.int32, device=cdev) for _ in range(world)]
            dist.all_gather(parts, torch.from_numpy(pad).to(cdev))
            everything = np.concatenate([p_.cpu().numpy()[: int(c.item())] for p_, c in zip(parts, cnts)])
        else:
            everything = mine
        gext = G * (max(layout) if sharded_map is not None else 1)

        def query_d2(v):
            d = m.GetDistance(v)
            return np.where(d >= 10000.0, 0x7FFFFFFF, np.rint((d / res) ** 2)).astype(np.int64)
        t_v = time.perf_counter()
        sampled, bad = verify_against_kdtree(query_d2, box_lo, (G, G, G), everything, args.verify_samples, 777 + rank, gext > 1024)
        nranks_rccl, rank_rccl = sharded_map.comm_info() if sharded_map is not None else (0, 0)
        tv = torch.tensor([sampled, bad, 1, nranks_rccl], device=cdev, dtype=torch.float64)
        if dist:
            tmax = tv.clone()
            dist.all_reduce(tv, op=dist.ReduceOp.SUM)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            nranks_rccl = int(tmax[3].item())
        if sharded_map is not None and args.backend == "nccl" and world > 1 and nranks_rccl != world:
            raise SystemExit(f"bench.py --gpus {world}: the RCCL communicator of the shard group reports {nranks_rccl} ranks -- "
                             "not the protocol this line is meant to measure")
        verify = {"sampled": int(tv[0].item()), "mismatches": int(tv[1].item()), "ranks_reporting": int(tv[2].item()),
                  "ranks_seen_by_rccl": nranks_rccl, "global_obstacles": int(len(everything)),
                  "method": "exact nearest obstacle (scipy cKDTree over the all-gathered global obstacle list, d^2 recomputed in "
                            "integers); a third of the samples within 3 voxels of the owned box's faces",
                  "seconds": time.perf_counter() - t_v}

    if args.full and args.verify_samples > 0 and args.unobserved > 0:
        # A partially observed map is not the exact transform: what CAN be checked on every sampled voxel is the
        # lower bound -- no propagated distance is smaller than the distance to the nearest obstacle -- and how many of them
        # reach it; the full-size comparison with the reference is the committed envelope (parity, below).
        from scipy.spatial import cKDTree
        rng = np.random.RandomState(777)
        v = (rng.rand(args.verify_samples, 3) * G).astype(np.int64)
        obs_list = np.ascontiguousarray(m.GetOccupiedVoxels(), dtype=np.int64)
        _, nn = cKDTree(obs_list.astype(np.float64)).query(v.astype(np.float64), k=4)
        exact = ((v[:, None, :] - obs_list[nn]) ** 2).sum(-1).min(1)
        d = m.GetDistance(v.astype(np.int32))
        got = np.where(d >= 10000.0, 0x7FFFFFFF, np.rint((d / res) ** 2)).astype(np.int64)
        seen = got != 0x7FFFFFFF   # (GetDistance reads +10000 on a never-observed voxel and on one no obstacle has reached, src/ESDFMap.cpp:477-479)
        verify = {"sampled": int(len(v)), "never_observed_or_unreached": int((~seen).sum()),
                  "closer_than_the_nearest_obstacle": int((seen & (got < exact)).sum()),
                  "equal_to_the_nearest_obstacle": int((seen & (got == exact)).sum()),
                  "farther_than_the_nearest_obstacle": int((seen & (got > exact)).sum()),
                  "method": "sampled voxels against the exact nearest obstacle (scipy cKDTree over the map's occupied voxels): on a partially "
                            "observed map a distance may be LARGER (the shadows of the unobserved space, obstacles hidden in it) but never "
                            "smaller; the voxel-by-voxel comparison with the reference is `parity`"}
    if rank == 0:
        # HBM bytes per launch of the dominant kernel come from rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE cannot be
        # read from inside the process); the newest committed summary of tools/pmc_traffic.py is quoted here.
        traffic, traffic_src = None, None
        all_bulk = all(int(s.get("bulk", 0)) for s in timed)
        try:
            all_cells = all(int(s.get("cells", 0)) for s in timed)
            tag = "pmc_traffic_cells" if all_cells else "pmc_traffic_ft" if all_bulk else "pmc_traffic_k_relax_q"
            if any(int(s.get("masked", 0)) for s in timed):
                tag = "pmc_traffic_masked"   # (no such collection: the cell transform's traffic is not the masked transform's)
            cands = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if tag in f and f.endswith(".json"))
            if cands and world == 1 and args.scene == "scatter" and G == 512:
                tj = json.load(open(os.path.join(ROOT, "profiles", cands[-1])))
                traffic = tj["hbm_bytes_per_launch"]
                traffic_src = (f"profiles/{cands[-1]} ({tj['kernel']}, {tj['command']}); NOT measured in this run: counters "
                               f"collected at commit {tj.get('commit', 'unrecorded (round 2)')}")
        except Exception:
            pass
        relax_ms = sum(s["relax_ms"] for s in timed)
        launches = sum(s["relax_launches"] for s in timed)
        my_updated = float(sum(updated))
        achieved = my_updated * ALGO_BYTES_PER_UPDATED_VOXEL / (relax_ms * 1e-3) / 1e9 if relax_ms > 0 else 0.0
        call_p50_ms = statistics.median(s["host_ms"] for s in timed)
        call_achieved = my_updated / args.steps * ALGO_BYTES_PER_UPDATED_VOXEL / (call_p50_ms * 1e-3) / 1e9
        n_bulk = sum(int(s.get("bulk", 0)) for s in timed)
        n_cells = sum(int(s.get("cells", 0)) for s in timed)
        engine_steps = {"cells": n_cells, "envelope": n_bulk - n_cells, "levels": sum(int(s.get("levels", 0)) for s in timed),
                        "cell_transform_attempts_that_failed": sum(1 for s in timed if int(s.get("nn_failed", 0)) > 0)}
        engine_steps["rounds"] = len(timed) - n_bulk - engine_steps["levels"]
        engine_steps["masked"] = sum(int(s.get("masked", 0)) for s in timed)
        engine_steps["cells_incremental"] = sum(int(s.get("nn_incremental", 0)) for s in timed)
        engine_steps["cells_served_by_brute_force_per_update"] = statistics.mean(int(s.get("nn_brute_cells", 0)) for s in timed)
        # why the updates took the path they took (fiesta_hip_stats.path_notes): note -> timed steps that carried it
        engine_steps["path_notes"] = {w: sum(1 for s in timed if w in s.get("why", ())) for w in sorted({w for s in timed for w in s.get("why", ())})}
        if n_bulk == len(timed) and 0 < n_cells < len(timed):
            # a mix of the two transforms (a cell transform that met a cell it could not serve hands that update -- and the next
            # few eligible ones -- to the envelope passes): the phases below describe the majority, the counts say so
            major = [s for s in timed if bool(s.get("cells")) == (2 * n_cells >= len(timed))]
            n_cells = len(major) if major[0].get("cells") else 0
            phase_src = major
        else:
            phase_src = timed
        if n_bulk == len(timed) and n_cells == len(phase_src) and n_cells > 0:
            kernel = "k_nn_cells + k_nn_lists + k_nn_fill (cell transform: every kernel of UpdateESDF)"
            phases = {k: statistics.median(s[k] for s in phase_src) for k in ("nn_cells_ms", "nn_lists_ms", "nn_fill_ms")}
            if all(int(s.get("masked", 0)) for s in phase_src):   # a partially observed map: + certificate and repair
                kernel = "k_nn_cells + k_nn_lists + k_nn_fill + k_mask_certify + k_repair_* (masked cell transform: every kernel of UpdateESDF)"
                phases.update({k: statistics.median(s[k] for s in phase_src) for k in ("mask_certify_ms", "mask_repair_ms")})
                phases.update({k: statistics.median(s[k] for s in phase_src) for k in ("mask_uncertified", "mask_iterations", "mask_walks", "mask_quads")})
            # the dominant kernel on ITS OWN bytes: k_nn_fill writes 4 B per voxel of the grid and reads only the cells' lists
            own = float(G) ** 3 * 4.0
            dominant = {"kernel": "k_nn_fill", "ms": phases["nn_fill_ms"], "own_bytes": own, "own_bytes_what": "4 B written per grid voxel",
                        "achieved_GBs": own / (phases["nn_fill_ms"] * 1e-3) / 1e9,
                        "frac": own / (phases["nn_fill_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "list_entries_per_cell": statistics.mean(s["nn_entries"] for s in phase_src) / (math.ceil(G / 8) ** 3)}
            overflow = None
        elif n_bulk == len(timed):
            kernel = "k_ft_rows + k_ft_plane + k_ft_x (bulk feature transform: every kernel of UpdateESDF)"
            phases = {k: statistics.median(s[k] for s in phase_src) for k in ("ft_rows_ms", "ft_plane_ms", "ft_x_ms")}
            # the dominant kernel on ITS OWN bytes: pass B reads 4 B and writes 4 B per voxel of the grid
            own = float(G) ** 3 * 8.0
            dominant = {"kernel": "k_ft_x", "ms": phases["ft_x_ms"], "own_bytes": own, "own_bytes_what": "4 B read + 4 B written per grid voxel",
                        "achieved_GBs": own / (phases["ft_x_ms"] * 1e-3) / 1e9,
                        "frac": own / (phases["ft_x_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
            overflow = [int(sum(s["ft_overflow"][k] for s in timed)) for k in range(6)]
        else:
            n_lv = sum(int(s.get("levels", 0)) for s in timed)
            kernel = "k_level_run / k_level_pull + k_level_push (level engine)" if n_lv == len(timed) else "k_relax_q (frontier rounds)"
            phases, dominant, overflow = None, None, None
        out = {
            "metric": "esdf_updated_voxels_per_sec",
            "value": total_updated / elapsed,
            "unit": "voxels/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic",
            "config": {
                "workload": f"{('C2' if G == 512 else 'C2 shape at another size') if world == 1 else 'C5 shape (per rank)'}: {G}^3 dense-array grid @0.1 m {'fully observed' if args.unobserved <= 0 else f'PARTIALLY observed ({args.unobserved:.0%} of its 32^3-voxel blocks never observed)'}, {args.obstacles} "
                            f"{'scattered' if args.scene == 'scatter' else 'surface (3 planes + 20 spheres)'} obstacle voxels, "
                            f"per step a {args.obstacles}-voxel delta = {args.obstacles // 2} inserts + {args.obstacles // 2} deletes "
                            "landing in one UpdateESDF (ingest: 3 SetOccupancy+UpdateOccupancy cycles, inputs resident in HBM)",
                "grid": [G, G, G], "delta_voxels": args.obstacles,
                "parallelism": "single GPU" if world == 1 else (
                    f"{world} independent map replicas (one per GPU)" if sharded_map is None else
                    f"one map of {'x'.join(str(G * l) for l in layout)} voxels sharded {'x'.join(map(str, layout))} over {world} GPUs "
                    f"({G}^3 owned per GPU + 2-voxel ghost layer; RCCL ghost exchange + transition all-gather, "
                    f"{statistics.mean(s_['sweeps'] for s_ in timed):.1f} ghost sweeps per update)"),
                "update_engine": args.engine, "unobserved_block_fraction": args.unobserved,
                "protocol": None if sharded_map is None else sharded_map.protocol,
            },
            "update_esdf_p50_ms": statistics.median(s["host_ms"] for s in timed),
            "update_esdf_device_p50_ms": statistics.median(s["device_ms"] for s in timed),
            "updated_voxels_per_step": my_updated / args.steps,
            "update_esdf_voxels_per_sec": my_updated / (sum(s["host_ms"] for s in timed) * 1e-3),
            "rounds_per_update": statistics.mean(s["rounds"] for s in timed),
            # frac: algorithmic bytes of one UpdateESDF / the CALL's p50 (host wall time of fiesta_hip_update_esdf: every
            # kernel, every gap between them, the final synchronisation) -- VERDICT r3: not the sum of the kernels' own events,
            # which flatters it; that number stays as frac_kernels_only
            "roofline": {
                "bound": "hbm", "kernel": kernel,
                "achieved": call_achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": call_achieved / HBM_PEAK_GBS,
                "frac_definition": "16 B x updated voxels per UpdateESDF / update_esdf_p50_ms / 8 TB/s",
                "achieved_kernels_only": achieved, "frac_kernels_only": achieved / HBM_PEAK_GBS,
                "frac_on_ms_per_step": my_updated / args.steps * ALGO_BYTES_PER_UPDATED_VOXEL / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                "traffic": traffic, "traffic_unit": "bytes/launch", "traffic_source": traffic_src,
                "launches": launches, "avg_launch_us": relax_ms * 1e3 / max(1, launches),
                "algorithmic_bytes_per_launch": my_updated * ALGO_BYTES_PER_UPDATED_VOXEL / max(1, launches),
                "frac_of_measured_copy_6.29TBs": call_achieved / 6290.0,
                "phases_p50_ms": phases, "dominant_kernel": dominant, "ring_overflows": overflow, "engine_steps": engine_steps,
            },
            "revision": revision(),
        }
        if args.full:
            out["scatter_full_update"] = {"updated_voxels": scatter_updated, "device_ms": st_scatter["device_ms"],
                                          "host_ms": st_scatter["host_ms"], "rounds": st_scatter["rounds"],
                                          "relax_ms": st_scatter["relax_ms"],
                                          "voxels_per_sec": scatter_updated / (st_scatter["host_ms"] * 1e-3),
                                          "roofline_frac": scatter_updated * 16 / (st_scatter["relax_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
            out["verify"] = verify
            out["parity"] = parity_summary(args, G, world) if args.unobserved <= 0 else parity_partial(args, G, world, timed)
        if args.full and world == 1 and not args.no_cpu_baseline:
            if sharded_map is None:
                m.close()   # (the GPU side is finished; the CPU legs get the host to themselves)
            out["cpu_baseline"] = run_cpu_baseline(args)
            # ... and the SAME step at the SAME size in the same run on this box: the verbatim reference, one core
            from oracle import pyoracle
            full_ok = (not args.no_cpu_full and pyoracle.available("ref", "array") and G <= 512 and free_host_gb() > 0.09 * (G / 512.0) ** 3 * 100)
            if full_ok:
                full = run_cpu_baseline(args, grid=G)
                out["cpu_baseline"]["sample_value"] = out["cpu_baseline"]["value"]
                out["cpu_baseline"]["sample"] = "SAME box, SAME run, SAME size: " + full["sample"] + " [bounded sample beside it: " + out["cpu_baseline"]["sample"] + "]"
                for k in ("value", "update_esdf_s", "updated_voxels", "wall_s"):
                    out["cpu_baseline"][k] = full[k]
                out["cpu_baseline"]["full_size"] = True
            else:
                out["cpu_baseline"]["full_size"] = False
                try:  # the one-off full-size run of the reference in the build container (tests/golden/make_golden_c2.py)
                    full = json.load(open(os.path.join(ROOT, "profiles", "r02_cpu_512.json")))[args.scene]["steady_state_step"]
                    out["cpu_baseline"]["full_size_512_other_box"] = {"voxels_per_sec": full["voxels_per_sec"], "seconds": full["seconds"],
                                                                      "updated_voxels": full["updated_voxels"], "source": "profiles/r02_cpu_512.json"}
                except Exception:
                    pass
        print(json.dumps(out), flush=True)
    m.close()
    if dist:
        dist.barrier()
        dist.destroy_process_group()


def dump_outputs(path, m, box_lo, G, rank=None):
    """--dump-outputs: what a caller reads from the map after the last timed step, for comparing two builds output for output.
    The whole field is 4 B x G^3 (512 MB at 512^3), so a fixed seeded sample of 2^20 voxels of the owned box (their coordinates,
    GetDistance in metres, GetOccupancy) and GetSlice of the middle z-plane (single map, up to 16 MB); about 26 MB at 512^3.
    With --gpus N every rank writes its own box, the names suffixed _rank<r>."""
    os.makedirs(path, exist_ok=True)
    lo = np.asarray(box_lo, np.int64)
    v = (lo + np.random.RandomState(4711).randint(0, G, (1 << 20, 3))).astype(np.int32)
    arrays = {"sample_voxels": v.astype(np.float32),
              "sample_distance": np.asarray(m.GetDistance(v), np.float64),
              "sample_occupancy": np.asarray(m.GetOccupancy(v)).astype(np.float32)}
    if rank is None and G * G * 8 <= 16 << 20:
        arrays["mid_plane_distance"] = np.asarray(m.GetSlice(G // 2), np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ("" if rank is None else f"_rank{rank}") + ".npy"), a)


def parity_partial(args, G, world, timed):
    """C2-partial: the reference's result depends on its queue order there, so the pin is the ENVELOPE of K + 1 runs of the verbatim
    reference on these very inputs at this very size (tests/golden/make_golden_c2_partial.py), which
    tests/test_gpu_masked.py::test_masked_c2_partial_against_the_committed_envelope compares every voxel of two checkpoints with."""
    masked = sum(int(s.get("masked", 0)) for s in timed)
    out = {"engine": f"masked transform on {masked} of {len(timed)} timed updates" if masked else "frontier rounds / level engine",
           "contract": "closer / farther than every run of the reference on at most max(voxels its own runs disagree on, 1e-4 of the finite "
                       "voxels) (masked transform; the frontier rounds' allowance is 0.5 %, tests/scenarios.py: assert_envelope)"}
    try:
        d = np.load(os.path.join(ROOT, "tests", "golden", f"c2_partial_{G}_envelope.npz"))
        if world != 1 or abs(args.unobserved - float(d["unobserved"])) > 1e-9 or args.obstacles != int(round(50000 * (G / 512.0) ** 3)) or \
                args.delta is not None or args.scene != "scatter":
            raise ValueError("the committed envelope covers bench.py --unobserved 0.27 at the default obstacle count only")
        out["pinned_by"] = (f"tests/golden/c2_partial_{G}_envelope.npz: {int(d['runs'])} runs of the verbatim reference on these inputs, all "
                            f"{G ** 3} voxels of both checkpoints (test_masked_c2_partial_against_the_committed_envelope)")
        out["reference_runs_disagree_on"] = {cp: int(d[f"{cp}/disagree"]) for cp in ("scatter", "step")}
        out["reference_differs_from_the_exact_transform_on"] = {cp: int(len(d[f"{cp}/exc_idx"])) for cp in ("scatter", "step")}
        out["finite_voxels"] = {cp: int(d[f"{cp}/finite"]) for cp in ("scatter", "step")}
    except Exception as e:  # noqa: BLE001
        out["pinned_by"] = None
        out["note"] = repr(e)
    return out


def parity_summary(args, G, world):
    """What pins the distances of THIS workload to the reference (tests/test_gpu_full_size.py): at the headline size the
    verbatim reference ran once on these very inputs (tests/golden/make_golden_c2.py); its per-x-slab CRC32s of d^2 are
    reproduced by the GPU field except on the listed voxels, where the reference holds an artefact of its own insert order
    (a larger distance, by at most half a voxel) and the GPU the exact transform."""
    if world != 1 or G != 512 or args.obstacles != 50000 or args.delta is not None:
        return {"pinned_by": "sampled k-d tree check of this run (verify); the full-size digest covers the 512^3 / 50k workload only"}
    try:
        d = np.load(os.path.join(ROOT, "tests", "golden", f"c2_512_{args.scene}_digest.npz"))
        n = int(np.prod(d["grid"]))
        return {"pinned_by": f"tests/golden/c2_512_{args.scene}_digest.npz (verbatim reference, all {n} voxels of both checkpoints, "
                             "test_config2_512cube_matches_reference_digest)",
                "exact_voxels": {"scatter_insert": n - int(len(d["scatter/exc_idx"])), "steady_state_step": n - int(len(d["step/exc_idx"]))},
                "reference_order_artefacts": {"scatter_insert": int(len(d["scatter/exc_idx"])), "steady_state_step": int(len(d["step/exc_idx"]))},
                "artefact_note": "voxels where the reference itself deviates from the exact transform depending on its insert order "
                                 "(tests/test_oracle_order_sensitivity.py); the GPU holds the exact value there"}
    except Exception as e:  # noqa: BLE001
        return {"pinned_by": None, "error": repr(e)}


if __name__ == "__main__":
    main()
