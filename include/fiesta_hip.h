/* fiesta_hip.h -- the drop-in boundary of the MI355X-native incremental ESDF engine.
 *
 * A plain C ABI (no C++ types, no HIP types, no torch types) exported by fiesta_amd/libfiesta_hip.so.
 * The reference (HKUST-Aerial-Robotics/FIESTA) has no FFI/plugin layer: its operator API for this path IS
 * the public section of `class fiesta::ESDFMap` (include/ESDFMap.h:111-166) plus the free function
 * `Raycast` (include/raycast.h:16-18) and the per-frame driver `Fiesta::RaycastProcess`
 * (include/Fiesta.h:194-278). Every entry point below names the reference interface it replaces; the C++
 * facade include/fiesta/ESDFMap.h re-creates the reference's class on top of these calls, so a maintainer
 * swaps the implementation file, not the callers.
 *
 * Conventions
 *   - every function returns an int status: 0 = FIESTA_HIP_OK, otherwise an error code; the message of
 *     the last failure on the calling thread is fiesta_hip_last_error(). Nothing throws across the ABI.
 *   - "vox" arrays are n x 3 int32 (x,y,z voxel coordinates), "pos" arrays are n x 3 double (metres);
 *     linear voxel index = x*Ny*Nz + y*Nz + z (src/ESDFMap.cpp:91), z fastest.
 *   - pointers are HOST pointers unless the function name ends in _dev (device pointers on the map's GPU).
 *   - one host thread drives one map (the reference is single-threaded by contract). All work of a map is
 *     ordered on one HIP stream; calls return after the device work they need has completed unless stated.
 *   - there is NO CPU fallback: if no gfx950 device is usable, fiesta_hip_create fails.
 */
#ifndef FIESTA_HIP_H
#define FIESTA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIESTA_HIP_OK 0
#define FIESTA_HIP_ERR_INVALID 1  /* bad argument / unsupported configuration */
#define FIESTA_HIP_ERR_DEVICE 2   /* a HIP runtime call failed */
#define FIESTA_HIP_ERR_NOMEM 3    /* device allocation failed */
#define FIESTA_HIP_ERR_STATE 4    /* call sequence error */

/* Reference sentinels (src/ESDFMap.cpp:181-182). */
#define FIESTA_HIP_UNDEFINED (-10000)
#define FIESTA_HIP_INFINITY 10000

#define FIESTA_HIP_MODE_ARRAY 0 /* ESDFMap(origin,res,map_size)  src/ESDFMap.cpp:171  */
#define FIESTA_HIP_MODE_HASH 1  /* ESDFMap(origin,res,reserve)   src/ESDFMap.cpp:130  (HASH_TABLE+BLOCK+BITWISE) */

typedef struct fiesta_hip_map fiesta_hip_map; /* opaque */

typedef struct fiesta_hip_config {
  int32_t mode;         /* FIESTA_HIP_MODE_* (array vs hash is a RUNTIME choice here, a macro upstream) */
  int32_t device;       /* HIP device ordinal */
  double origin[3];     /* l_cornor_ / origin_ */
  double resolution;    /* metres per voxel */
  double map_size[3];   /* array mode: grid = ceil(map_size/resolution) (src/ESDFMap.cpp:175-176) */
  int32_t reserve_size; /* hash mode: initial voxel reserve (src/ESDFMap.cpp:141-145) */
  int32_t update_engine; /* UpdateESDF engine: 0 = chosen per update (default), 1 = frontier rounds only, 2 = bulk
                            feature transform whenever the map is fully observed, 3 = level engine for
                            every update its lists can hold, 4 = as 2 with the envelope passes only, 5 = as 2
                            with the cell transform wherever it applies (2 chooses between the two), 6 = on
                            partially observed maps the masked transform for every update the map's history allows it for
                            (0, 2, 4 and 5 take it for deltas too large for the level engine), else as 0; on
                            fully observed maps the distances do not depend on it */
  /* Spatial sharding. A map may be one shard of a larger global grid: it owns the global
   * voxel box [shard_lo, shard_lo + grid) and stores closest-obstacle ids in GLOBAL coordinates. For an
   * unsharded map leave these zero. */
  int32_t shard_lo[3];
  int32_t global_grid[3];
} fiesta_hip_config;

/* Counters of one UpdateESDF; the reference only prints its counters (src/ESDFMap.cpp:277,394). */
typedef struct fiesta_hip_stats {
  int64_t inserted;      /* insert-queue length at entry */
  int64_t deleted;       /* delete-queue length at entry */
  int64_t invalidated;   /* voxels reset because their closest obstacle vanished */
  int64_t rounds;        /* level-synchronous frontier rounds */
  int64_t tile_visits;   /* tiles relaxed, summed over rounds */
  int64_t sweeps;        /* in-LDS relaxation sweeps, summed over tile visits */
  int64_t voxel_writes;  /* voxel states written back to HBM (a voxel may be written in several rounds) */
  double device_ms;      /* HIP-event time from first to last kernel of the update */
  double host_ms;        /* wall time of the call */
  double relax_ms;       /* sum of the HIP-event durations of the relaxation launches (k_relax) */
  int64_t relax_launches;
  int64_t prof[8];       /* engine profiling counters (only with FIESTA_HIP_PROF=1 in the environment) */
  int64_t bulk;          /* 1: this update ran the bulk feature transform (rounds == 0), relax_ms = its kernels */
  double ft_rows_ms, ft_plane_ms, ft_x_ms; /* bulk path: HIP-event time of k_ft_rows / pass A / pass B */
  int64_t ft_overflow[6];/* bulk path: column groups that moved ring entries to the backing store (deques deeper than
                            their LDS ring): [0] pass A, [3] pass B; the other entries are unused (0) */
  int64_t observed_voxels, occupied_voxels; /* map totals at entry (array mode): observed at least once / Exist() */
  int64_t ft_max_d2;     /* bulk path on a shard: largest squared distance written (decides whether the margin sufficed) */
  int64_t dropped_observations; /* hash mode, cumulative: observations that fell outside the window even after it moved
                                   to their batch (a single batch or frame spanning more than 1024 voxels on an axis,
                                   non-finite positions) and were ignored -- a non-zero value means lost map data */
  int64_t levels;        /* 1: this update ran the level engine from start to end (rounds = its levels, one per layer of the
                            reference's FIFO); 0 with bulk == 0: the frontier rounds ran (possibly after the level engine's
                            lists overflowed) */
  int64_t grid_levels;   /* of `rounds` with levels == 1: levels that ran on many CUs (k_level_grid) rather than one */
  int64_t cells;         /* with bulk == 1: the transform was the cell transform (nn_kernels.hpp: per-cell obstacle lists), not
                            the envelope passes */
  double nn_cells_ms, nn_lists_ms, nn_fill_ms; /* cell transform: HIP-event time of k_nn_cells / k_nn_lists / k_nn_fill */
  int64_t nn_entries;    /* cell transform: list entries over all cells */
  int64_t nn_failed;     /* cells that got no list when the cell transform was tried (> 0: the envelope passes served the
                            update instead, cells == 0).  Once a cell has failed the launch stops early: nn_failed and
                            nn_entries are then LOWER BOUNDS (how many work-groups were already running depends on scheduling) */
  int64_t nn_incremental; /* with cells == 1: only the cells whose search window held a changed voxel were redone (the lists of the
                             last transform were still valid), nn_dirty_cells of them */
  int64_t nn_dirty_cells;
  int64_t nn_brute_cells; /* with cells == 1: cells that got no list (nothing within reach, more candidates than a list holds) and were
                             served one by one by brute force instead of failing the transform (r06) */
  int64_t masked;        /* with bulk == 1: a PARTIALLY observed map -- the transform ran masked (mask_kernels.hpp): its result kept
                            on the observed voxels whose segment to their obstacle is observed, the others repaired by pulls */
  int64_t mask_uncertified, mask_iterations, mask_walks, mask_quads; /* masked: voxels under repair, repair iterations, segment
                                                                        walks, quads (8 x 8 x 32 voxels) under repair */
  double mask_certify_ms, mask_repair_ms;               /* masked: HIP-event time of k_mask_certify / of the repair launches */
  int64_t path_notes;    /* dense-array maps: WHY this update took the path it took -- FIESTA_HIP_NOTE_* bits (0: nothing stood in the
                            way of the exact transform, or there was nothing to do) */
} fiesta_hip_stats;

/* fiesta_hip_stats.path_notes: the gates and back-offs that decided an UpdateESDF's engine (each is a place where the latency of a
   call changes by a factor; `bulk`, `cells`, `masked`, `levels`, `rounds` say WHAT ran, these say why) */
#define FIESTA_HIP_NOTE_PARTLY_OBSERVED 0x0001    /* voxels never observed: the exact transforms are gated (src/ESDFMap.cpp:345,382) */
#define FIESTA_HIP_NOTE_PARTIAL_WINDOW 0x0002     /* the update window is not the whole array (SetUpdateRange) */
#define FIESTA_HIP_NOTE_WINDOW_HISTORY 0x0004     /* an earlier update ran under a partial window: the field depends on that history */
#define FIESTA_HIP_NOTE_LATE_OBSERVATION 0x0008   /* voxels first observed free while obstacles stood still wait for a wave (:246-249) */
#define FIESTA_HIP_NOTE_FIRST_WAVE_PENDING 0x0010 /* ... the same on a fully observed map: the exact transform waits for them too */
#define FIESTA_HIP_NOTE_DENSITY 0x0020            /* obstacle density outside the cell transform's range: envelope passes */
#define FIESTA_HIP_NOTE_CELLS_BACKOFF 0x0040      /* the cell transform failed or lost recently and is not retried yet */
#define FIESTA_HIP_NOTE_CELLS_FAILED 0x0080       /* the cell transform was tried, a cell got no list: the envelope passes served the update */
#define FIESTA_HIP_NOTE_INCREMENTAL_REDONE 0x0100 /* the incremental cell transform failed and the same call ran it in full */
#define FIESTA_HIP_NOTE_SMALL_DELTA 0x0200        /* too few changes for a whole-grid transform to pay: level engine / rounds */
#define FIESTA_HIP_NOTE_MASKED_GAVE_UP 0x0400     /* the masked transform gave the update back (lists or repair outgrew their buffers) */
#define FIESTA_HIP_NOTE_LEVELS_GAVE_UP 0x0800     /* the level engine handed the update on to the rounds */
#define FIESTA_HIP_NOTE_SHARDED 0x1000            /* a shard of a larger map: level engine and masked transform excluded */
#define FIESTA_HIP_NOTE_ID_WRAP 0x2000            /* an extent beyond 1024 voxels: ids wrap, masked transform and incremental lists excluded */
#define FIESTA_HIP_NOTE_ENGINE_PINNED 0x4000      /* update_engine is not "auto" */

const char *fiesta_hip_last_error(void);
/* 100: the interface up to fiesta_hip_stats ending in path_notes; 101: fiesta_hip_path_clearance[_dev].
 * fiesta_hip_path_cost[_dev], fiesta_hip_get_frontier_voxels[_dev], fiesta_hip_ray_query[_dev], fiesta_hip_reach_field[_dev] and
 * fiesta_hip_reach_paths[_dev] came later without a new number, and so did fiesta_hip_cluster_voxels[_dev],
 * fiesta_hip_view_coverage[_dev], fiesta_hip_reach_matrix[_dev], fiesta_hip_site_tour[_dev], fiesta_hip_free_boxes[_dev],
 * fiesta_hip_path_corridor[_dev], fiesta_hip_path_refine[_dev], fiesta_hip_corridor_bounds[_dev],
 * fiesta_hip_split_clusters[_dev], fiesta_hip_leg_paths[_dev], fiesta_hip_path_timing[_dev], fiesta_hip_get_skeleton_voxels[_dev],
 * fiesta_hip_body_query[_dev], fiesta_hip_articulated_query[_dev] and fiesta_hip_body_sweep[_dev]: detect them by symbol lookup
 * (dlsym). */
int fiesta_hip_version(void);
/* Number of usable gfx950 devices (0 on a box without a GPU; never an error). */
int fiesta_hip_device_count(void);

/* ---- life cycle: ESDFMap::ESDFMap / ~ESDFMap (include/ESDFMap.h:112-121) ---- */
int fiesta_hip_create(const fiesta_hip_config *cfg, fiesta_hip_map **out);
int fiesta_hip_destroy(fiesta_hip_map *m);
/* array mode: grid_size_ and grid_total_size_ (include/ESDFMap.h:78,115); hash mode: allocated voxels. */
int fiesta_hip_grid_size(fiesta_hip_map *m, int32_t out[3]);
int fiesta_hip_grid_total_size(fiesta_hip_map *m, int64_t *out);
/* What SetOccupancy(Vector3i) returns for each voxel WITHOUT observing it (host arithmetic only): the reference's
 * callers test the value against -10000 and use it as the per-frame de-duplication key (include/Fiesta.h:221-232,
 * 253-273), so it must identify the voxel.  Array mode: Vox2Idx = x*Ny*Nz + y*Nz + z (src/ESDFMap.cpp:84-93; no range
 * check, like the reference).  Hash mode: the reference returns an allocation-order slot number; here the voxel's map
 * coordinates modulo 1024, packed (30 bits, never negative): unique among the voxels of one window position, which is
 * all a frame can observe. */
int fiesta_hip_voxel_key(fiesta_hip_map *m, const int32_t *vox, int64_t n, int32_t *out);

/* ---- hash-block map: the moving window ----
 * The hash-block map is unbounded like the reference's (src/ESDFMap.cpp:46-48: PosInMap/VoxInMap are always true); the
 * part of it that queries, observations and UpdateESDF work on is a WINDOW of 1024^3 voxels that starts centred on map
 * voxel (0,0,0) and FOLLOWS THE OBSERVATIONS: a SetOccupancy batch or ray-cast frame whose bounding box does not fit
 * the window recentres it on that box (per axis, in whole tiles of 16 x 16 x 32 voxels).  Pages that leave the window
 * are parked -- kept, listed by fiesta_hip_download_hash, still ANSWERING every query (GetDistance, GetOccupancy,
 * GetDistWithGradTrilinear go through a map-wide page table outside the window: a planner may ask about a goal far from
 * the sensor) with the field they held when the window left, but taking no part in observations or UpdateESDF -- and
 * rejoin, with their distance field rebuilt at the next UpdateESDF, when the window returns.  Inside the window the field
 * is the ESDF of the obstacles inside the window (reach of a closest-obstacle id: 512 voxels).
 *   fiesta_hip_hash_window    origin = map voxel of the window's lowest corner; moves (nullable) = moves so far
 *   fiesta_hip_hash_recentre  move the window so that `centre` is at its middle (e.g. to query around a goal pose) */
int fiesta_hip_hash_window(fiesta_hip_map *m, int32_t origin[3], int64_t *moves);
int fiesta_hip_hash_recentre(fiesta_hip_map *m, const int32_t centre[3]);

/* ---- parameters and window ---- */
/* ESDFMap::SetParameters (src/ESDFMap.cpp:218-224). */
int fiesta_hip_set_prob_params(fiesta_hip_map *m, double p_hit, double p_miss, double p_min, double p_max,
                               double p_occ);
/* ESDFMap::SetUpdateRange (src/ESDFMap.cpp:792-810) / SetOriginalRange (:812-824). */
int fiesta_hip_set_update_range(fiesta_hip_map *m, const double min_pos[3], const double max_pos[3],
                                int new_vec);
int fiesta_hip_set_original_range(fiesta_hip_map *m);
/* fiesta_hip_config.update_engine, changed on a live map (takes effect with the next UpdateESDF).  Array maps take 0-6;
 * hash-block maps take 0, 1 and 3 (2, 4, 5 and 6 behave as 0 there: the transforms need a dense array).  No reference
 * counterpart: the reference has one engine. */
int fiesta_hip_set_update_engine(fiesta_hip_map *m, int32_t engine);
/* Diagnostics of the last UpdateESDF the level engine served (fiesta_hip_stats.levels): for each of its first 48 levels
 * (= layers of the reference's FIFO, src/ESDFMap.cpp:339-392) the number of frontier entries (high 16 bits) and the time
 * the level took inside the one-work-group kernel in units of 10 ns (low 16 bits).  *n_levels = levels of that update
 * (may exceed 48).  No reference counterpart. */
int fiesta_hip_level_trace(fiesta_hip_map *m, uint32_t out[48], int32_t *n_levels);
/* Diagnostics of the level engine's wide levels (k_level_grid): `grid_groups` work-groups of one XCD take part
 * (0..32; 0: never launched -- wide frontiers go to the frontier rounds as before); a barrier among them waits `spin_limit`
 * polls (~1 us each) before the update is given up and repaired by the frontier rounds (0: gives up at its first barrier --
 * how the tests reach that path).  Negative values leave a setting as it is.  Defaults: 32, 262144. */
int fiesta_hip_level_tuning(fiesta_hip_map *m, int32_t grid_groups, int64_t spin_limit);

/* ---- occupancy ingest: ESDFMap::SetOccupancy x2 (src/ESDFMap.cpp:401-437), batched ----
 * Observations are applied as if SetOccupancy had been called once per entry; hit/total counters are
 * accumulated with atomics so the order inside a batch is irrelevant. ret (nullable, host) receives what
 * each individual call would have returned (the linear index, or FIESTA_HIP_UNDEFINED). */
int fiesta_hip_set_occupancy_vox(fiesta_hip_map *m, const int32_t *vox, const int32_t *occ, int64_t n,
                                 int32_t *ret);
int fiesta_hip_set_occupancy_pos(fiesta_hip_map *m, const double *pos, const int32_t *occ, int64_t n,
                                 int32_t *ret);
/* Same, inputs already resident in HBM; no return values, no host synchronisation. */
int fiesta_hip_set_occupancy_vox_dev(fiesta_hip_map *m, const int32_t *vox_dev, const int32_t *occ_dev,
                                     int64_t n);

/* SetOccupancy(Vector3i, occ) for every voxel of the inclusive box [lo, hi] (map voxel coordinates), device
 * side: the usual way to mark a whole region observed-free (the reference's callers loop over voxels). */
int fiesta_hip_set_occupancy_box(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], int32_t occ);

/* ---- ray casting: Raycast (src/raycast.cpp:56-158) + Fiesta::RaycastProcess (include/Fiesta.h:194-278) ---- */
typedef struct fiesta_hip_raycast_params {
  double min_ray_length, max_ray_length; /* parameters_.min/max_ray_length_ (src/parameters.cpp:9-10) */
  double l_cornor[3], r_cornor[3];       /* ray clipping box in metres (parameters_.l_cornor_/r_cornor_) */
  int32_t dedup;                         /* 1: per-frame de-dup of end points and free-space voxels with
                                            the reference's early ray termination made order-independent
                                            (see DESIGN.md); 0: every ray marks every voxel it crosses */
  int32_t inverse;                       /* 1: this map is the -DSIGNED_NEEDED companion inv_esdf_map_ (include/Fiesta.h:39-41,
                                            216-218, 249-251): the frame's end points are counted as FREE and the voxels
                                            the rays cross as OCCUPIED; same rays, same de-duplication.  A caller that
                                            wants the signed field keeps two maps of equal geometry, feeds every frame
                                            to both (inverse = 0 / 1), updates both, and subtracts the inverse map's
                                            distance (distance to the nearest free voxel) from the map's own */
} fiesta_hip_raycast_params;
/* One sensor frame: points are n x 3 float (sensor frame), transform the row-major 4x4 transform_,
 * origin the raycast_origin_. Equivalent to RaycastMultithread with ray_cast_num_thread_ == 0. */
int fiesta_hip_raycast_frame(fiesta_hip_map *m, const float *points, int64_t n, const double transform[16],
                             const double origin[3], const fiesta_hip_raycast_params *p);
int fiesta_hip_raycast_frame_dev(fiesta_hip_map *m, const float *points_dev, int64_t n,
                                 const double transform[16], const double origin[3],
                                 const fiesta_hip_raycast_params *p);
/* Depth-image front end (pinhole part of Fiesta::DepthConversion, include/Fiesta.h:341-351): uint16
 * millimetre depth, rows x cols, converted to sensor-frame points on the device, then ray cast. */
int fiesta_hip_raycast_depth(fiesta_hip_map *m, const uint16_t *depth, int32_t rows, int32_t cols,
                             double fx, double fy, double cx, double cy, const double transform[16],
                             const double origin[3], const fiesta_hip_raycast_params *p);
/* The same front end with the temporal depth-consistency filter of Fiesta::DepthConversion (use_depth_filter_,
 * include/Fiesta.h:352-379): a pixel casts a ray only if it lies inside the margin, its depth within [min_dist, max_dist],
 * and its re-projection into the PREVIOUS depth image agrees with the depth stored there within `tolerance`. The map
 * keeps the previous image on the device; the first image of a run (none stored yet, or reset != 0) casts nothing, as
 * upstream (image_cnt_ == 1). rel_transform = last_transform_^-1 * transform_, row-major 4x4, supplied by the caller
 * (the node has both poses). Defaults upstream: tolerance 0.1, max 10, min 0.1, margin 0 (src/parameters.cpp:38-42). */
typedef struct fiesta_hip_depth_filter {
  double tolerance, max_dist, min_dist;
  int32_t margin;
  int32_t reset;
  double rel_transform[16];
} fiesta_hip_depth_filter;
int fiesta_hip_raycast_depth_filtered(fiesta_hip_map *m, const uint16_t *depth, int32_t rows, int32_t cols, double fx,
                                      double fy, double cx, double cy, const double transform[16], const double origin[3],
                                      const fiesta_hip_raycast_params *p, const fiesta_hip_depth_filter *filter);
/* Fiesta::DepthConversion alone (array mode): the frame's point cloud to a host buffer of rows x cols x 3 floats in
 * pixel order; a pixel the filter rejects (filter nullable: none) reads NaN, NaN -- such points are skipped by the ray
 * cast like upstream's NaN points (include/Fiesta.h:202). *n_valid = points that survived. Advances the stored previous
 * image like the call above. */
int fiesta_hip_depth_conversion(fiesta_hip_map *m, const uint16_t *depth, int32_t rows, int32_t cols, double fx, double fy,
                                double cx, double cy, const fiesta_hip_depth_filter *filter, float *points_out,
                                int64_t *n_valid);
/* The free function Raycast itself, for one ray (voxel units); returns the voxel count in *n_out
 * (FIESTA_HIP_ERR_INVALID if the reference would throw: more than 1500 voxels). out is cap x 3 doubles. */
int fiesta_hip_raycast_single(const double start[3], const double end[3], const double minv[3],
                              const double maxv[3], double *out, int32_t cap, int32_t *n_out, int32_t device);

/* ---- occupancy fusion and the ESDF update ---- */
/* ESDFMap::CheckUpdate (src/ESDFMap.cpp:227-233): *out = 1 iff some voxel was observed since the last
 * UpdateOccupancy. */
int fiesta_hip_check_update(fiesta_hip_map *m, int32_t *out);
/* ESDFMap::UpdateOccupancy (src/ESDFMap.cpp:235-271). n_insert/n_delete (nullable) receive the lengths of
 * the insert and delete queues after the call, *any (nullable) the reference's bool return value. */
int fiesta_hip_update_occupancy(fiesta_hip_map *m, int32_t global_map, int64_t *n_insert, int64_t *n_delete,
                                int32_t *any);
/* ESDFMap::UpdateESDF (src/ESDFMap.cpp:273-398). stats is nullable. */
int fiesta_hip_update_esdf(fiesta_hip_map *m, fiesta_hip_stats *stats);

/* ---- queries, batched ---- */
/* ESDFMap::GetDistance(Vector3i) (src/ESDFMap.cpp:477-479); out-of-grid voxels read as +10000. */
int fiesta_hip_get_distance_vox(fiesta_hip_map *m, const int32_t *vox, int64_t n, double *out);
/* ESDFMap::GetDistance(Vector3d) (:467-475): -10000 outside the map. */
int fiesta_hip_get_distance_pos(fiesta_hip_map *m, const double *pos, int64_t n, double *out);
/* ESDFMap::GetDistWithGradTrilinear (:481-540): dist -1 outside the map; grad is n x 3. */
int fiesta_hip_get_dist_grad(fiesta_hip_map *m, const double *pos, int64_t n, double *dist, double *grad);
/* ESDFMap::GetOccupancy x2 (:452-465). */
int fiesta_hip_get_occupancy_vox(fiesta_hip_map *m, const int32_t *vox, int64_t n, int32_t *out);
int fiesta_hip_get_occupancy_pos(fiesta_hip_map *m, const double *pos, int64_t n, int32_t *out);
/* Device-resident query: pos_dev n x 3 double, dist_dev n double, grad_dev n x 3 double (nullable). */
int fiesta_hip_get_dist_grad_dev(fiesta_hip_map *m, const double *pos_dev, int64_t n, double *dist_dev,
                                 double *grad_dev);
/* The five host-pointer queries above, called with n <= 8 on an array map (what fiesta::ESDFMap::GetDistance & co. do:
 * one position per call, as the reference's callers -- planners, 10^4-10^6 calls a second, src/ESDFMap.cpp:467-540 is an
 * array read there), are answered from a host-side cache of 16^3-voxel bricks of the field: the first query into a brick
 * fetches it (one small kernel writing into pinned host memory, one synchronisation), every further one is a host read
 * with the same arithmetic, bit for bit.  UpdateOccupancy, UpdateESDF, a restore or load and the ghost exchange of a
 * shard invalidate the cache.  *fetches = bricks fetched so far (a statistic for tests and the benchmark). */
int fiesta_hip_host_cache_fetches(fiesta_hip_map *m, int64_t *fetches);

/* ---- path clearance, batched: minimum distance and first contact along polylines ----
 * No reference counterpart: the reference's callers loop over GetDistWithGradTrilinear (src/ESDFMap.cpp:481-540) sample by
 * sample.  Since fiesta_hip_version() 101.
 * Input: n_paths polylines over n_waypoints waypoints (n_waypoints x 3 double, metres) in CSR form -- path p is
 * waypoints[offsets[p] .. offsets[p+1]-1]; offsets holds n_paths + 1 int64 entries, offsets[0] = 0, non-decreasing,
 * offsets[n_paths] = n_waypoints.  step: the sample spacing in metres, finite and > 0.  margin: metres, not NaN (+-inf allowed).
 *
 * The sample rule -- exact in f64, identical on the device, on the host, in fiesta_amd.path_samples (numpy) and in
 * fiesta::ESDFMap::PathSample (C++); the library is built with -ffp-contract=off, numpy does not contract either:
 *   for each segment a = w[i], b = w[i+1] of a path, in order:
 *     d = b - a, per component;  L = sqrt(d0*d0 + d1*d1 + d2*d2), evaluated left to right;  S = max(1, (int64)ceil(L / step));
 *     the samples are a[c] + d[c] * ((double)k / (double)S) for k = 0 .. S-1 (a zero-length segment: one sample, at a);
 *   after the last segment one final sample: the last waypoint itself (a path of one waypoint has exactly that sample).
 *   Sample indices run in this order from 0 to n_samples - 1.
 * The value of a sample is bit for bit what fiesta_hip_get_dist_grad returns at that position on the same map (dense maps, a
 * single shard, hash-block maps): -1 outside a dense map (PosInMap), unobserved corners read +10000.
 *
 * Outputs, one per path; every pointer of the result is nullable:
 *   min_dist             the minimum sample value
 *   min_index            the smallest sample index that attains it
 *   min_pos (x3)         that sample's position by the rule
 *   min_grad (x3)        fiesta_hip_get_dist_grad's gradient at that sample, bit for bit
 *   first_below          the smallest sample index whose value is < margin (strictly), -1 if there is none.  A path that leaves a
 *                        dense map "contacts" where it leaves (value -1): what the point query tells a planner there too.  A
 *                        sphere robot of radius r asks with margin = r.
 *   first_below_pos (x3) that sample's position, NaN if there is none
 *   n_samples            the path's sample count
 * Special paths:
 *   empty (offsets[p] == offsets[p+1]): n_samples 0, min_dist +inf, indices -1, positions NaN, gradient 0;
 *   invalid -- a non-finite waypoint, a segment with L / step > 2^24, or (device variant only) offsets out of order or out of
 *   range: n_samples -1, min_dist NaN, indices -1, positions NaN, gradient 0.  The other paths are unaffected.  On the device
 *   "out of order or out of range" means offsets[p+1] < offsets[p], a range outside [0, n_waypoints], or offsets[p] below an
 *   earlier entry that lies inside [0, n_waypoints] (valid paths must not overlap).  An entry outside [0, n_waypoints] costs
 *   only the two paths that share it; swapped entries offsets[q], offsets[q+1] flag paths q and q+1; but an entry inside the
 *   range that is too LARGE (say offsets[q] = n_waypoints in the middle of the batch) flags every later path that starts below
 *   it: which of two in-range entries is the wrong one cannot be told, and overlapping paths are never evaluated.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): step not finite or <= 0, margin NaN, the
 * host variant's offsets breaking the CSR rules, a null waypoints / offsets / result pointer.  n_paths = 0 does nothing.
 * Results depend neither on the launch shape nor on the scheduling of work-groups (no atomics in the min or its index).
 * fiesta_hip_path_clearance      host pointers; stages the inputs, runs, synchronises (like fiesta_hip_get_dist_grad).  A batch
 *                                of at most 256 samples is answered on the host from the brick cache above, same arithmetic.
 * fiesta_hip_path_clearance_dev  every array (inputs and those of *result -- the struct itself is a host object) is a device
 *                                pointer; only enqueued on the map's stream, no host round trip (like _get_dist_grad_dev; a
 *                                hash-block map whose page set changed since its last query rebuilds its page table first, as
 *                                every query does). */
typedef struct fiesta_hip_path_result {
  double *min_dist;
  int64_t *min_index;
  double *min_pos;
  double *min_grad;
  int64_t *first_below;
  double *first_below_pos;
  int64_t *n_samples;
} fiesta_hip_path_result;
int fiesta_hip_path_clearance(fiesta_hip_map *m, const double *waypoints, int64_t n_waypoints, const int64_t *offsets,
                              int64_t n_paths, double step, double margin, const fiesta_hip_path_result *result);
int fiesta_hip_path_clearance_dev(fiesta_hip_map *m, const double *waypoints_dev, int64_t n_waypoints,
                                  const int64_t *offsets_dev, int64_t n_paths, double step, double margin,
                                  const fiesta_hip_path_result *result);

/* ---- path cost, batched: a smooth obstacle cost per polyline and its derivative with respect to every waypoint ----
 * What a trajectory optimiser needs per iteration (path clearance above serves the search half of a planner; a minimum and its
 * gradient at one sample is no descent direction).  No reference counterpart.  fiesta_hip_version() is still 101: detect these
 * two calls by symbol lookup.
 * Input: as path clearance -- CSR polylines, step, margin (here margin must be FINITE).  The samples are exactly path
 * clearance's (same rule, same indices), and a sample's value d and gradient g are fiesta_hip_get_dist_grad's bit for bit
 * (dense maps, a single shard, hash-block maps).  A sample outside a dense map has value -1 and gradient 0, the point query's
 * answer: it is penalised by phi(-1), pulls nowhere, and n_below counts it.
 *
 * Per sample, in f64, each operation rounded once (the library is built with -ffp-contract=off), in exactly this order:
 *   if d < margin:  e = margin - d;  phi = e * e;  psi = -2.0 * e;  gamma[c] = psi * g[c]      else phi = 0, gamma = 0.
 * Per segment j of a path (a = w[j], b = w[j+1]; d[c], L, S as in the sample rule; Sd = (double)S):
 *   the two end samples are the waypoints themselves: sample 0 of segment j is w[j]; w[j+1] is sample 0 of segment j+1 or the
 *   path's final sample.  Interior samples k = 1 .. S-1:  t = (double)k / Sd;  r = 1.0 - t;  their seven terms are
 *   phi,  r * gamma[c],  t * gamma[c];  P = sum phi, A[c] = sum r * gamma[c], B[c] = sum t * gamma[c] over the interior samples.
 *   h = L / Sd;   Q = (phi(w[j]) * 0.5 + P) + phi(w[j+1]) * 0.5;   qs = Q / Sd;   u[c] = d[c] / L;
 *   cost term           h * Q                                             (the trapezoid rule for the integral of phi along j)
 *   to the start, N[c]  h * (gamma(w[j])[c] * 0.5 + A[c]) - qs * u[c]
 *   to the end,   E[c]  h * (B[c] + gamma(w[j+1])[c] * 0.5) + qs * u[c]
 *   A segment with L = 0 contributes nothing to cost or gradient.
 * Outputs; every pointer of the result is nullable:
 *   cost       per path: the sum of h * Q over its segments, added in segment order -- approximates the integral of phi(d) ds
 *   grad (x3)  per WAYPOINT (n_waypoints rows): N of the segment that starts there + E of the segment that ends there (a missing
 *              one is 0): the exact derivative of `cost` of the waypoint's path at fixed S, wherever the interpolant is
 *              differentiable.  Every one of the n_waypoints rows is written by every call; rows that belong to no valid path are 0.
 *   length     per path: the sum of L over its segments, added in segment order
 *   n_below    per path: samples whose value is < margin (strictly)
 *   n_samples  per path: as fiesta_hip_path_result.n_samples
 * Every TERM above is bit-identical on the device, on the host and in fiesta_amd.path_cost_model (numpy); only the order in which
 * the interior samples' terms are added into P, A, B is left free: it is fixed by the call's arguments and the map (the device
 * adds by lane groups inside pieces whose size follows n_paths, the small-batch host route in sample order), so the two routes
 * are NOT promised bit-equal.  With n the number of terms that enter an output and a the sum of their absolute values on the
 * output's scale, any two orders differ by at most (n + 16) * 2^-52 * a (the bound the tests hold both routes to).
 * Determinism: no floating-point atomics; the same call on the same map gives the same bits; nothing depends on the launch
 * shape or on scheduling.
 * Special paths: empty or one waypoint: cost 0, length 0, gradient row 0, n_below by its samples (0 or 1).  Invalid (the rules of
 * path clearance, the device variant's offset rules included): cost NaN, length NaN, n_below -1, n_samples -1, its gradient rows
 * 0; the other paths are unaffected.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): those of path clearance, and a margin that
 * is not finite.  n_paths = 0 does nothing.
 * fiesta_hip_path_cost      host pointers; stages, runs, synchronises.  A batch of at most 256 samples is answered on the host from
 *                           the brick cache.
 * fiesta_hip_path_cost_dev  every array a device pointer (the struct itself is a host object); only enqueued on the map's stream. */
typedef struct fiesta_hip_path_cost_result {
  double *cost;
  double *grad;
  double *length;
  int64_t *n_below;
  int64_t *n_samples;
} fiesta_hip_path_cost_result;
int fiesta_hip_path_cost(fiesta_hip_map *m, const double *waypoints, int64_t n_waypoints, const int64_t *offsets, int64_t n_paths,
                         double step, double margin, const fiesta_hip_path_cost_result *result);
int fiesta_hip_path_cost_dev(fiesta_hip_map *m, const double *waypoints_dev, int64_t n_waypoints, const int64_t *offsets_dev,
                             int64_t n_paths, double step, double margin, const fiesta_hip_path_cost_result *result);

/* ---- body queries, batched: a robot body given as a set of spheres, checked at many poses ----
 * Every call above treats the robot as a point (its size is one scalar: margin, min_clearance).  A sampling planner checks a
 * candidate POSE of a body that is not round -- does anything touch, how close is it, where; an optimiser that models the body as
 * spheres needs per pose the summed obstacle penalty and its derivative with respect to the pose, a force and a torque.  No
 * reference counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * Input:
 *   spheres    f64 x 4 per sphere: the body-frame centre cx, cy, cz and the radius r; n_spheres in 1 .. FIESTA_HIP_BODY_MAX_SPHERES.
 *              A HOST pointer in BOTH variants (a property of the robot, small, validated by the call); the call copies it to the
 *              map's scratch on the map's stream, and the caller may reuse it as soon as the call returns.
 *   poses      f64 x 7 per pose: px, py, pz (metres), qw, qx, qy, qz.  The quaternion need not be normalised.
 *   margin     finite.
 * Per pose, in f64, each operation rounded once (the library is built with -ffp-contract=off), in exactly this order:
 *   s  = ((qw*qw + qx*qx) + qy*qy) + qz*qz;   k = 2.0 / s
 *   the pose is VALID iff its seven numbers are finite, s > 0 and k is finite
 *   xx=qx*qx  yy=qy*qy  zz=qz*qz  xy=qx*qy  xz=qx*qz  yz=qy*qz  wx=qw*qx  wy=qw*qy  wz=qw*qz
 *   R00 = 1.0 - k*(yy+zz)   R01 = k*(xy-wz)         R02 = k*(xz+wy)
 *   R10 = k*(xy+wz)         R11 = 1.0 - k*(xx+zz)   R12 = k*(yz-wx)
 *   R20 = k*(xz-wy)         R21 = k*(yz+wx)         R22 = 1.0 - k*(xx+yy)
 * Per sphere i of a valid pose:
 *   a[c] = (Rc0*cx + Rc1*cy) + Rc2*cz;   x[c] = p[c] + a[c]
 *   (d, g) = fiesta_hip_get_dist_grad's value and gradient at x, bit for bit (the path calls' evaluator)
 *   s_i = d - r
 *   if s_i < margin:  e = margin - s_i;  phi = e*e;  psi = -2.0*e;  gamma[c] = psi*g[c]     else phi = 0, gamma = 0   (path cost's penalty)
 *   t[0] = a[1]*gamma[2] - a[2]*gamma[1];  t[1] = a[2]*gamma[0] - a[0]*gamma[2];  t[2] = a[0]*gamma[1] - a[1]*gamma[0]
 * A sphere centre outside a dense map or in never-observed space reads what the point query reads there (-1 with gradient 0; the
 * +10000 corners): no special case, exactly as in path cost.
 * Outputs; every pointer of the result is nullable:
 *   min_clearance     per pose: the minimum over i of s_i
 *   min_sphere        per pose: the LOWEST i that attains it (compared with <)
 *   min_pos, min_grad per pose (x3): x and g of that sphere
 *   n_below           per pose: spheres with s_i < margin (strictly)
 *   cost              per pose: sum phi
 *   grad (x6)         per pose: sum gamma -- the derivative of cost with respect to p -- then sum t, the derivative with respect to a
 *                     small world-frame rotation vector theta about the body origin, R <- exp([theta]x) R
 *   sphere_clearance  per pose x sphere, row-major: s_i (per-link costs; callers with a penalty of their own)
 * Every TERM above (x, s_i, phi, gamma, t) is bit-identical on the device and in fiesta_amd.body_query_model (numpy), and
 * sphere_clearance, min_clearance, min_sphere, min_pos, min_grad and n_below are exact.  Only the order in which the n_spheres terms
 * are added into cost and grad is left free; it is FIXED BY n_spheres ALONE (a team of T lanes per pose, T the smallest power of
 * two >= n_spheres and at most 64: lane t adds spheres t, t + T, ... in that order, then a butterfly over the team), so the bits
 * of a pose's outputs depend neither on n_poses, nor on the pose's place in the batch, nor on the variant, the launch shape or
 * scheduling.  Against another order of summation cost and grad differ by at most path cost's bound (n + 16) * 2^-52 * a, n =
 * n_spheres, a = the sum of the absolute values of the output's terms.  No floating-point atomics.
 * Invalid pose: min_clearance, cost, its min_pos / min_grad and its sphere_clearance row NaN; min_sphere and n_below -1; its grad
 * row 0.  The other poses are unaffected.  Validity is decided on the device.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable, fiesta_hip_last_error() names the cause): a
 * null map; n_spheres outside 1 .. 1024; n_poses < 0; a null spheres; a null poses with n_poses > 0; a null result; a sphere whose
 * centre or radius is not finite or whose radius is < 0; a margin that is not finite.  n_poses = 0 does nothing.
 * The call is read-only and reads the field as it stands: before fiesta_hip_update_esdf has run it answers from the old field
 * (the path calls' rule).
 * fiesta_hip_body_query      poses and results are host pointers; stages, runs, synchronises.  Always on the device.
 * fiesta_hip_body_query_dev  poses and every result array are device pointers (the struct itself and spheres are host objects);
 *                            only enqueued on the map's stream. */
#define FIESTA_HIP_BODY_MAX_SPHERES 1024
typedef struct fiesta_hip_body_result {
  double *min_clearance;
  int32_t *min_sphere;
  double *min_pos;
  double *min_grad;
  int32_t *n_below;
  double *cost;
  double *grad;
  double *sphere_clearance;
} fiesta_hip_body_result;
int fiesta_hip_body_query(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses, int64_t n_poses, double margin,
                          const fiesta_hip_body_result *result);
int fiesta_hip_body_query_dev(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses_dev, int64_t n_poses,
                              double margin, const fiesta_hip_body_result *result);

/* ---- articulated body queries, batched: spheres on frames, one pose per frame and configuration ----
 * The body call above moves one rigid set of spheres.  An arm, a drone with a gimbal or a slung load, a formation of several robots
 * is a set of rigid links -- FRAMES -- each with spheres of its own.  Here every sphere names its frame, a CONFIGURATION gives one
 * pose per frame, and one call returns per configuration what the body call returns per pose and, per frame, the clearance, the
 * penalty and the force and torque on that frame -- what a caller multiplies with its geometric Jacobian.  Forward kinematics is
 * the caller's: it needs sin / cos, whose bits differ between hosts and the device.  Self-collision between the links is not
 * checked.  No reference counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * Input:
 *   spheres       f64 x 4 per sphere: the centre cx, cy, cz in the frame of its own link and the radius r; n_spheres in
 *                 1 .. FIESTA_HIP_BODY_MAX_SPHERES.
 *   sphere_frame  i32 per sphere: its frame, in 0 .. n_frames - 1, NON-DECREASING over the table (the spheres are grouped by frame;
 *                 fiesta_amd.group_spheres_by_frame sorts a table that is not).  A frame may own no sphere.
 *                 Both are HOST pointers in BOTH variants, as the body call's table: copied on the map's stream, free for reuse
 *                 as soon as the call returns.
 *   n_frames      F, in 1 .. FIESTA_HIP_BODY_MAX_FRAMES.
 *   frame_poses   f64 x 7 per configuration and frame, configuration-major (n_configs x F x 7): px, py, pz (metres), qw, qx, qy, qz.
 *                 The quaternions need not be normalised.
 *   margin        finite.
 * Per configuration n and frame f the rotation R and the validity of the pose are the body call's rule above, operation by
 * operation (s, k = 2.0 / s, the nine products, R00 .. R22); p is the pose's position.  A configuration is VALID iff all F frame
 * poses are valid by that rule, the poses of frames that own no sphere included.
 * Per sphere i of frame f of a valid configuration, with R, p of frame f, the body call's terms verbatim:
 *   a[c] = (Rc0*cx + Rc1*cy) + Rc2*cz;   x[c] = p[c] + a[c];   (d, g) = the point query at x;   s_i = d - r
 *   phi, gamma[c] = path cost's penalty of s_i against margin;   t = a x gamma, component by component as written above
 * Outputs; every pointer of the result is nullable:
 *   min_clearance     per configuration: the minimum over ALL spheres of s_i
 *   min_sphere        per configuration: the LOWEST i that attains it (compared with <), whatever its frame
 *   min_pos, min_grad per configuration (x3): x and g of that sphere
 *   n_below           per configuration: spheres with s_i < margin (strictly)
 *   cost              per configuration: sum phi over all spheres
 *   frame_clearance   per configuration x frame: the minimum of s_i over the frame's spheres; +inf for a frame without spheres
 *   frame_cost        per configuration x frame: sum phi over the frame's spheres (0 without spheres)
 *   frame_grad (x6)   per configuration x frame: sum gamma, then sum t, over the frame's spheres (0 without spheres): the derivative
 *                     of the configuration's cost with respect to frame f's position and to a small world-frame rotation vector
 *                     theta about frame f's origin, R_f <- exp([theta]x) R_f, the other frames fixed
 *   sphere_clearance  per configuration x sphere, row-major: s_i
 * Every TERM is bit-identical on the device and in fiesta_amd.articulated_query_model (numpy); min_clearance, min_sphere, min_pos,
 * min_grad, n_below, frame_clearance and sphere_clearance are exact.  Only the order in which terms are added into cost, frame_cost
 * and frame_grad is left free; it is FIXED BY n_spheres AND sphere_frame ALONE (a team of T lanes per configuration, T as in the body
 * call; per pass of T consecutive spheres and per frame present in it a butterfly over the team, the passes of a frame added in
 * order; cost is the frame costs added in frame order), so the bits of a configuration's outputs depend neither on n_configs, nor
 * on its place in the batch, nor on the variant, the launch shape or scheduling.  Against another order of summation they differ by
 * at most (n + 16) * 2^-52 * a, n = the number of summed terms (the frame's sphere count; n_spheres for cost), a = the sum of the
 * absolute values of the output's terms.  No floating-point atomics.
 * Invalid configuration: min_clearance, cost, its min_pos / min_grad and its frame_clearance, frame_cost and sphere_clearance rows
 * NaN; min_sphere and n_below -1; its frame_grad rows 0.  The other configurations are unaffected.  Validity is decided on the device.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable, fiesta_hip_last_error() names the cause): a
 * null map; n_spheres outside 1 .. 1024; n_frames outside 1 .. 64; n_configs < 0; a null spheres or sphere_frame; a null
 * frame_poses with n_configs > 0; a null result; a sphere whose centre or radius is not finite or whose radius is < 0; a frame index
 * outside 0 .. n_frames - 1; frame indices that decrease (not grouped by frame); a margin that is not finite.  n_configs = 0 does
 * nothing.
 * The call is read-only and reads the field as it stands: before fiesta_hip_update_esdf has run it answers from the old field
 * (the path calls' rule).
 * fiesta_hip_articulated_query      frame poses and results are host pointers; stages, runs, synchronises.  Always on the device.
 * fiesta_hip_articulated_query_dev  frame poses and every result array are device pointers (the struct itself, spheres and
 *                                   sphere_frame are host objects); only enqueued on the map's stream. */
#define FIESTA_HIP_BODY_MAX_FRAMES 64
typedef struct fiesta_hip_articulated_result {
  double *min_clearance;
  int32_t *min_sphere;
  double *min_pos;
  double *min_grad;
  int32_t *n_below;
  double *cost;
  double *frame_clearance;
  double *frame_cost;
  double *frame_grad;
  double *sphere_clearance;
} fiesta_hip_articulated_result;
int fiesta_hip_articulated_query(fiesta_hip_map *m, const double *spheres, const int32_t *sphere_frame, int32_t n_spheres, int32_t n_frames,
                                 const double *frame_poses, int64_t n_configs, double margin, const fiesta_hip_articulated_result *result);
int fiesta_hip_articulated_query_dev(fiesta_hip_map *m, const double *spheres, const int32_t *sphere_frame, int32_t n_spheres,
                                     int32_t n_frames, const double *frame_poses_dev, int64_t n_configs, double margin,
                                     const fiesta_hip_articulated_result *result);

/* ---- body sweeps, batched: a sphere-set body checked along polylines of poses ----
 * Path clearance answers "is this path free for a point", the body query "is this pose free for a body".  A sampling planner asks of
 * every edge it tries whether the MOTION is free for the BODY: a rod-shaped drone that yaws while it flies through a door.  This call
 * samples the poses between the waypoint poses, evaluates each as the body query does and reduces per path.  No reference
 * counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * Input:
 *   spheres, n_spheres   the body query's table, a HOST pointer in both variants, with the same validation
 *   poses      f64 x 7 per WAYPOINT pose: px, py, pz (metres), qw, qx, qy, qz.  The quaternions need not be normalised.
 *   offsets    n_paths + 1 int64: path p is the pose rows offsets[p] .. offsets[p + 1] - 1 (the CSR rules of path clearance)
 *   step       metres, finite and > 0;   margin   finite
 * The table's reach, computed on the host (fiesta_amd.body_reach is the same rule in numpy):
 *   reach = max over i of sqrt((cx*cx + cy*cy) + cz*cz)
 * Per waypoint pose: validity is the body query's rule verbatim -- seven finite numbers, s = ((qw*qw + qx*qx) + qy*qy) + qz*qz > 0,
 * k = 2.0 / s finite -- then   n = sqrt(s);   u[c] = q[c] / n.
 * Per segment j of a path, between the waypoints (a, u0) and (b, u1); in f64, each operation rounded once (the library is built with
 * -ffp-contract=off), in exactly this order:
 *   d[c] = b[c] - a[c];   L = sqrt(d0*d0 + d1*d1 + d2*d2)                       (left to right: the path rule)
 *   dot = ((u0w*u1w + u0x*u1x) + u0y*u1y) + u0z*u1z;   v = u1 if dot >= 0, else -u1   (the shorter arc)
 *   e[c] = v[c] - u0[c];   ch = sqrt(((e0*e0 + e1*e1) + e2*e2) + e3*e3);   W = (2.25 * reach) * ch
 *   S = max(1, (int64)ceil((L + W) / step));   Sd = (double)S
 *   sample k = 0 .. S-1:   t = (double)k / Sd;   r = 1.0 - t;   p[c] = a[c] + d[c]*t;   q[c] = r*u0[c] + t*v[c]
 * After the last segment comes one final sample: the last waypoint's position with its own u.  A path of one pose has exactly that
 * sample.  Sample indices run in this order.
 * A sample's pose (p, q) goes through the body query's rule verbatim: R from q with k = 2 / |q|^2, then per sphere a = R c,
 * x = p + a, (d, g) = fiesta_hip_get_dist_grad's value and gradient at x bit for bit, s_i = d - r_i.
 * Why W: the segment rotates by theta = 4 asin(ch / 2); q(t) is normalised linear interpolation, which follows slerp's arc at a speed
 * proportional to 1 / |q(t)|^2 (with dot >= 0, |q(t)|^2 >= 1/2: every sample of a valid path is a valid pose).  2.25 ch >= theta up
 * to 90 degrees and exceeds it by at most 12.5 %: there no sphere centre moves farther than step between consecutive samples; up
 * to 180 degrees at most 1.26 step.  A segment without rotation has W = 0 and path clearance's positions bit for bit.
 * This is a SAMPLED check, as path clearance is: no continuous guarantee.
 * Outputs, one row per path; every pointer of the result is nullable:
 *   min_clearance        the minimum of s_i over all samples and spheres
 *   min_sample (i64)     the lowest sample index that attains it
 *   min_sphere (i32)     the lowest sphere that attains it in that sample (compared with <, as the body query)
 *   min_pose (x7)        that sample's (p, q) by the rule
 *   min_pos, min_grad (x3)  x and g of that sphere there
 *   first_below (i64)    the lowest sample index with any s_i < margin (strictly), -1 if none
 *   first_below_sphere (i32)  the lowest such sphere in that sample, -1 if none
 *   first_below_pose (x7)     that sample's pose, NaN if none
 *   n_below (i64)        samples with at least one sphere below the margin
 *   n_samples (i64)      the path's sample count
 * Every output is exact -- bits and NaN pattern -- on the device and in fiesta_amd.body_sweep_model (numpy): nothing is summed.  The
 * results depend neither on the batch, nor on the path's place in it, nor on the variant, the launch shape or scheduling; no atomics.
 * Empty path: n_samples 0, min_clearance +inf, the indices -1, poses and positions NaN, min_grad 0, n_below 0.
 * Invalid path: n_samples -1, min_clearance NaN, the indices -1, poses and positions NaN, min_grad 0, n_below -1.  A path is invalid
 * for an invalid waypoint pose, a segment with (L + W) / step > 2^24, or -- device variant -- offsets out of order or out of range by
 * path clearance's rules.  The other paths are unaffected.  Validity is decided on the device.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable, fiesta_hip_last_error() names the cause): the
 * body query's on the table and the margin (n_spheres outside 1 .. 1024, a null spheres, a sphere that is not finite or has a
 * negative radius, a margin that is not finite); path clearance's on step, offsets and null pointers (a null map, poses, offsets or
 * result; negative counts; a step that is not finite or <= 0; host variant: offsets[0] != 0, offsets[n_paths] != n_poses, offsets
 * that decrease).  n_paths = 0 does nothing.
 * The call is read-only and reads the field as it stands: before fiesta_hip_update_esdf has run it answers from the old field
 * (the path calls' rule).
 * fiesta_hip_body_sweep      poses, offsets and results are host pointers; stages, runs, synchronises.  Always on the device.
 * fiesta_hip_body_sweep_dev  poses, offsets and every result array are device pointers (the struct itself and spheres are host
 *                            objects); only enqueued on the map's stream. */
typedef struct fiesta_hip_sweep_result {
  double *min_clearance;
  int64_t *min_sample;
  int32_t *min_sphere;
  double *min_pose;
  double *min_pos;
  double *min_grad;
  int64_t *first_below;
  int32_t *first_below_sphere;
  double *first_below_pose;
  int64_t *n_below;
  int64_t *n_samples;
} fiesta_hip_sweep_result;
int fiesta_hip_body_sweep(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses, int64_t n_poses,
                          const int64_t *offsets, int64_t n_paths, double step, double margin, const fiesta_hip_sweep_result *result);
int fiesta_hip_body_sweep_dev(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses_dev, int64_t n_poses,
                              const int64_t *offsets_dev, int64_t n_paths, double step, double margin,
                              const fiesta_hip_sweep_result *result);

/* ---- frontier voxels: observed-free voxels that border never-observed space, compacted on the device ----
 * What an exploration planner asks after every frame: where does known free space end, and which of those places can the robot
 * reach?  No reference counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * For a voxel v of the map, in map voxel coordinates (those fiesta_hip_get_occupied_voxels reports):
 *   observed(v)  v has been observed at least once: exactly the voxels where fiesta_hip_download_field's d2 >= 0; on a hash-block
 *                map the voxels fiesta_hip_download_hash lists with d2 >= 0 (a voxel of a tile without a page is not observed).
 *   free(v)      observed(v) and Exist(v) is false (GetOccupancy(v) == 0).
 *   u(v)         the unknown-neighbour mask, six bits: a bit is set where that 6-neighbour is inside the map and not observed.
 *                bit 0: -x, bit 1: +x, bit 2: -y, bit 3: +y, bit 4: -z, bit 5: +z.  A neighbour outside a dense map's array is NOT
 *                unknown (the outer face of the map is no frontier); a hash-block map has no outside.  The query box below does
 *                not clip the neighbour test.
 *   frontier(v)  free(v) and u(v) != 0, v inside the inclusive voxel box [lo, hi], and -- only if min_clearance > 0 --
 *                GetDistance(Vector3i v) >= min_clearance, with the very f64 value the voxel query returns
 *                (sqrt((double)d2) * resolution; +10000 for "observed, no obstacle", which therefore passes).  With
 *                min_clearance <= 0 the field is not read at all.  The field is read as it stands, like every query: after
 *                UpdateOccupancy and before UpdateESDF the filter sees the old distances.
 * lo / hi are HOST pointers in both variants.  Both NULL: the whole array of a dense map, every page of a hash-block map (parked
 * pages included: they answer every query).  The box is intersected with the map; an empty intersection, or lo[c] > hi[c], gives
 * a total of 0 and is no error.
 * At most `capacity` entries are written: vox holds 3 int32 per entry, mask holds u(v), entry k of both arrays describes the same
 * voxel; each of the two is nullable.  *n_out is the total whatever the capacity (call with capacity 0 to size the buffers, as
 * with the visualisation getters).  Order is unspecified; the SET of (v, u(v)) pairs is exact and the same for every launch shape.
 * A map created as a shard answers for its own array, like fiesta_hip_get_occupied_voxels; there is no shard-group call.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): min_clearance is NaN, exactly one of lo / hi
 * is NULL, capacity is negative, n_out is NULL.
 * fiesta_hip_get_frontier_voxels      host arrays; stages, runs, synchronises, copies min(total, capacity) entries back.
 * fiesta_hip_get_frontier_voxels_dev  vox_dev / mask_dev / n_out_dev are device pointers; only enqueued on the map's stream, no host
 *                                     round trip: the call zeroes *n_out_dev itself (a hash-block map first rebuilds its page table
 *                                     if its page set changed, as every query does). */
int fiesta_hip_get_frontier_voxels(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], double min_clearance, int32_t *vox,
                                   uint8_t *mask, int64_t capacity, int64_t *n_out);
int fiesta_hip_get_frontier_voxels_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], double min_clearance,
                                       int32_t *vox_dev, uint8_t *mask_dev, int64_t capacity, unsigned long long *n_out_dev);

/* ---- skeleton voxels: the distance field's ridge between obstacles, compacted on the device ----
 * Where is the robot equally far from two different obstacles?  Every field word names its voxel's closest obstacle; where two
 * neighbouring voxels name obstacles that lie apart, the field has a ridge: the generalised Voronoi skeleton of free space -- the
 * middle of corridors, doorways and gaps, the routes of maximum clearance, the topology of free space as a sparse voxel set.  No
 * reference counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * For a voxel v of the map, in map voxel coordinates:
 *   observed(v), free(v)  exactly as for fiesta_hip_get_frontier_voxels.
 *   site(v)      defined iff observed(v) and the field word carries an obstacle: 0 <= d2 < INT32_MAX in fiesta_hip_download_field /
 *                fiesta_hip_download_hash.  ("Observed, no obstacle" has no site, whatever stale link the word keeps.)  Its value is
 *                the stored closest obstacle in map voxel coordinates, the coc triple those dumps report.
 *   ridge(v, n)  for a 6-neighbour n of v with a = site(v) and b = site(n) both defined, sep2 = |a - b|^2 and
 *                g(x) = |x - b|^2 - |x - a|^2 (linear in x: the signed side of the bisector plane of a and b):
 *                  sep2 >= min_sep2  and  g(v) >= 0  and  g(n) <= 0  and  g(v) <= -g(n)
 *                -- the bisector passes between the two voxels and v is at least as close to it as n (a tie marks both).  A pair that
 *                the field's own inexactness puts on the wrong side of its bisector is skipped.  Integers only.  A neighbour
 *                outside a dense map's array, not observed or without a site gives no ridge.  The query box below does not clip the
 *                neighbour test.
 *   r(v)         the six-bit mask of the neighbours with ridge(v, n).  bit 0: -x, bit 1: +x, bit 2: -y, bit 3: +y, bit 4: -z, bit 5: +z.
 *   skeleton(v)  free(v), site(v) defined, r(v) != 0, v inside the inclusive voxel box [lo, hi], and -- only if min_clearance > 0 --
 *                GetDistance(Vector3i v) >= min_clearance, with the very f64 value the voxel query returns.  The field is read as
 *                it stands, like every query: after UpdateOccupancy and before UpdateESDF occupancy is new and the sites are old.
 * min_sep2 >= 1.  Adjacent voxels of one flat surface are distinct sites 1, 2 or 4 apart (squared): values up to 4 mark the whole
 * neighbourhood of any flat surface; 9 or more keeps the ridges between separate obstacles.  Callers who prune by ANGLE do so from
 * the returned sep2 and d2 (the sites subtend an angle of 2 asin(sqrt(sep2 / d2) / 2) at v, roughly); the call itself does not.
 * lo / hi are HOST pointers in both variants; both NULL, clipping and empty boxes exactly as for fiesta_hip_get_frontier_voxels.
 * At most `capacity` entries are written.  Entry k of every array of the result describes the same voxel; each array is nullable.
 * *n_out is the total whatever the capacity (call with capacity 0 to size the buffers).  Order is unspecified; the SET of
 * (v, r(v), d2, sep2) rows is exact and the same for every launch shape.  A map created as a shard answers for its own array;
 * there is no shard-group call.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): min_sep2 < 1, min_clearance is NaN, exactly
 * one of lo / hi is NULL, capacity is negative, result or n_out is NULL.
 * fiesta_hip_get_skeleton_voxels      host arrays; stages, runs, synchronises, copies min(total, capacity) entries back.
 * fiesta_hip_get_skeleton_voxels_dev  the result's arrays and n_out_dev are device pointers; only enqueued on the map's stream, no
 *                                     host round trip: the call zeroes *n_out_dev itself.  The counter feeds
 *                                     fiesta_hip_cluster_voxels_dev; with d2 as the key every cluster comes with its narrowest
 *                                     member, the bottleneck of the passage. */
typedef struct fiesta_hip_skeleton_result { /* every pointer nullable */
  int32_t *vox;                             /* per entry x 3, map voxel coordinates */
  uint8_t *mask;                            /* per entry: r(v) */
  int32_t *d2;                              /* per entry: the voxel's own squared distance, in voxels */
  int32_t *sep2;                            /* per entry: the largest sep2 over the set bits of r(v) */
} fiesta_hip_skeleton_result;
int fiesta_hip_get_skeleton_voxels(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], int32_t min_sep2, double min_clearance,
                                   int64_t capacity, const fiesta_hip_skeleton_result *result, int64_t *n_out);
int fiesta_hip_get_skeleton_voxels_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], int32_t min_sep2,
                                       double min_clearance, int64_t capacity, const fiesta_hip_skeleton_result *result,
                                       unsigned long long *n_out_dev);

/* ---- ray queries: what a sensor ray from start to end would cross, read-only and batched ----
 * Line of sight for path shortcutting and any-angle search (occupied AND unknown must block, which the distance field cannot tell
 * apart), the information gain of a candidate view (unknown voxels along its rays up to the first obstacle -- the question after
 * fiesta_hip_get_frontier_voxels), an expected depth image.  Nothing is written to the map.  No reference counterpart as a call;
 * the traversal is the reference's.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 *
 * start / end: n x 3 f64, metres.  All arithmetic is f64, in the order written here, every operation rounded once.
 * The walk W of a ray:
 *   1. a[c] = start[c] / resolution, b[c] = end[c] / resolution (the operands the ray cast hands to its traversal).
 *   2. R = the voxel sequence of the reference's Raycast(a, b, min, max) (src/raycast.cpp:56-158; in voxel units, like the output
 *      of fiesta_hip_raycast_single) with min = -2^31 and max = 2^31 on every axis -- nothing is clipped -- and without its
 *      1500-voxel exception; its loop runs at most 8192 iterations.
 *   3. W = R with its LAST element replaced by e = floor(b); R empty (start and end in one voxel): W = [e].
 *      (The per-frame loop of the ray cast never marks Raycast's last output -- include/Fiesta.h:239 starts one before it -- and
 *      marks the end point's voxel on its own; that last output is not always e, the traversal can stop one voxel to the side
 *      through its squared-reach test.  So W is what a ray cast alone in a frame observes: after it, and UpdateOccupancy, no voxel
 *      of W is unknown, given min_ray_length 0 and a map origin that is a multiple of the resolution.)
 *   Indices k = 0 .. |W| - 1 run from start to end.
 * The class of W[k] = r:
 *   1. centre p[c] = (r[c] + 0.5) * resolution;  2. map voxel v[c] = floor((p[c] - origin[c]) / resolution) (Pos2Vox; saturated
 *      at +-(2^31 - 1)) -- the arithmetic of the ray cast's visits;
 *   3. dense map: OUTSIDE if PosInMap(p) is false (p outside [origin, origin + map_size]; a shard: the global map's range) or v is
 *      not in the map's array (a shard answers for its own array, ghost layers included, like fiesta_hip_get_frontier_voxels);
 *   4. UNKNOWN if v is not observed: fiesta_hip_download_field's d2 < 0; on a hash-block map a voxel fiesta_hip_download_hash
 *      lists with d2 < 0 or a voxel of a tile without a page (parked pages answer, as for every query; a hash-block map has no
 *      OUTSIDE);
 *   5. else OCCUPIED if Exist(v) (GetOccupancy(v) == 1), else FREE.  UNKNOWN takes precedence over a stale occupancy bit.
 *   Classes are read from the occupancy state as it stands: UpdateOccupancy changes them, UpdateESDF does not (the distance field
 *   is never read).
 * stop_mask: a subset of OCCUPIED | UNKNOWN | OUTSIDE (0..7).  Per ray (every pointer of the result struct is nullable):
 *   hit_index  the smallest k with class(W[k]) & stop_mask != 0; -1: none
 *   hit_class  that voxel's class; 0: none
 *   hit_vox    that voxel's map voxel v; INT32_MIN x 3: none
 *   hit_dist   q[c] = p[c] - start[c] for that voxel's centre p, sqrt(q0*q0 + q1*q1 + q2*q2) summed left to right; NaN: none
 *   n_visited  hit_index + 1 with a hit, else |W|
 *   counts     the numbers of FREE, OCCUPIED, UNKNOWN, OUTSIDE voxels among W[k], k < n_visited, the hit voxel itself not counted
 *   Every output is an integer or an f64 in a fixed operation order: the same bits for every launch shape, and the bits of
 *   fiesta_amd.ray_query_model (the definition in numpy) and of the C++ facade.
 *   Uses: line of sight through known free space -- stop_mask 7, the segment is clear iff hit_index == -1 (and n_visited >= 0);
 *   the gain of a view -- stop_mask 1 (OCCUPIED), read counts[2]; expected depth -- stop_mask 1 or 3, read hit_dist.
 * An INVALID ray -- a non-finite component, |a[c]| or |b[c]| >= 2^30, or M = |floor(b)[0] - floor(a)[0]| + |..[1]| + |..[2]| > 4095
 * -- reads n_visited -1, hit_index -1, hit_class 0, hit_vox INT32_MIN x 3, hit_dist NaN, counts 0; the other rays are unaffected.
 * (A valid ray's walk has at most M + 1 voxels.)
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): start, end or result NULL, stop_mask outside
 * 0..7, n negative.  n = 0 does nothing.
 * fiesta_hip_ray_query      host arrays; stages, runs, synchronises, copies back.
 * fiesta_hip_ray_query_dev  start_dev / end_dev and the arrays the result struct names are device pointers (the struct itself is a
 *                           host object); only enqueued on the map's stream (a hash-block map first rebuilds its page table if its
 *                           page set changed, as every query does).
 * Both launch one kernel whatever n is: there is no host-cache route, a call with one ray costs a launch (and the host variant a
 * synchronisation) -- batch the rays of a view or of a search front. */
#define FIESTA_HIP_RAY_FREE 0
#define FIESTA_HIP_RAY_OCCUPIED 1
#define FIESTA_HIP_RAY_UNKNOWN 2
#define FIESTA_HIP_RAY_OUTSIDE 4
typedef struct fiesta_hip_ray_result { /* every pointer nullable */
  int32_t *n_visited;                  /* per ray */
  int32_t *hit_index;                  /* per ray */
  uint8_t *hit_class;                  /* per ray */
  int32_t *hit_vox;                    /* per ray x 3, map voxel coordinates */
  double *hit_dist;                    /* per ray, metres */
  int32_t *counts;                     /* per ray x 4: free, occupied, unknown, outside */
} fiesta_hip_ray_result;
int fiesta_hip_ray_query(fiesta_hip_map *m, const double *start, const double *end, int64_t n, int32_t stop_mask,
                         const fiesta_hip_ray_result *result);
int fiesta_hip_ray_query_dev(fiesta_hip_map *m, const double *start_dev, const double *end_dev, int64_t n, int32_t stop_mask,
                             const fiesta_hip_ray_result *result);

/* ---- reachability: the cost-to-go field through traversable space, flooded on the device ----
 * The second half of the frontier question: WHICH of those places can the robot reach, and how far is it?  A clearance per voxel is
 * a local test -- a frontier voxel behind a wall, in a pocket seen through a window or behind a door narrower than the robot passes
 * it.  This call floods the traversable voxels of a box from seed voxels and reports the travel cost of every voxel and of a list
 * of targets (e.g. the frontier call's output).  Read-only; no reference counterpart.  fiesta_hip_version() is still 101: detect
 * these two calls by symbol lookup.
 * The box: lo / hi are HOST pointers in both variants, an inclusive voxel box in map voxel coordinates (those
 *   fiesta_hip_get_frontier_voxels reports).  It is intersected with a dense map's array (a map created as a shard answers for its
 *   own array, like the frontier call; there is no shard-group call); both NULL: the whole array.  A hash-block map has no outside:
 *   there the box is mandatory (both NULL is an error) and only clamped to +-2^30 per coordinate.  With extents ex, ey, ez the
 *   clipped box must satisfy ex * ey * ez <= 2^28.  An empty intersection, or lo[c] > hi[c], is no error: *info reads all zero and
 *   the target costs read -1.
 * traversable(v), for v inside the clipped box: either
 *   - free(v) exactly as the frontier call defines it (observed and not Exist) and -- only if min_clearance > 0 --
 *     GetDistance(Vector3i v) >= min_clearance with the voxel query's own f64 value (+10000 passes); or
 *   - flags & FIESTA_HIP_REACH_THROUGH_UNKNOWN and v is not observed (optimistic planning; no clearance test on such a voxel; a
 *     tile without a page on a hash-block map is unknown).
 *   A voxel outside the clipped box is not traversable.  With min_clearance <= 0 the distance field is not read at all.  The map is
 *   read as it stands: after UpdateOccupancy and before UpdateESDF the clearance filter sees the old distances.
 * Moves: between two traversable voxels that differ by at most 1 per axis; a move that changes 1, 2 or 3 axes weighs 3, 4 or 5 (the
 *   3-4-5 chamfer), so costs are integers in units of a third of a voxel: metres ~ cost * resolution / 3.  connectivity 6 allows
 *   only the weight-3 moves, 26 all of them.  A diagonal move needs only its two ends traversable (ask with 6, or with a clearance,
 *   for no corner cutting).
 * Seeds: n_seeds x 3 int32 map voxels; a seed outside the clipped box or not traversable is ignored.  n_seeds = 0 or no usable
 *   seed is no error: nothing is reached.
 * cost(v), per voxel of the clipped box: the minimum total weight over all move sequences from any usable seed to v; INT32_MAX if
 *   v is traversable and there is none; -1 if v is not traversable.  This is the fixed point of a shortest-path relaxation on
 *   integer weights: it is unique, so every output is exact and the same bits for any launch shape and scheduling, and the bits of
 *   fiesta_amd.reach_model (the definition in numpy).
 * Outputs; every pointer of the result struct is nullable (the struct itself is not):
 *   cost         int32, ex * ey * ez entries in box-local linear order ((x - lo'x) * ey + (y - lo'y)) * ez + (z - lo'z), lo' the
 *                clipped corner (info->box_lo)
 *   target_cost  int32 per target (targets: n_targets x 3 map voxels): cost(v), or -1 for a target outside the clipped box
 * info (a HOST struct in both variants, nullable): the clipped box, the number of traversable voxels, of usable seed entries (a
 *   voxel listed twice counts twice), of traversable voxels with a finite cost, the largest finite cost (0: nothing reached), and
 *   how the flood ran: rounds (launches that found work) and tile visits (16 x 16 x 32-voxel tiles of the box relaxed, over all rounds).
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): min_clearance is NaN, exactly one of lo / hi
 *   is NULL, both NULL on a hash-block map, a clipped box above 2^28 voxels, connectivity other than 6 or 26, unknown flag bits, a
 *   negative count, seeds NULL with n_seeds > 0, targets NULL with n_targets > 0, target_cost given without targets, result NULL.
 *   The flood's scratch memory (the box's bitmap, tile flags and lists, a cost field when the caller passes none) belongs to the
 *   map: allocated on first use, grown as needed, freed by fiesta_hip_destroy; a failed allocation is FIESTA_HIP_ERR_NOMEM and leaves
 *   the map usable.  FIESTA_HIP_ERR_STATE: the flood ran more rounds than there are traversable voxels (a defect, never expected).
 * fiesta_hip_reach_field      host arrays; stages, runs, synchronises, copies back.
 * fiesta_hip_reach_field_dev  seeds / targets and the arrays the result struct names are device pointers.  UNLIKE the other _dev
 *                             calls this one synchronises with the map's stream: the number of rounds depends on the data, so
 *                             the call reads a small counter block after every batch of eight rounds (a hash-block map first
 *                             rebuilds its page table if its page set changed, as every query does). */
#define FIESTA_HIP_REACH_THROUGH_UNKNOWN 1
typedef struct fiesta_hip_reach_result { /* every pointer nullable */
  int32_t *cost;                         /* ex * ey * ez, box-local order */
  int32_t *target_cost;                  /* per target */
} fiesta_hip_reach_result;
typedef struct fiesta_hip_reach_info {
  int32_t box_lo[3], box_hi[3]; /* the clipped box, map voxel coordinates, inclusive */
  int64_t n_traversable;
  int64_t n_seeds_used;
  int64_t n_reached;
  int64_t max_cost;
  int64_t rounds;
  int64_t tile_visits;
} fiesta_hip_reach_info;
int fiesta_hip_reach_field(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds, int64_t n_seeds,
                           const int32_t *targets, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                           const fiesta_hip_reach_result *result, fiesta_hip_reach_info *info);
int fiesta_hip_reach_field_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds_dev, int64_t n_seeds,
                               const int32_t *targets_dev, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                               const fiesta_hip_reach_result *result, fiesta_hip_reach_info *info);

/* ---- reach matrix: pairwise travel costs between sites, the floods batched on the device ----
 * What a tour planner needs after the chain frontier voxels -> clusters -> views -> reachability: the travel cost between every
 * pair of sites (the robot and one viewpoint per frontier cluster), the cost matrix a tour solver takes.  Row s is the flood of
 * fiesta_hip_reach_field from source s alone, read at the columns; the floods of one call share ONE traversability bitmap and run
 * side by side, a launch per round for all of them.  Read-only; no reference counterpart.  fiesta_hip_version() is still 101:
 * detect these two calls by symbol lookup.
 * Shared with fiesta_hip_reach_field, word for word: the box (lo / hi HOST pointers in both variants, clipped to a dense map's
 *   array, mandatory on a hash-block map and clamped there, at most 2^28 voxels after clipping, an empty intersection is no error),
 *   traversable(v) with min_clearance and FIESTA_HIP_REACH_THROUGH_UNKNOWN, the moves with their weights 3 / 4 / 5, connectivity
 *   6 or 26.
 * Sources: n_sources x 3 int32 map voxels; each source is a flood of its own from that single voxel.  source_status:
 *   FIESTA_HIP_REACH_SITE_OK; _OUTSIDE: the source lies outside the clipped box; _BLOCKED: inside, not traversable.
 * Columns: targets, n_targets x 3 int32 map voxels; with targets == NULL and n_targets == 0 the columns are the sources themselves
 *   (the square form, n_cols = n_sources).
 * cost[s * n_cols + j]: if source s is OK, bit for bit target_cost[j] of fiesta_hip_reach_field with seeds = {source s}: the minimum
 *   total weight of a move sequence from the source to column voxel j, INT32_MAX if that voxel is traversable and not reached, -1
 *   if it lies outside the clipped box or is not traversable.  If source s is OUTSIDE or BLOCKED its whole row is -1 and
 *   source_reached[s] is 0 (reach_field with an unusable seed reports INT32_MAX for traversable targets instead): -1 always means
 *   "this site is no place to be", and since moves are symmetric and traversability belongs to the voxel, the square form is
 *   SYMMETRIC.  Every number is an integer and the fixed point is unique: every output has the same bits for any launch shape,
 *   batch width and scheduling, and the bits of fiesta_amd.reach_matrix_model.
 * max_fields: an upper bound on the floods run side by side; 0: as many as the budget allows.  The budget: B * (voxels of the
 *   clipped box) <= 2^28 cost entries (1 GiB of scratch at most), B >= 1 always.  Sources are processed in batches of B consecutive
 *   entries; a source listed twice may be flooded twice.  The outputs do not depend on max_fields; info->fields and info->batches
 *   say what happened.
 * info (a HOST struct in both variants, nullable): the clipped box, the traversable voxels, the sources with status OK (a voxel
 *   listed twice counts twice), the widest batch, the batches, and over all batches the rounds (launches that found work) and the
 *   tile visits ((tile, flood) pairs relaxed).  n_sources = 0 is no error: nothing is written, info holds the box and
 *   n_traversable.  An empty box: every written cost is -1, every status OUTSIDE, info all zero.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): those of fiesta_hip_reach_field (NaN
 *   clearance, exactly one of lo / hi NULL, both NULL on a hash-block map, a clipped box above 2^28 voxels, connectivity other
 *   than 6 or 26, unknown flag bits, a negative count, result NULL), max_fields < 0, sources NULL with n_sources > 0, targets NULL
 *   with n_targets > 0, n_sources * n_cols > 2^28.  The scratch memory (the cost planes of a batch, item flags and lists, the
 *   bitmap) belongs to the map: grown on demand, freed by fiesta_hip_destroy; a failed allocation is FIESTA_HIP_ERR_NOMEM and leaves
 *   the map usable.  FIESTA_HIP_ERR_STATE: a batch ran more rounds than there are traversable voxels + 1 (a defect, never expected).
 * The field that fiesta_hip_reach_paths RETAINS is left alone: this call neither reads nor writes it, so a reach_field /
 *   reach_paths pair may be interleaved with it.
 * The BATCH that fiesta_hip_leg_paths descends is RETAINED by this call, in the map's scratch memory: the cost planes of all floods,
 *   the clipped box, the connectivity, the per-source status and a copy of the source voxels.  Every call that gets past the
 *   whole-call argument errors above first drops what was retained; a batch is retained when the call then succeeds with
 *   n_sources >= 1, a non-empty clipped box and ALL sources in one batch -- info->batches == 1 says so.  The retained batch is a
 *   SNAPSHOT, as the retained field is: map updates do not invalidate it, and reach_field / reach_paths calls neither read nor
 *   write it.  No output of this call depends on it.
 * fiesta_hip_reach_matrix      host arrays; stages, runs, synchronises, copies back.
 * fiesta_hip_reach_matrix_dev  sources / targets and the arrays the result struct names are device pointers; writes exactly
 *                              n_sources * n_cols costs and nothing beyond them.  Synchronises with the map's stream like
 *                              fiesta_hip_reach_field_dev: the number of rounds depends on the data (one small counter read after
 *                              every eight rounds of a batch). */
#define FIESTA_HIP_REACH_SITE_OK 0
#define FIESTA_HIP_REACH_SITE_OUTSIDE 1 /* source outside the clipped box */
#define FIESTA_HIP_REACH_SITE_BLOCKED 2 /* source inside, not traversable */
typedef struct fiesta_hip_reach_matrix_result { /* every pointer nullable */
  int32_t *cost;                                /* n_sources x n_cols, row-major */
  int32_t *source_status;                       /* per source, FIESTA_HIP_REACH_SITE_* */
  int64_t *source_reached; /* per source: traversable voxels with a finite cost in its flood; 0 unless OK */
} fiesta_hip_reach_matrix_result;
typedef struct fiesta_hip_reach_matrix_info {
  int32_t box_lo[3], box_hi[3]; /* the clipped box, map voxel coordinates, inclusive */
  int64_t n_traversable;
  int64_t n_sources_used; /* sources with status OK; a voxel listed twice counts twice */
  int64_t fields;         /* floods run side by side (the widest batch) */
  int64_t batches;
  int64_t rounds;      /* launches that found work, over all batches */
  int64_t tile_visits; /* (tile, flood) pairs relaxed, over all rounds */
} fiesta_hip_reach_matrix_info;
int fiesta_hip_reach_matrix(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *sources, int64_t n_sources,
                            const int32_t *targets, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                            int32_t max_fields, const fiesta_hip_reach_matrix_result *result, fiesta_hip_reach_matrix_info *info);
int fiesta_hip_reach_matrix_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *sources_dev, int64_t n_sources,
                                const int32_t *targets_dev, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                                int32_t max_fields, const fiesta_hip_reach_matrix_result *result, fiesta_hip_reach_matrix_info *info);

/* ---- site tour: the order in which to visit the sites of a cost matrix, a restart-parallel local search on the device ----
 * What an exploration planner decides after fiesta_hip_reach_matrix: which site to fly to next and in which order to take the
 * rest.  Given a SYMMETRIC cost matrix and a start site, the call returns the order in which to visit every site the start can
 * reach, minimising the summed leg cost, as an open path from the start or (FIESTA_HIP_TOUR_CLOSED) a closed tour back to it.
 * No voxel is read: the call is the same on array-mode and hash-block maps.  No reference counterpart.  fiesta_hip_version() is
 * still 101: detect these two calls by symbol lookup.  Every number is an integer; fiesta_amd.tour_model is the definition.
 * Inputs: cost, n x n int32, row-major with leading dimension ld >= n; 1 <= n <= FIESTA_HIP_TOUR_MAX_SITES; start, a site; flags,
 *   FIESTA_HIP_TOUR_CLOSED or 0; restarts R, 1 <= R <= FIESTA_HIP_TOUR_MAX_RESTARTS; seed; max_moves, the applied moves a restart
 *   may make (0: 8 * m).
 * Sites: an entry c is a CONNECTION iff 0 <= c < INT32_MAX (the reach matrix's convention: -1 is an unusable site, INT32_MAX is
 *   traversable but not reached).  Site j is VISITED iff j == start or cost[start][j] is a connection; every other site is
 *   SKIPPED.  The m visited sites in ascending site index, with the start moved to the front, are the LOCAL indices 0 .. m - 1.
 *   Among visited sites every pair must be a connection and cost[a][b] must equal cost[b][a]; the diagonal is ignored.  A
 *   violation is FIESTA_HIP_ERR_INVALID, found on the device before any search, and nothing is written.  (A square reach matrix
 *   always meets both: one connected component is mutually reachable, and moves are symmetric.)
 * Initial tour of restart r, in local indices: r = 0 is nearest neighbour from index 0 (append the unvisited index with the least
 *   cost from the last one, ties to the lowest index).  r >= 1: t = [0, 1, .., m - 1]; for k = m - 1 down to 2:
 *   j = 1 + rnd(seed, r, k) % k, swap t[k] and t[j]; rnd(seed, r, k) = mix(mix(seed + r * 0x9E3779B97F4A7C15) + k) in uint64
 *   arithmetic, mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31.
 * Local search, best improvement, lengths and deltas in int64: an iteration evaluates every move of the current tour and applies
 *   the one with the most negative delta, ties to the lowest key (type, i, x) compared lexicographically; it stops when no move
 *   has delta < 0, or -- capped -- when one has and max_moves moves were applied already.  C(a, b): the cost between the sites at
 *   tour positions a and b; position m is position 0 of a closed tour; in an open tour it does not exist and every term that
 *   names it is dropped.
 *   type 0, 2-opt(i, j = x), 1 <= i < j <= m - 1: reverses t[i..j];
 *     delta = C(i-1, j) - C(i-1, i) + C(i, j+1) - C(j, j+1).
 *   type L = 1, 2, 3, Or-opt(i, p = x): the segment t[i..e], e = i + L - 1, 1 <= i, e <= m - 1, moves, keeping its orientation, to
 *     directly after position p of the current tour; p = 0 .. m - 1 but not i - 1 <= p <= e;
 *     delta = [C(i-1, e+1) - C(i-1, i) - C(e, e+1)] + [C(p, i) + C(e, p+1) - C(p, p+1)].
 *   The length is an integer and only falls, so the search ends.  The best restart has the least final length, ties to the lowest r.
 * Outputs (every pointer nullable): order[n], the site indices in tour order, the start first: m entries, then -1; site_status[n]:
 *   FIESTA_HIP_TOUR_SITE_VISITED / _SKIPPED; leg_cost[n]: the cost of arriving at order[k] -- leg_cost[0] is 0 for an open tour and
 *   the closing leg for a closed one -- and -1 past the tour; restart_length[R]: every restart's final length.  info (a HOST
 *   struct in both variants, nullable): n_visited = m, the best restart and its length, nn_length (restart 0 before any move),
 *   moves (applied, summed over the restarts) and capped (the restarts stopped by max_moves).  With m <= 2 there is no move and
 *   nothing to search; the call succeeds.  Every output has the same bits for any launch shape, and the bits of
 *   fiesta_amd.tour_model.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): cost NULL, n outside 1 .. 512, start outside
 *   0 .. n - 1, ld < n, R outside 1 .. 4096, unknown flag bits, max_moves < 0.  The scratch memory (the compact matrix of the visited
 *   sites, the restarts' tours and lengths) belongs to the map: grown on demand, freed by fiesta_hip_destroy, touched by no other
 *   call; the field that fiesta_hip_reach_paths RETAINS is left alone.
 * fiesta_hip_site_tour      host arrays; stages, runs, synchronises, copies back.
 * fiesta_hip_site_tour_dev  cost and the arrays the result struct names are device pointers -- the matrix is read where
 *                           fiesta_hip_reach_matrix_dev left it, no copy goes through the host; writes exactly n entries of order,
 *                           site_status and leg_cost and R of restart_length.  Synchronises with the map's stream: m and the two
 *                           error words are read back before the search is launched. */
#define FIESTA_HIP_TOUR_MAX_SITES 512
#define FIESTA_HIP_TOUR_MAX_RESTARTS 4096
#define FIESTA_HIP_TOUR_CLOSED 1
#define FIESTA_HIP_TOUR_SITE_VISITED 0
#define FIESTA_HIP_TOUR_SITE_SKIPPED 1
typedef struct fiesta_hip_tour_result { /* every pointer nullable */
  int32_t *order;                       /* n: site indices in tour order, then -1 */
  int32_t *site_status;                 /* n: FIESTA_HIP_TOUR_SITE_* */
  int32_t *leg_cost;                    /* n: the cost of arriving at order[k], then -1 */
  int64_t *restart_length;              /* R: the final length of every restart */
} fiesta_hip_tour_result;
typedef struct fiesta_hip_tour_info {
  int32_t n_visited;    /* m */
  int32_t best_restart; /* least final length, ties to the lowest r */
  int64_t length;       /* of the returned tour */
  int64_t nn_length;    /* restart 0 before any move */
  int64_t moves;        /* applied, over all restarts */
  int64_t capped;       /* restarts stopped by max_moves */
} fiesta_hip_tour_info;
int fiesta_hip_site_tour(fiesta_hip_map *m, const int32_t *cost, int32_t n, int64_t ld, int32_t start, int32_t flags, int32_t restarts,
                         uint64_t seed, int32_t max_moves, const fiesta_hip_tour_result *result, fiesta_hip_tour_info *info);
int fiesta_hip_site_tour_dev(fiesta_hip_map *m, const int32_t *cost_dev, int32_t n, int64_t ld, int32_t start, int32_t flags, int32_t restarts,
                             uint64_t seed, int32_t max_moves, const fiesta_hip_tour_result *result, fiesta_hip_tour_info *info);

/* ---- reach paths: the paths themselves, extracted from the cost-to-go field on the device ----
 * The last step of the chain frontier voxels -> reachability -> paths -> path cost: fiesta_hip_reach_field says which targets the
 * robot can reach and at what cost, this call descends the cost field from every target to the seed it was reached from and
 * returns the paths in exactly the input form of fiesta_hip_path_clearance[_dev] and fiesta_hip_path_cost[_dev] -- CSR offsets
 * (int64) over n x 3 f64 waypoints in metres -- so the whole chain stays on the device.  A raw path is a staircase of one-voxel
 * moves; FIESTA_HIP_REACH_PATHS_SHORTCUT pulls it tight by line of sight through the flood's own traversable set.  Read-only; no
 * reference counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * The field: either explicit -- `cost` holds ex * ey * ez int32 in fiesta_hip_reach_field's box-local order, box_lo / box_hi (HOST
 *   pointers in both variants) are the inclusive box it covers in map voxel coordinates (fiesta_hip_reach_info.box_lo / box_hi of
 *   the flood that made it; lo[c] <= hi[c], at most 2^28 voxels), connectivity the one it was flooded with -- or RETAINED: cost,
 *   box_lo and box_hi all NULL.  A map retains the field of its last fiesta_hip_reach_field[_dev] call if that call succeeded, its
 *   clipped box was not empty and its cost field lived in the map's own scratch memory (every host-variant call; a _dev call with
 *   result->cost == NULL); any other reach_field call leaves nothing retained.  The host variant of THIS call with an explicit cost
 *   uploads it into that scratch memory: it becomes the retained field, with the box and connectivity as given.  The _dev variant
 *   reads an explicit cost in place and leaves what is retained alone.  With NULLs and nothing retained: FIESTA_HIP_ERR_STATE; with
 *   NULLs and a connectivity other than the retained field's: FIESTA_HIP_ERR_INVALID.
 *   The retained field is a SNAPSHOT: later fiesta_hip_update_occupancy / _update_esdf calls do not invalidate it, and paths run
 *   through space as it was when it was flooded.  Nothing else of the map is read but its resolution and origin, so the call is
 *   the same for dense maps, shards (whose info reports global voxel coordinates: use them) and hash-block maps.
 * Descent: the moves are (dx, dy, dz) over -1, 0, 1 in lexicographic order, those that change one axis (connectivity 6) or any
 *   (26), with weights 3 / 4 / 5 (fiesta_amd.reach_moves).  D[0] is the target.  From D[k] = v with c = cost(v) > 0, D[k + 1] is
 *   v + move for the FIRST move, in that order, whose voxel n lies inside the box and has cost(n) >= 0 and cost(n) + weight == c.
 *   The descent ends at cost 0 after L moves.  Every step lowers the cost by at least 3, so it ends after at most c / 3 steps
 *   whatever the array holds.  A step reads every neighbour its moves name that lies inside the box; if none qualifies, or one of
 *   them (or the target itself) has a cost below -1, the path is BROKEN -- the field is no fixed point for this connectivity.  No
 *   read ever leaves the box.
 * visible(p, q), for map voxels p and q: |p - q| summed over the axes is at most 4095, and every voxel that the reference traversal
 *   (Raycast, src/raycast.cpp:56-158: the ray cast's and the ray query's, without clipping box and without the 1500-voxel
 *   exception) emits from a = p + 0.5 to b = q + 0.5 -- f64, exact, in map voxel units, nothing is divided by the resolution --
 *   its last one included, lies inside the box and has cost >= 0.  This is NOT the ray query's walk W: W replaces the traversal's
 *   last voxel by floor(b), while between two centres the unsubstituted sequence followed by q is a 6-connected chain, so a
 *   visible segment cuts no corner of a voxel that is not traversable.
 * Anchors: without SHORTCUT every index 0 .. L (max_span is ignored).  With SHORTCUT (max_span >= 1):
 *     K = [0]; i = 0
 *     while i < L:  j = i + 1;  while j < L and j + 1 - i <= max_span and visible(D[i], D[j + 1]): j += 1;  K.append(j); i = j
 *   (the first move from an anchor is never tested: it is a legal move of the flood; max_span = 1 reproduces the raw path).
 * Outputs, per target p (targets: n_targets x 3 int32 map voxels):
 *   offsets        int64, n_targets + 1: CSR over the waypoints, the TRUE totals whatever capacity is; REQUIRED
 *   waypoints_vox  int32 x 3 per waypoint, map voxel coordinates; a path's waypoints are D[k] for k in K IN REVERSE: from the seed it
 *                  reached to the target
 *   waypoints_pos  f64 x 3 per waypoint, metres: ((double)v[c] + 0.5) * resolution + origin[c] (Vox2Pos)
 *   status         FIESTA_HIP_REACH_PATH_*; n_moves: L.  A target of cost 0 yields one waypoint and 0 moves; every status other
 *                  than OK yields no waypoint and n_moves -1.
 *   Waypoints with a global index below `capacity` are written, nothing beyond it is touched: call with capacity 0 (the waypoint
 *   arrays may then be NULL) and read offsets[n_targets] to size the buffers.  n_targets = 0 writes offsets[0] = 0.
 *   All arithmetic is integer, the traversal and the positions apart: every output has the same bits for any launch shape, and the
 *   bits of fiesta_amd.reach_paths_model (the definition in plain Python).
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): result or result->offsets NULL,
 *   connectivity other than 6 or 26, unknown flag bits, SHORTCUT with max_span < 1, a negative count or capacity, targets NULL
 *   with n_targets > 0, not all or none of cost / box_lo / box_hi given, an explicit box with lo[c] > hi[c] or more than 2^28 voxels.
 * fiesta_hip_reach_paths      host arrays; stages through the path queries' buffers, runs, copies back min(total, capacity)
 *                             waypoints, synchronises.
 * fiesta_hip_reach_paths_dev  cost, targets and the result's arrays are device pointers; only enqueued on the map's stream (count,
 *                             scan, write: no data-dependent allocation), unlike fiesta_hip_reach_field_dev. */
#define FIESTA_HIP_REACH_PATHS_SHORTCUT 1
#define FIESTA_HIP_REACH_PATH_OK 0        /* status values */
#define FIESTA_HIP_REACH_PATH_OUTSIDE 1   /* target outside the field's box */
#define FIESTA_HIP_REACH_PATH_BLOCKED 2   /* cost -1: not traversable */
#define FIESTA_HIP_REACH_PATH_UNREACHED 3 /* cost INT32_MAX */
#define FIESTA_HIP_REACH_PATH_BROKEN 4    /* the descent met a voxel with no predecessor, or a cost below -1 */
typedef struct fiesta_hip_reach_paths_result {
  int64_t *offsets;       /* n_targets + 1; REQUIRED */
  int32_t *waypoints_vox; /* capacity x 3, map voxel coordinates; nullable */
  double *waypoints_pos;  /* capacity x 3, metres; nullable */
  int32_t *status;        /* per target; nullable */
  int32_t *n_moves;       /* per target; nullable */
} fiesta_hip_reach_paths_result;
int fiesta_hip_reach_paths(fiesta_hip_map *m, const int32_t *cost, const int32_t box_lo[3], const int32_t box_hi[3], const int32_t *targets,
                           int64_t n_targets, int32_t connectivity, int32_t flags, int32_t max_span, int64_t capacity,
                           const fiesta_hip_reach_paths_result *result);
int fiesta_hip_reach_paths_dev(fiesta_hip_map *m, const int32_t *cost_dev, const int32_t box_lo[3], const int32_t box_hi[3],
                               const int32_t *targets_dev, int64_t n_targets, int32_t connectivity, int32_t flags, int32_t max_span,
                               int64_t capacity, const fiesta_hip_reach_paths_result *result);

/* ---- leg paths: the legs of a tour, extracted from the floods the reach matrix has just run ----
 * Where the two halves of the planner chain meet: fiesta_hip_reach_matrix -> fiesta_hip_site_tour gives an ORDER of sites and integer
 * leg costs, fiesta_hip_path_corridor -> fiesta_hip_corridor_bounds -> fiesta_hip_path_refine take PATHS.  This call gives the way
 * along every leg without flooding anything again: it descends the cost planes that the map's last fiesta_hip_reach_matrix call
 * RETAINED (see there: that call succeeded, n_sources >= 1, a non-empty box, info->batches == 1).  Read-only; no reference
 * counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.  fiesta_amd.leg_paths_model is the
 * definition.
 * Legs: leg k runs from site from[k], an index into the retained batch's sources, to site to[k], or to map voxel
 *   to_vox[3k .. 3k + 2]; exactly one of to and to_vox is non-NULL when n_legs > 0.  The legs of a tour need no array to be built:
 *   with `order` and n_visited of fiesta_hip_site_tour, from = order, to = order + 1, n_legs = n_visited - 1 (a closed tour's last
 *   leg, order[n_visited - 1] -> order[0], is one more leg of its own).  flags: 0 or FIESTA_HIP_REACH_PATHS_SHORTCUT; max_span as
 *   in fiesta_hip_reach_paths.  There is no connectivity argument: the retained batch's is used.
 * status[k], in this order of precedence: FIESTA_HIP_LEG_BAD_INDEX, from[k] or to[k] outside 0 .. n_sources - 1;
 *   FIESTA_HIP_LEG_NO_SOURCE, source from[k] is not FIESTA_HIP_REACH_SITE_OK in the retained batch; else the FIESTA_HIP_REACH_PATH_*
 *   status (0 .. 4) of fiesta_hip_reach_paths for the leg's target on the source's plane.
 * Path: for status OK, bit for bit what fiesta_hip_reach_paths returns for that target on the explicit field of
 *   fiesta_hip_reach_field with seeds = {source from[k]} and the matrix call's box, clearance, flags and connectivity, with the
 *   same flags and max_span: stored SOURCE FIRST, TARGET LAST, so consecutive legs of a tour concatenate into the route (the last
 *   waypoint of one leg is the first of the next).  from[k] == to[k] yields one waypoint and 0 moves; a leg that is not OK has no
 *   waypoint and n_moves -1.
 * cost[k]: the source's plane at the target voxel -- -1 outside the box or not traversable, INT32_MAX not reached -- and -1 for
 *   NO_SOURCE and BAD_INDEX; with `to` therefore cost[from[k]][to[k]] of the matrix call's square form, bit for bit.
 * offsets (REQUIRED, n_legs + 1, always the true totals), waypoints_vox, waypoints_pos and capacity behave exactly as in
 *   fiesta_hip_reach_paths: entries below `capacity` are written, nothing beyond it is touched, capacity 0 sizes the buffers.
 *   n_legs = 0 is no error: offsets[0] = 0.  info (a HOST struct in both variants, nullable): what is retained -- the clipped box,
 *   the connectivity and the number of sources -- filled from the host-side record.
 * Whole-call errors, FIESTA_HIP_ERR_INVALID, checked before the map handle is looked at: result or result->offsets NULL, a negative
 *   n_legs or capacity, unknown flag bits, SHORTCUT with max_span < 1, from NULL with n_legs > 0, both or neither of to / to_vox
 *   with n_legs > 0.  FIESTA_HIP_ERR_STATE: the map retains no batch; the message says why (no fiesta_hip_reach_matrix call yet, the
 *   last one ran more than one batch -- lower the box or raise max_fields -- or it had nothing to keep).  Nothing is written then.
 * fiesta_hip_leg_paths      host arrays; stages, runs, copies back min(total, capacity) waypoints, synchronises.
 * fiesta_hip_leg_paths_dev  from / to / to_vox and the result's arrays are device pointers (from and to may be views into the order
 *                           array where fiesta_hip_site_tour_dev left it); only enqueued on the map's stream (count, scan, write),
 *                           like fiesta_hip_reach_paths_dev. */
#define FIESTA_HIP_LEG_NO_SOURCE 5 /* the leg's source is not FIESTA_HIP_REACH_SITE_OK in the retained batch */
#define FIESTA_HIP_LEG_BAD_INDEX 6 /* from, or to, outside 0 .. n_sources - 1 */
typedef struct fiesta_hip_leg_paths_result {
  int64_t *offsets;       /* n_legs + 1, CSR; REQUIRED: always the true totals */
  int32_t *waypoints_vox; /* capacity x 3, map voxel coordinates; nullable */
  double *waypoints_pos;  /* capacity x 3, metres (Vox2Pos); nullable */
  int32_t *status;        /* per leg; nullable */
  int32_t *n_moves;       /* per leg; nullable */
  int32_t *cost;          /* per leg; nullable */
} fiesta_hip_leg_paths_result;
typedef struct fiesta_hip_leg_paths_info {
  int32_t box_lo[3], box_hi[3]; /* the retained batch's clipped box, map voxel coordinates, inclusive */
  int32_t connectivity;
  int32_t reserved;
  int64_t n_sources;
} fiesta_hip_leg_paths_info;
int fiesta_hip_leg_paths(fiesta_hip_map *m, const int32_t *from, const int32_t *to, const int32_t *to_vox, int64_t n_legs, int32_t flags,
                         int32_t max_span, int64_t capacity, const fiesta_hip_leg_paths_result *result, fiesta_hip_leg_paths_info *info);
int fiesta_hip_leg_paths_dev(fiesta_hip_map *m, const int32_t *from_dev, const int32_t *to_dev, const int32_t *to_vox_dev, int64_t n_legs,
                             int32_t flags, int32_t max_span, int64_t capacity, const fiesta_hip_leg_paths_result *result,
                             fiesta_hip_leg_paths_info *info);

/* ---- free-space corridors: box inflation around voxels, and a corridor of overlapping boxes along voxel polylines ----
 * What a trajectory optimiser takes after the chain frontier voxels -> reachability -> reach paths: not a voxel staircase but a
 * SAFE FLIGHT CORRIDOR, a short sequence of overlapping axis-aligned boxes of traversable space around the path, inside which a
 * polynomial or B-spline is fitted under linear constraints.  fiesta_hip_free_boxes inflates one box around every seed voxel;
 * fiesta_hip_path_corridor builds the corridor of every polyline of a CSR batch, in exactly the form fiesta_hip_reach_paths writes
 * (waypoints_vox and offsets), so the whole chain stays on the device.  Read-only; no reference counterpart.
 * fiesta_hip_version() is still 101: detect these four calls by symbol lookup.  fiesta_amd.free_box_model and
 * fiesta_amd.corridor_model are the definition.
 * Window W: lo / hi are HOST pointers in both variants, an inclusive voxel box in map voxel coordinates; both may be NULL on every
 *   store.  A dense map or shard intersects the box with its own array; with both NULL, W is the whole array.  A hash-block map has
 *   no outside: a given box is clamped to +-2^30, and with both NULL W is unbounded (every voxel within +-2^30, as far as
 *   coordinates go anywhere in this interface).  An empty W, or lo[c] > hi[c], is no error: every seed then reads OUTSIDE and every
 *   path with a waypoint BLOCKED at its first.
 * traversable(v), for v in W: exactly fiesta_hip_reach_field's -- free (observed and not Exist) and, only if min_clearance > 0,
 *   GetDistance(Vector3i v) >= min_clearance with the voxel query's own f64 value; with flags & FIESTA_HIP_CORRIDOR_THROUGH_UNKNOWN
 *   a never-observed voxel is traversable too (a tile without a page counts as never observed).  Outside W a voxel is not
 *   traversable.  With min_clearance <= 0 the distance field is not read.  The map is read as it stands.
 * inflate(lo0, hi0, max_grow): faces f = 0 .. 5 are -x, +x, -y, +y, -z, +z (the bit order of the frontier mask), axis a = f >> 1.
 *     lo, hi = lo0, hi0;  g[0..5] = 0;  stop[0..5] = 0
 *     while some stop[f] == 0:
 *       for f in 0 .. 5 in this order, skipping faces with stop[f] != 0:
 *         if g[f] == max_grow:                     stop[f] = LIMIT (3);   continue
 *         c = hi[a] + 1 (odd f)  or  lo[a] - 1 (even f)
 *         if c lies outside W on axis a:           stop[f] = EDGE (2);    continue
 *         slab = the voxels with coordinate c on axis a and the CURRENT [lo, hi] on the other two axes (extensions made earlier
 *                in the same round included)
 *         if some slab voxel is not traversable:   stop[f] = BLOCKED (1); continue
 *         extend the box to c on that side;  g[f] += 1
 *   Each step grows or stops a face: at most 6 * (max_grow + 1) face tests, and the result is unique.  max_grow lies in
 *   0 .. FIESTA_HIP_CORRIDOR_MAX_GROW.
 * fiesta_hip_free_boxes, per seed (seeds: n x 3 int32 map voxels); every pointer of the result struct is nullable:
 *   box      int32 x 6: lo xyz, then hi xyz, inclusive -- inflate([seed, seed])
 *   box_pos  f64 x 6: (double)lo[c] * resolution + origin[c], then ((double)hi[c] + 1.0) * resolution + origin[c]
 *   stop     uint8 x 6: the stop code of each face
 *   volume   int64: the number of voxels in the box
 *   status   int32: FIESTA_HIP_FREE_BOX_OK; _OUTSIDE: the seed is not in W; _BLOCKED: it is not traversable.  For any status other
 *            than OK box is INT32_MIN x 6, box_pos NaN, stop 0 and volume 0; the other seeds are unaffected.
 *   Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable; each is checked before the map handle is
 *   looked at): min_clearance is NaN, exactly one of lo / hi is NULL, max_grow out of range, unknown flag bits, a negative n, seeds
 *   NULL with n > 0, result NULL.  n = 0 does nothing.
 * fiesta_hip_path_corridor: waypoints_vox, n_waypoints x 3 int32, and offsets, int64 x (n_paths + 1) in CSR form.
 *   Chain: for waypoints p -> q, walk(p, q) is the voxel sequence of the reference traversal from centre to centre
 *     (fiesta_amd.reach_walk: what visible() of fiesta_hip_reach_paths walks).  Candidate A is walk(p, q) followed by q unless q is
 *     already its last element; candidate B is the reverse of (walk(q, p) followed by p, with the same exception).  Both are
 *     6-connected monotone chains of 1 + |p - q|_1 voxels from p to q.  The segment uses A if all its voxels are traversable,
 *     otherwise B if all of B's are, otherwise the path is BLOCKED there.  (For a diagonal move of a 26-connected path A and B
 *     are two of the axis orders, so a path may round a wall corner on whichever side is free; for a path shortcut by
 *     fiesta_hip_reach_paths B is exactly the sequence its visible() tested, because its output runs from the seed to the target.)
 *   Corridor of a path w[0 .. m - 1]:
 *     visit(v):  if a box exists and v lies in the LAST box: prev = v; return
 *                seed box = [v, v] if prev is none, else the bounding box of {prev, v} (two 6-adjacent traversable voxels)
 *                append inflate(seed box); entry = v's chain index; prev = v
 *     w[0] outside W or not traversable: BLOCKED at segment -1 with no boxes, blocked_vox = w[0].  Otherwise visit it with chain
 *     index 0; then for each segment j with w[j] != w[j + 1] choose A or B and visit its voxels after the first in order, the chain
 *     indices counting on.  A BLOCKED path keeps the boxes made so far and reports blocked_segment = j and blocked_vox = the first
 *     voxel of A that is not traversable.  A path is INVALID, and yields no box, if a waypoint has a coordinate beyond +-2^30 or a
 *     segment has |p - q|_1 > 4095 and -- in the _dev variant only -- if offsets[p + 1] < offsets[p] or its range leaves
 *     [0, n_waypoints]; the host variant refuses such offsets as a whole-call error.  An empty path is OK with no box.
 *   Outputs, per box: boxes (int32 x 6), boxes_pos (f64 x 6), stop (uint8 x 6) as above, and entry (int32); per path: status
 *     (FIESTA_HIP_CORRIDOR_OK / _INVALID / _BLOCKED), n_chain (the chain voxels visited), blocked_segment (-1 if none), blocked_vox
 *     (INT32_MIN x 3 if none); offsets, int64 x (n_paths + 1), REQUIRED: CSR over the boxes, the TRUE totals whatever capacity is
 *     (n_paths = 0 writes offsets[0] = 0).  Boxes with a global index below `capacity` are written and nothing beyond is touched:
 *     call with capacity 0 (the per-box arrays may then be NULL) and read offsets[n_paths] to size the buffers.
 *   Whole-call errors: those of fiesta_hip_free_boxes (with waypoints_vox NULL while n_waypoints > 0, a negative count or capacity),
 *     offsets NULL, result or result->offsets NULL, and in the host variant offsets that do not start at or above 0, decrease, or
 *     end above n_waypoints.
 * Guarantees: (1) every voxel of every box is traversable and lies inside W; (2) consecutive boxes of a path share at least one
 *   voxel; (3) every visited chain voxel lies in the box that was last when it was visited; (4) every stop code is truthful for the
 *   final box -- LIMIT: that side grew max_grow, EDGE: the next plane leaves W, BLOCKED: the slab beyond that face over the final
 *   cross-section holds a voxel that is not traversable; (5) max_grow = 0 returns the seed boxes; (6) all arithmetic is integer
 *   apart from the traversal, the clearance comparison and *_pos: every output has the same bits for any launch shape and
 *   scheduling, and the bits of fiesta_amd.free_box_model / fiesta_amd.corridor_model.
 * fiesta_hip_free_boxes / fiesta_hip_path_corridor          host arrays; stage, run, synchronise, copy back (the corridor call
 *                                                           copies min(total, capacity) boxes).
 * fiesta_hip_free_boxes_dev / fiesta_hip_path_corridor_dev  seeds / waypoints, offsets and the result's arrays are device pointers;
 *                                                           only enqueued on the map's stream (the corridor: count, scan, write;
 *                                                           no host round trip, no data-dependent allocation).  A hash-block map
 *                                                           first rebuilds its page table if its page set changed, as every
 *                                                           query does.  Shards answer for their own array; there is no
 *                                                           shard-group call. */
#define FIESTA_HIP_CORRIDOR_THROUGH_UNKNOWN 1
#define FIESTA_HIP_CORRIDOR_MAX_GROW 256
#define FIESTA_HIP_CORRIDOR_STOP_BLOCKED 1 /* stop codes of a face */
#define FIESTA_HIP_CORRIDOR_STOP_EDGE 2
#define FIESTA_HIP_CORRIDOR_STOP_LIMIT 3
#define FIESTA_HIP_FREE_BOX_OK 0      /* status values of fiesta_hip_free_boxes */
#define FIESTA_HIP_FREE_BOX_OUTSIDE 1 /* seed not in W */
#define FIESTA_HIP_FREE_BOX_BLOCKED 2 /* seed not traversable */
#define FIESTA_HIP_CORRIDOR_OK 0      /* status values of fiesta_hip_path_corridor */
#define FIESTA_HIP_CORRIDOR_INVALID 1 /* a segment too long, a coordinate too far, bad offsets (_dev) */
#define FIESTA_HIP_CORRIDOR_BLOCKED 2 /* the first waypoint, or both chains of a segment, are not traversable */
typedef struct fiesta_hip_free_boxes_result { /* every pointer nullable */
  int32_t *box;                               /* n x 6: lo xyz, hi xyz */
  double *box_pos;                            /* n x 6, metres */
  uint8_t *stop;                              /* n x 6 */
  int64_t *volume;                            /* n */
  int32_t *status;                            /* n */
} fiesta_hip_free_boxes_result;
typedef struct fiesta_hip_corridor_result {
  int64_t *offsets;         /* n_paths + 1; REQUIRED */
  int32_t *boxes;           /* capacity x 6; nullable */
  double *boxes_pos;        /* capacity x 6, metres; nullable */
  uint8_t *stop;            /* capacity x 6; nullable */
  int32_t *entry;           /* capacity; nullable */
  int32_t *status;          /* per path; nullable */
  int32_t *n_chain;         /* per path; nullable */
  int32_t *blocked_segment; /* per path; nullable */
  int32_t *blocked_vox;     /* per path x 3; nullable */
} fiesta_hip_corridor_result;
int fiesta_hip_free_boxes(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds, int64_t n, double min_clearance,
                          int32_t max_grow, int32_t flags, const fiesta_hip_free_boxes_result *result);
int fiesta_hip_free_boxes_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds_dev, int64_t n,
                              double min_clearance, int32_t max_grow, int32_t flags, const fiesta_hip_free_boxes_result *result);
int fiesta_hip_path_corridor(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *waypoints_vox, int64_t n_waypoints,
                             const int64_t *offsets, int64_t n_paths, double min_clearance, int32_t max_grow, int32_t flags,
                             int64_t capacity, const fiesta_hip_corridor_result *result);
int fiesta_hip_path_corridor_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *waypoints_vox_dev,
                                 int64_t n_waypoints, const int64_t *offsets_dev, int64_t n_paths, double min_clearance, int32_t max_grow,
                                 int32_t flags, int64_t capacity, const fiesta_hip_corridor_result *result);

/* ---- path refinement: bounded descent of the waypoints of a CSR batch, the whole loop on the device ----
 * The optimiser's loop that path cost (the evaluator) and the corridors (the constraints) were made for: every path of the batch
 * takes `iterations` projected-gradient steps on an obstacle cost plus a smoothness cost, every waypoint clamped to a box of its
 * own -- such as the corridor box it lies in (fiesta_amd.corridor_bounds).  The paths are independent: one launch runs every
 * path's whole loop, its positions resident on chip; no host round trip, no global synchronisation.  Read-only on the map; no
 * reference counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * fiesta_amd.path_refine_model (numpy) is the definition.
 * Input: waypoints and offsets are path clearance's CSR polylines.  bounds is nullable: n_waypoints x 6 f64, lo xyz then hi xyz,
 *   metres; +-inf is allowed and means free on that side; bounds NULL means every waypoint is free.  The first and the last
 *   waypoint of a path never move, and their bounds rows are not read.
 * The sample: for a waypoint x, (d, g) is fiesta_hip_get_dist_grad at x, bit for bit (dense maps, a single shard, hash-block
 *   maps; outside a dense map -1 with zero gradient).  phi and gamma[c] are exactly path cost's:
 *   if d < margin:  e = margin - d;  phi = e * e;  psi = -2.0 * e;  gamma[c] = psi * g[c]      else phi = 0, gamma = 0.
 * One iteration of a path w[0 .. m-1] is a Jacobi step: everything is computed from the positions of the previous iteration, in
 *   f64, each operation rounded once (the library is built with -ffp-contract=off), in exactly this order:
 *     a_j[c] = (w[j-1][c] - 2.0 * w[j][c]) + w[j+1][c]   for 1 <= j <= m-2,   a_0 = a_{m-1} = 0
 *   and for every interior i (1 <= i <= m-2) and component c:
 *     s = (a_{i-1}[c] - 2.0 * a_i[c]) + a_{i+1}[c]
 *     G = w_obstacle * gamma_i[c] + (2.0 * w_smooth) * s
 *     delta = alpha * G
 *     if (delta > max_step) delta = max_step;   if (delta < -max_step) delta = -max_step;
 *     x = w[i][c] - delta
 *     if (x < lo) x = lo;   if (x > hi) x = hi;
 *     move = |x - w[i][c]|
 *   Both clamps are comparisons, not fmin / fmax: the sign of a zero is ruled.  last_move is the maximum of move over the interior
 *   waypoints and components of the iteration (a maximum of non-negative numbers: no order).  If last_move <= tolerance the path
 *   stops after this iteration (with tolerance 0: only after an iteration that moved nothing, which changes no later position);
 *   result.iterations is the number of iterations run.  With iterations = 0, or m <= 2, nothing moves: last_move 0, iterations 0.
 *   G is the exact derivative with respect to w[i][c] of
 *     J = sum over i = 1 .. m-2 of e_i,   e_i = w_obstacle * phi_i + w_smooth * ((a_i[0]*a_i[0] + a_i[1]*a_i[1]) + a_i[2]*a_i[2])
 *   wherever the field's interpolant is differentiable.
 *   Stability: the smoothness operator (the second difference applied twice) has eigenvalues up to 16, so a caller wants
 *   alpha * w_smooth < 1/16; max_step bounds the motion per component and iteration whatever the weights are.
 * Outputs; every pointer of the result is nullable:
 *   waypoints (x3)  n_waypoints rows, every one written by every call: the rows of a valid path get its final positions, every
 *                   other row (gaps of a device batch's offsets, INVALID paths) equals the input row.  result.waypoints may be
 *                   exactly the input pointer (in place) or disjoint from it; any other overlap is the caller's error and is not
 *                   detected.
 *   cost (x2)       per path: J at the input positions, J at the final positions.  Every term e_i is bit-identical on the device
 *                   and in the model; the order of the sum is left free, but it is fixed by the call's arguments (it follows the
 *                   path's length alone).  Two orders differ by at most (n + 16) * 2^-52 * A, n the number of terms, A the sum of
 *                   their magnitudes (path cost's bound).  No floating-point atomics: the same call gives the same bits.
 *   last_move       per path: of the last iteration run
 *   iterations      per path: iterations actually run
 *   n_below         per path, over all m final waypoints, ends included: those with d < margin (strictly); exact
 *   min_dist        per path, over the same waypoints: the minimum d; exact; an empty path gives 0 and +inf
 *   status          per path: FIESTA_HIP_REFINE_OK, or _INVALID: a non-finite waypoint or a coordinate beyond +-2^40; more than
 *                   FIESTA_HIP_REFINE_MAX_WAYPOINTS waypoints; an interior bounds row that holds a NaN or has lo > hi; in the _dev
 *                   variant only, offsets that break path clearance's offset rules.  An INVALID path gives cost NaN, NaN,
 *                   last_move NaN, iterations -1, n_below -1, min_dist NaN, and its rows equal the input; the other paths are
 *                   unaffected.
 *   With the parameter and coordinate limits every intermediate is finite.  Everything except cost has the bits of the model for
 *   any launch shape and scheduling.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable; each is checked before the map handle is
 *   looked at): a parameter outside its range, flags != 0, a NULL waypoints, offsets, params or result, negative counts, more
 *   than 2^30 paths, and in the host variant offsets that break the CSR rules (offsets[0] = 0, non-decreasing, offsets[n_paths] =
 *   n_waypoints).  n_paths = 0 does nothing.
 * fiesta_hip_path_refine      host pointers; stages, runs, synchronises (no host route for small batches: always the device).
 * fiesta_hip_path_refine_dev  waypoints, offsets, bounds and the result's arrays are device pointers (the two structs themselves
 *                             are host objects); only enqueued on the map's stream: the row copy, the offset check, the kernels.
 *                             Shards answer for their own array; there is no shard-group call. */
#define FIESTA_HIP_REFINE_MAX_WAYPOINTS 1024   /* per path */
#define FIESTA_HIP_REFINE_MAX_ITERATIONS 1024
#define FIESTA_HIP_REFINE_OK 0
#define FIESTA_HIP_REFINE_INVALID 1
typedef struct fiesta_hip_refine_params {
  double margin;      /* metres; finite, |margin| <= 2^20 */
  double w_obstacle;  /* finite, 0 .. 2^20 */
  double w_smooth;    /* finite, 0 .. 2^20 */
  double alpha;       /* step size; finite, > 0, <= 2^20 */
  double max_step;    /* metres per component and iteration; finite, > 0, <= 2^20 */
  double tolerance;   /* metres; finite, >= 0; 0: never stop early */
  int32_t iterations; /* 0 .. FIESTA_HIP_REFINE_MAX_ITERATIONS */
  int32_t flags;      /* 0; any other value is an error */
} fiesta_hip_refine_params;
typedef struct fiesta_hip_refine_result { /* every pointer nullable */
  double *waypoints;   /* n_waypoints x 3: the refined positions */
  double *cost;        /* n_paths x 2: J before, J after */
  double *last_move;   /* n_paths */
  int32_t *iterations; /* n_paths: iterations actually run */
  int64_t *n_below;    /* n_paths */
  double *min_dist;    /* n_paths */
  int32_t *status;     /* n_paths */
} fiesta_hip_refine_result;
int fiesta_hip_path_refine(fiesta_hip_map *m, const double *waypoints, int64_t n_waypoints, const int64_t *offsets, int64_t n_paths,
                           const double *bounds, const fiesta_hip_refine_params *params, const fiesta_hip_refine_result *result);
int fiesta_hip_path_refine_dev(fiesta_hip_map *m, const double *waypoints_dev, int64_t n_waypoints, const int64_t *offsets_dev,
                               int64_t n_paths, const double *bounds_dev, const fiesta_hip_refine_params *params,
                               const fiesta_hip_refine_result *result);

/* ---- corridor bounds: per waypoint of a voxel polyline the box fiesta_hip_path_refine clamps it to, on the device ----
 * The link between fiesta_hip_path_corridor and fiesta_hip_path_refine: it turns a corridor into the `bounds` argument of the
 * refinement, and says per path whether refining inside those bounds is safe.  It reads no voxel: a pure function of the path
 * batch and the corridor arrays (the map lends its stream and scratch), the same on array and hash maps.  No reference counterpart.
 * fiesta_hip_version() is still 101: detect these two calls by symbol lookup.  fiesta_amd.corridor_bounds_model (numpy) is the
 * definition.
 * Inputs:
 *   waypoints_vox  int32 x 3 x n_waypoints.
 *   offsets        int64 x (n_paths + 1): the CSR batch that fiesta_hip_path_corridor took.
 *   the corridor call's outputs for that batch: box_offsets, int64 x (n_paths + 1); boxes, int32 x 6; boxes_pos, f64 x 6; entry,
 *                  int32; status, int32 per path.
 *   n_boxes        the number of box rows actually present in the per-box arrays: min(total, the corridor call's capacity).
 *   inset          f64, metres, finite and >= 0.
 *   flags          0 or FIESTA_HIP_BOUNDS_VOID_BROKEN.
 * Per path p with waypoint range [o0, o1) and box range [b0, b1):
 *   1. The chain index is c_0 = 0, c_{i+1} = c_i + |w_{i+1} - w_i|_1, accumulated in int64.
 *   2. b(i) is the last box of the path with entry <= c_i.
 *   3. ok = (status == FIESTA_HIP_CORRIDOR_OK).  It is cleared if some b(i+1) > b(i) + 1.
 *   4. ok is also cleared if b(1) = b(0) + 1 and w_0 lies outside the integer box b(0) + 1.
 *   5. Row i is boxes_pos[b(i)].
 *   6. On an ok path, where b(i+1) = b(i) + 1, row i is intersected with boxes_pos[b(i) + 1]: lo is the componentwise larger, hi
 *      the componentwise smaller.  Both are written as comparisons, a > b ? a : b and a < b ? a : b (a: row i, b: the other box),
 *      so that the result is ruled bit for bit.
 *   7. Then inset is subtracted from the three upper faces of every row: one f64 subtraction with no contraction.
 * Special cases:
 *   A path with waypoints but no box gets NaN rows.  An empty path writes nothing, and its ok follows its status.
 *   With flags & FIESTA_HIP_BOUNDS_VOID_BROKEN every row of a path that is not ok is NaN: fiesta_hip_path_refine then reports that
 *   path INVALID and leaves it alone, so the chain stays on the device with no host-side masking.
 *   The entries of a path are trusted to be non-decreasing and to start at 0, as the corridor call writes them.  Whatever the
 *   entries hold, every index is clamped into [b0, b1): no read ever leaves the arrays.
 * Outputs; every pointer of the result is nullable:
 *   bounds  f64 x 6 per waypoint (lo xyz, hi xyz): exactly the bounds argument of fiesta_hip_path_refine.
 *   ok      int32 per path.
 *   box     int64 per waypoint: the global index of b(i), or -1 where there is none (which box constrains which waypoint).
 * _dev only: no whole-call refusal of offsets is possible on the device.  A path whose waypoint offsets break path clearance's
 *   offset rule (its start is not the running maximum of the in-range entries before it, or its range is reversed or leaves
 *   [0, n_waypoints]) gets ok = 0, and so does a path whose box range decreases, is negative, or ends above n_boxes (a truncated
 *   corridor).  Such a path reads nothing and writes no row.  The call first fills bounds with NaN and box with -1, so rows that
 *   belong to no valid path are NaN / -1 and deterministic.
 * Host variant: it refuses such offsets (offsets[0] != 0, decreasing, offsets[n_paths] != n_waypoints; a box range that decreases,
 *   is negative or ends above n_boxes) as a whole-call error.  It stages, enqueues exactly what _dev enqueues, and synchronises once
 *   (no host route for small batches: always the device).
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable; each is checked before the map handle is
 *   looked at): negative counts, more than 2^30 paths; a required input NULL while its count is > 0 (waypoints_vox: n_waypoints;
 *   offsets, box_offsets, status: n_paths; boxes, boxes_pos, entry: n_boxes); result NULL; inset NaN, negative or infinite; unknown
 *   flag bits.  n_paths = 0 does nothing.
 * Guarantees: every output has the model's bits for any launch shape and scheduling (integers, comparisons and one subtraction; no
 *   atomics).  On inputs that fiesta_amd.corridor_bounds accepts, holding no negative zero, and with the same explicit inset,
 *   bounds equals its result bit for bit and ok equals it exactly.
 * fiesta_hip_corridor_bounds      host arrays.
 * fiesta_hip_corridor_bounds_dev  every array, input and output, is a device pointer (the result struct itself is a host object);
 *                                 only enqueued on the map's stream: the fill, the offset check, one kernel.  The outputs may
 *                                 feed fiesta_hip_path_refine_dev on the same map with nothing in between.  There is no shard-group
 *                                 call. */
#define FIESTA_HIP_BOUNDS_VOID_BROKEN 1
typedef struct fiesta_hip_bounds_result { /* every pointer nullable */
  double *bounds; /* n_waypoints x 6: lo xyz, hi xyz, metres */
  int32_t *ok;    /* n_paths */
  int64_t *box;   /* n_waypoints */
} fiesta_hip_bounds_result;
int fiesta_hip_corridor_bounds(fiesta_hip_map *m, const int32_t *waypoints_vox, int64_t n_waypoints, const int64_t *offsets, int64_t n_paths,
                               const int64_t *box_offsets, const int32_t *boxes, const double *boxes_pos, const int32_t *entry,
                               const int32_t *status, int64_t n_boxes, double inset, int32_t flags, const fiesta_hip_bounds_result *result);
int fiesta_hip_corridor_bounds_dev(fiesta_hip_map *m, const int32_t *waypoints_vox_dev, int64_t n_waypoints, const int64_t *offsets_dev,
                                   int64_t n_paths, const int64_t *box_offsets_dev, const int32_t *boxes_dev, const double *boxes_pos_dev,
                                   const int32_t *entry_dev, const int32_t *status_dev, int64_t n_boxes, double inset, int32_t flags,
                                   const fiesta_hip_bounds_result *result);

/* ---- path timing: clearance-limited speed profiles and travel times of a CSR batch of polylines, on the device ----
 * Every other cost of the planner chain is a length; this call says how long a path TAKES.  The robot brakes where the distance
 * field says obstacles are near, slows at bends, starts and ends at given speeds (rest by default) and changes speed no faster
 * than its acceleration limit allows.  Per path the call returns the travel time and the slowest sample, per waypoint a time stamp
 * and a speed.  The paths are independent: one launch runs every path's whole computation.  Read-only on the map; no reference
 * counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.  fiesta_amd.path_timing_model (numpy) is
 * the definition.
 * Input: waypoints and offsets are path clearance's CSR polylines; params: every field f64 --
 *   step finite, > 0; margin finite, >= 0; v_max finite, > 0; v_min finite, 0 < v_min <= v_max; a_max finite, > 0; corner_dev in
 *   metres, > 0, +inf switches the corner rule off; v_start and v_end finite, >= 0.
 * Samples: path clearance's, by the same rule and with the same indices: per segment j of a path of m waypoints d[c] = b[c] - a[c],
 *   L_j, S_j, Sd_j = (double)S_j; n = sum S + 1 samples, sample 0 of segment i is waypoint i, the final sample is the last waypoint.
 *   A sample's value d is fiesta_hip_get_dist_grad's at its position, bit for bit (dense maps, a single shard, hash-block maps; -1
 *   outside a dense map, +10000 at unobserved corners).
 * The rule, in f64, every operation rounded once (the library is built with -ffp-contract=off), every min and clamp a comparison
 *   `if (x < y) y = x`.  A = 2.0 * a_max, Vq = v_max * v_max, Mq = v_min * v_min.
 *   Arc length: W_0 = 0, W_{j+1} = W_j + L_j in segment order; length = W_{m-1} (path cost's length bits).  Sample k of segment j
 *     lies at s = W_j + L_j * ((double)k / Sd_j), the final sample at W_{m-1}; s is non-decreasing (rounding is monotone).
 *   Clearance limit: if d < margin: lq = Mq and the sample counts in n_below; else e = d - margin; lq = A * e;
 *     if (lq > Vq) lq = Vq; if (lq < Mq) lq = Mq.
 *   Corner limit (junction deviation), at the sample of interior waypoint i (1 <= i <= m-2), only if corner_dev is finite and
 *     L_{i-1} > 0 and L_i > 0:  u[c] = d_{i-1}[c] / L_{i-1};  w[c] = d_i[c] / L_i;  c = (u0*w0 + u1*w1) + u2*w2;
 *     if (c > 1.0) c = 1.0; if (c < -1.0) c = -1.0;  sh = sqrt(0.5 * (1.0 + c));  den = 1.0 - sh;
 *     if (den > 0): cq = ((a_max * corner_dev) * sh) / den;  if (cq < lq) lq = cq.   A straight joint limits nothing, a reversal
 *     gives 0, a zero-length segment limits nothing.
 *   Ends: sample 0: vs = v_start * v_start; if (vs < lq) lq = vs.  Sample n-1 the same with v_end.  A path of one sample takes both.
 *   Profile: P_k = A * s_k;  f_k = min_{j <= k} (lq_j - P_j) + P_k;  b_k = min_{j >= k} (lq_j + P_j) - P_k;
 *     q_k = lq_k; if (f_k < q_k) q_k = f_k; if (b_k < q_k) q_k = b_k;  v_k = sqrt(q_k).  min is exact and associative: any scan
 *     shape gives the same bits; q_k >= 0 because P is non-decreasing.
 *   Interval k, between samples k and k+1 in segment j: h = L_j / Sd_j; if (h == 0) dt = 0; else sv = v_k + v_{k+1};
 *     if (sv > 0) dt = (2.0 * h) / sv (exact for constant acceleration); else dt = 2.0 * sqrt(h / a_max) (the rest-to-rest triangle).
 * Outputs; every pointer of the result is nullable:
 *   per path: duration (the sum of dt), length, n_samples, n_below, min_speed (the minimum v_k), min_index (the smallest sample
 *     index that attains it), status:
 *       FIESTA_HIP_TIMING_OK
 *       FIESTA_HIP_TIMING_INVALID   a non-finite waypoint, a segment with L / step > 2^24; in the _dev variant only, offsets that
 *                                   break path clearance's offset rules
 *       FIESTA_HIP_TIMING_TOO_LONG  more than FIESTA_HIP_TIMING_MAX_WAYPOINTS waypoints or more than FIESTA_HIP_TIMING_MAX_SAMPLES
 *                                   samples
 *     checked in this order: the offset rules, the waypoint count (such a path's waypoints are not read), the waypoints and
 *     segments, the sample count.
 *   per waypoint (n_waypoints rows, every row written by every call): time (the sum of the dt before the waypoint's sample) and
 *     speed (v at the waypoint's sample).
 *   An empty path: duration 0, length 0, n_samples 0, n_below 0, min_speed +inf, min_index -1, status OK.  One waypoint: one
 *   sample, duration 0.  An INVALID or TOO_LONG path: duration, length and min_speed NaN, n_samples -1, n_below -1, min_index -1,
 *   its time and speed rows NaN; rows that belong to no path are NaN too; the other paths are unaffected.
 *   Everything but duration and time has the model's bits for any launch shape, and so has every single dt.  duration and time
 *   are sums whose order is free (fixed by the path's sample count alone): with n terms of absolute sum a they stay within
 *   (n + 16) * 2^-52 * a of the model.  No floating-point atomics: the same call on the same map gives the same bits.
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable; each is checked before the map handle is
 *   looked at): a parameter outside its rule, a NULL waypoints, offsets, params or result, negative counts, more than 2^30 paths,
 *   and in the host variant offsets that break the CSR rules.  n_paths = 0 does nothing.
 * fiesta_hip_path_timing      host pointers; stages, runs, synchronises (no host route for small batches: always the device).
 * fiesta_hip_path_timing_dev  waypoints, offsets and the result's arrays are device pointers (the two structs themselves are host
 *                             objects); only enqueued on the map's stream, nothing is read back.  There is no shard-group call. */
#define FIESTA_HIP_TIMING_MAX_WAYPOINTS 1024 /* per path */
#define FIESTA_HIP_TIMING_MAX_SAMPLES 4096   /* per path */
#define FIESTA_HIP_TIMING_OK 0
#define FIESTA_HIP_TIMING_INVALID 1
#define FIESTA_HIP_TIMING_TOO_LONG 2
typedef struct fiesta_hip_timing_params {
  double step;       /* sample spacing, metres */
  double margin;     /* clearance the robot keeps: the free distance is d - margin */
  double v_max;
  double v_min;      /* the crawl below the margin and the floor of the clearance limit */
  double a_max;
  double corner_dev; /* junction deviation, metres; +inf: no corner rule */
  double v_start;
  double v_end;
} fiesta_hip_timing_params;
typedef struct fiesta_hip_path_timing_result { /* every pointer nullable */
  double *duration;    /* n_paths */
  double *length;      /* n_paths */
  int64_t *n_samples;  /* n_paths */
  int64_t *n_below;    /* n_paths */
  double *min_speed;   /* n_paths */
  int64_t *min_index;  /* n_paths */
  int32_t *status;     /* n_paths: FIESTA_HIP_TIMING_* */
  double *time;        /* n_waypoints */
  double *speed;       /* n_waypoints */
} fiesta_hip_path_timing_result;
int fiesta_hip_path_timing(fiesta_hip_map *m, const double *waypoints, int64_t n_waypoints, const int64_t *offsets, int64_t n_paths,
                           const fiesta_hip_timing_params *params, const fiesta_hip_path_timing_result *result);
int fiesta_hip_path_timing_dev(fiesta_hip_map *m, const double *waypoints_dev, int64_t n_waypoints, const int64_t *offsets_dev,
                               int64_t n_paths, const fiesta_hip_timing_params *params, const fiesta_hip_path_timing_result *result);

/* ---- voxel clusters: the connected groups of a voxel list, with per-cluster statistics, on the device ----
 * The step between fiesta_hip_get_frontier_voxels and fiesta_hip_reach_field: a planner does not visit frontier voxels, it visits
 * FRONTIERS -- it groups the voxels, drops the specks of sensor noise, takes each group's centre and extent to place a viewpoint
 * and asks which group is cheapest to reach.  Read-only: nothing of the map is read but its resolution and origin, so the call is
 * the same for dense maps, shards and hash-block maps (there is no shard-group call; clusters do not cross shards).  No reference
 * counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * Inputs: vox, n entries of 3 int32 map voxel coordinates in any order (typically the frontier call's output; the call does not
 *   care what the voxels are); mask, nullable, one uint8 per entry (the frontier call's unknown-neighbour mask); key, nullable, one
 *   int32 per entry (e.g. target_cost of fiesta_hip_reach_field); connectivity 6, 18 or 26; min_size >= 1.
 * INVALID entry: any coordinate with |c| >= 2^20 - 1.  It belongs to no cluster and does not affect the others (three coordinates
 *   and their +-1 neighbours then pack into one 64-bit key).
 * Representative: the lowest entry index among the valid entries that name the same voxel.  Later duplicates receive their voxel's
 *   label but count for nothing: not for size, sums, box, mask, key or members.
 * Adjacency: two distinct voxels are adjacent if they differ by at most 1 per axis and in at most 1 / 2 / 3 axes for connectivity
 *   6 / 18 / 26.  Component: a connected component of the distinct valid voxels under that relation.  Size: its number of distinct
 *   voxels.  Root: the lowest entry index in it.
 * Components with size < min_size are dropped; the kept ones are numbered 0 .. K - 1 in increasing root order -- a function of the
 *   input list alone.
 * Outputs; every pointer of the result struct is nullable, and so is the struct:
 *   label       int32 per entry: the cluster id; -1 for an invalid entry and for an entry of a dropped component
 *   per cluster k, entries k < cluster_capacity written:
 *   size        int32
 *   root        int64 entry index
 *   box_lo / box_hi  3 int32 each, inclusive
 *   centroid    3 f64, metres: ((double)sum_c / (double)size + 0.5) * resolution + origin[c], sum_c the exact int64 coordinate sum over
 *               the representatives; each operation rounded once, in this order (that of fiesta_hip_reach_paths' waypoints_pos)
 *   mask_or     uint8: the OR of the representatives' masks; 0 if mask is NULL
 *   key_min     int32, key_argmin int64 entry index: the minimum of key over representatives with key >= 0 and the lowest entry index
 *               that attains it; INT32_MAX and -1 if there is none or key is NULL.  So -1 ("not traversable") and every negative
 *               key are ignored; an INT32_MAX key ("out of reach") is >= 0 and takes part.
 *   offsets     int64, CSR: the representatives of cluster k occupy members[offsets[k] .. offsets[k + 1]).  The array holds
 *               cluster_capacity + 1 entries; entries 0 .. min(K, cluster_capacity) are written.
 *   members     int64 entry indices; entries below member_capacity are written.  The order inside a cluster's segment is unspecified,
 *               the set is exact.
 *   info        whatever the capacities (so a call with capacities 0 sizes the buffers): n_clusters = K; n_members, the number of
 *               representatives in kept clusters (= offsets[K]); n_invalid, invalid entries; n_duplicates, valid entries that are
 *               not their voxel's representative; n_dropped_clusters; largest, the size of the largest kept cluster (0: none).
 *   Every value is an integer but the centroid: every output other than the order inside a member segment has the same bits for any
 *   launch shape, scheduling and hash-table size, and the bits of fiesta_amd.cluster_model (the definition in plain Python).
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): n < 0 or n > 2^24, connectivity not 6, 18 or
 *   26, min_size < 1, a negative capacity, vox NULL with n > 0, info NULL.  The scratch memory (a hash table of the next power of
 *   two >= 2 n slots, union-find arrays, per-cluster accumulators) belongs to the map: allocated on first use, grown on demand,
 *   freed by fiesta_hip_destroy.
 * fiesta_hip_cluster_voxels      host arrays; stages through the path queries' buffers, runs, synchronises, copies back label and
 *                                min(total, capacity) of each cluster array.
 * fiesta_hip_cluster_voxels_dev  every array, and info, is a device pointer (the result struct itself is a host object).  n_dev,
 *                                nullable: a device counter; the entry count is min(n, *n_dev), read on the device -- so
 *                                fiesta_hip_get_frontier_voxels_dev feeds this call with its own counter and buffers and no host
 *                                round trip.  n is then the capacity that sizes the scratch (and is what the whole-call errors
 *                                test); label beyond the device count is left untouched.  Only enqueued on the map's stream:
 *                                nothing data-dependent is read back. */
typedef struct fiesta_hip_cluster_result { /* every pointer nullable */
  int32_t *label;                          /* per entry */
  int32_t *size;                           /* per cluster */
  int64_t *root;                           /* per cluster */
  int32_t *box_lo;                         /* per cluster x 3 */
  int32_t *box_hi;                         /* per cluster x 3 */
  double *centroid;                        /* per cluster x 3, metres */
  uint8_t *mask_or;                        /* per cluster */
  int32_t *key_min;                        /* per cluster */
  int64_t *key_argmin;                     /* per cluster */
  int64_t *offsets;                        /* cluster_capacity + 1 */
  int64_t *members;                        /* member_capacity */
} fiesta_hip_cluster_result;
typedef struct fiesta_hip_cluster_info {
  int64_t n_clusters;
  int64_t n_members;
  int64_t n_invalid;
  int64_t n_duplicates;
  int64_t n_dropped_clusters;
  int64_t largest;
} fiesta_hip_cluster_info;
int fiesta_hip_cluster_voxels(fiesta_hip_map *m, const int32_t *vox, const uint8_t *mask, const int32_t *key, int64_t n, int32_t connectivity,
                              int32_t min_size, int64_t cluster_capacity, int64_t member_capacity, const fiesta_hip_cluster_result *result,
                              fiesta_hip_cluster_info *info);
int fiesta_hip_cluster_voxels_dev(fiesta_hip_map *m, const int32_t *vox_dev, const uint8_t *mask_dev, const int32_t *key_dev, int64_t n,
                                  const unsigned long long *n_dev, int32_t connectivity, int32_t min_size, int64_t cluster_capacity,
                                  int64_t member_capacity, const fiesta_hip_cluster_result *result, fiesta_hip_cluster_info *info_dev);

/* ---- cluster splitting: bisect large clusters into view-sized parts, on the device ----
 * The step between fiesta_hip_cluster_voxels and fiesta_hip_view_coverage: frontier surfaces touch one another, so one cluster can
 * hold most of a frontier, and a ring of views around the centroid of such a cluster looks at nothing.  Every frontier planner of
 * this family cuts large frontiers into view-sized pieces before it places viewpoints; this call does that.  Read-only: nothing of
 * the map is read but its resolution and origin, so the call is the same for dense maps, shards and hash-block maps (there is no
 * shard-group call).  No reference counterpart.  fiesta_hip_version() is still 101: detect these two calls by symbol lookup.
 * Inputs: the cluster call's vox (n x 3 int32), the nullable per-entry mask (uint8) and key (int32), the cluster call's CSR pair
 *   offsets (n_clusters + 1 int64) and members (n_members int64 entry indices), and three parameters: max_size >= 0, max_extent >= 0
 *   and 0 <= max_depth <= 63 (FIESTA_HIP_SPLIT_MAX_DEPTH).  For max_size and max_extent, 0 means the criterion is off.
 * A PART is a multiset of member indices.  Each non-empty cluster segment members[offsets[k] .. offsets[k + 1]) starts as one part at
 *   depth 0.  An empty segment yields no part.  For a part: its box is the tight inclusive box of its members' voxels;
 *   extent[c] = hi[c] - lo[c] + 1.  A part is OVERSIZE if max_size > 0 && size > max_size, or if max_extent > 0 &&
 *   max(extent) > max_extent.
 * An oversize part at depth < max_depth is split as follows: the axis a is the one with the largest extent, ties go to the lowest
 *   axis; mid = lo[a] + ((hi[a] - lo[a]) >> 1); members with c[a] <= mid form the low child and the rest form the high child, both
 *   at depth + 1.  An oversize part of distinct voxels (what the cluster call lists) always has extent >= 2 on a, so both children
 *   are non-empty, and the extent on a at least halves (rounded up).  A part whose members all name ONE voxel (a member listed
 *   more than once) has extent 1 and is never split: if max_size calls it oversize it stays so and counts in n_oversize.  With the cluster call's coordinate limit (|c| < 2^20 - 1) no recursion is deeper than 63: max_depth = 63
 *   never cuts anything.
 * Parts are numbered cluster-major and, inside a cluster, in order with low before high.  That is the order of their segments in
 *   the output members.  The numbering is a function of the member sets alone.  The order inside a part's segment is unspecified;
 *   the set is exact.  A member listed twice counts twice.  PARTS NEED NOT BE CONNECTED: a cut plane can separate a part into
 *   pieces that only touched through the other side.
 * Outputs; every pointer of the result struct is nullable, and so is the struct.  The per-part arrays are written for
 *   p < min(P, part_capacity), P the number of parts:
 *   parent      int32: the input cluster of the part
 *   depth       uint8
 *   size        int32
 *   root        int64: the lowest entry index in the part
 *   box_lo / box_hi  3 int32 each, inclusive
 *   centroid    3 f64, metres: ((double)sum_c / (double)size + 0.5) * resolution + origin[c], sum_c the exact int64 coordinate sum
 *               over the part's members: exactly the cluster call's expression and operation order
 *   mask_or     uint8, key_min int32, key_argmin int64: under the cluster call's rules, over the part's members
 *   offsets     int64, CSR: part p occupies members[offsets[p] .. offsets[p + 1]).  part_capacity + 1 entries, of which
 *               min(P, part_capacity) + 1 are written.  A split is a partition inside the part's own range, so offsets[0] and
 *               offsets[P] are the input's offsets[0] and offsets[n_clusters]
 *   members     int64, n_members entries: the positions offsets[0] .. offsets[P) are written (the host variant copies the input's
 *               values below offsets[0]; the _dev variant leaves those positions untouched)
 *   label       int32 per entry: filled with -1, then set to the part that lists the entry.  If several parts list an entry, the
 *               largest part index wins.
 *   info        whatever the capacities (so a call with part_capacity 0 sizes the buffers): n_parts = P; n_members = offsets[P];
 *               n_split_clusters, the clusters cut at least once; n_oversize, the parts left oversize by max_depth; largest, the
 *               size of the largest part; depth, the deepest level used; status, FIESTA_HIP_SPLIT_OK or _INVALID.
 *   With both criteria off the call is the identity: every per-part array then equals the cluster call's per-cluster array bit for
 *   bit.  Every value is an integer but the centroid, every reduction is exact and commutative: every output other than the order
 *   inside a member segment has the same bits for any launch shape, and the bits of fiesta_amd.split_model (the definition in plain
 *   Python).  OUTPUTS MUST NOT OVERLAP INPUTS (members in particular: the call reads the input members while it writes the output).
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): n, n_clusters or n_members negative or above
 *   2^24; max_size < 0, max_extent < 0, max_depth outside 0 .. 63; vox NULL with n > 0, offsets NULL with n_clusters > 0, members
 *   NULL with n_members > 0, info NULL; a negative part_capacity.
 * Data errors: offsets[0] < 0, or a decreasing offset; offsets[n_clusters] > n_members; a member index outside [0, n); a member
 *   whose voxel breaks the cluster call's coordinate limit.  On a data error the host variant returns FIESTA_HIP_ERR_INVALID.  The
 *   _dev variant cannot refuse a batch: it sets info.status = FIESTA_HIP_SPLIT_INVALID and n_parts = 0 (every other counter 0) and
 *   writes nothing else but the label fill -- one validation pass sets a device flag that every later kernel tests first.  This is
 *   also how a cluster call cut off by its member_capacity shows up (its offsets end above the members that were written).
 * The scratch memory, O(n_members) (there can never be more parts than members), belongs to the map: allocated on first use, grown
 *   on demand, freed by fiesta_hip_destroy.
 * fiesta_hip_split_clusters      host arrays; stages through the path queries' buffers, runs, copies back and synchronises once.
 *                                Per-part entries at and beyond n_parts read 0.
 * fiesta_hip_split_clusters_dev  every array, and info, is a device pointer (the result struct itself is a host object).
 *                                n_clusters_dev, nullable: a device int64, e.g. &info_dev->n_clusters of
 *                                fiesta_hip_cluster_voxels_dev; the effective cluster count is min(n_clusters, *n_clusters_dev), and
 *                                the effective member count is offsets[that].  &info_dev->n_parts, offsets, members and centroid go
 *                                straight into fiesta_hip_view_coverage_dev as n_groups_dev and the group arrays.  Only enqueued on
 *                                the map's stream: nothing data-dependent is read back.  The host enqueues max_depth levels, and a
 *                                level with no oversize part returns at once on a device counter. */
#define FIESTA_HIP_SPLIT_MAX_DEPTH 63
#define FIESTA_HIP_SPLIT_OK 0
#define FIESTA_HIP_SPLIT_INVALID 1
typedef struct fiesta_hip_split_result { /* every pointer nullable */
  int32_t *parent;                       /* per part */
  uint8_t *depth;                        /* per part */
  int32_t *size;                         /* per part */
  int64_t *root;                         /* per part */
  int32_t *box_lo;                       /* per part x 3 */
  int32_t *box_hi;                       /* per part x 3 */
  double *centroid;                      /* per part x 3, metres */
  uint8_t *mask_or;                      /* per part */
  int32_t *key_min;                      /* per part */
  int64_t *key_argmin;                   /* per part */
  int64_t *offsets;                      /* part_capacity + 1 */
  int64_t *members;                      /* n_members */
  int32_t *label;                        /* per entry */
} fiesta_hip_split_result;
typedef struct fiesta_hip_split_info {
  int64_t n_parts;
  int64_t n_members;
  int64_t n_split_clusters;
  int64_t n_oversize;
  int64_t largest;
  int64_t depth;
  int64_t status;
} fiesta_hip_split_info;
int fiesta_hip_split_clusters(fiesta_hip_map *m, const int32_t *vox, const uint8_t *mask, const int32_t *key, int64_t n, const int64_t *offsets,
                              const int64_t *members, int64_t n_clusters, int64_t n_members, int32_t max_size, int32_t max_extent,
                              int32_t max_depth, int64_t part_capacity, const fiesta_hip_split_result *result, fiesta_hip_split_info *info);
int fiesta_hip_split_clusters_dev(fiesta_hip_map *m, const int32_t *vox_dev, const uint8_t *mask_dev, const int32_t *key_dev, int64_t n,
                                  const int64_t *offsets_dev, const int64_t *members_dev, int64_t n_clusters, const int64_t *n_clusters_dev,
                                  int64_t n_members, int32_t max_size, int32_t max_extent, int32_t max_depth, int64_t part_capacity,
                                  const fiesta_hip_split_result *result, fiesta_hip_split_info *info_dev);

/* ---- view coverage: which target voxels would a sensor at each candidate viewpoint see, per view, per target and per group ----
 * The step after fiesta_hip_cluster_voxels: a frontier planner samples candidate poses around each cluster, counts how many of the
 * cluster's voxels each pose would see -- inside the sensor's range and field of view, nothing blocking the ray -- and keeps the
 * best pose per cluster.  One fused call instead of building, culling, uploading and reducing every (view, member) segment by
 * hand around fiesta_hip_ray_query.  Read-only; dense maps, shards (a shard answers for its own array, like the ray query; there is
 * no shard-group call) and hash-block maps.  No reference counterpart.  fiesta_hip_version() is still 101: detect these two calls
 * by symbol lookup.
 * Targets: vox, n entries of 3 int32 map voxel coordinates, n <= 2^24.  The centre of entry i is
 *   p[c] = ((double)vox[3 i + c] + 0.5) * resolution + origin[c]   (the order of the cluster centroid and of waypoints_pos).
 * Groups (the CSR pair of the cluster call): offsets, int64, n_groups + 1 entries, and members, int64 entry indices into vox,
 *   n_members of them; both nullable.  Every offset is clamped into [0, n_members] when it is read; group g lists
 *   members[lo .. hi) with lo = offsets[g], hi = offsets[g + 1] (an empty group if hi <= lo).  members NULL: the segment indexes
 *   vox directly (n_members is ignored and taken as n).  offsets NULL: ONE group, [0, n_members), and n_groups is taken as 1.  A
 *   member index outside [0, n) contributes no pair.  n_groups, n_members <= 2^24.
 * Views, V <= 2^24 of them, in one of two forms (fiesta_hip_view_set; exactly one of pos and centroid is non-NULL):
 *   explicit  pos, V x 3 f64 metres; dir, V x 2 f64, the horizontal unit forward vector (the caller's cos / sin of the yaw: no
 *             trigonometry is part of the contract), nullable only with FIESTA_HIP_VIEW_OMNI; group, V int32, nullable: every view
 *             looks at group 0.  n_views = V; ring / n_ring unused.
 *   ring      centroid, n_groups x 3 f64 (the cluster call's output), and ring, n_ring rows of 5 f64 (ox, oy, oz, dx, dy): view
 *             k * n_ring + j has pos[c] = centroid[3 k + c] + ring[5 j + c] (one add), dir = (dx_j, dy_j) and group k;
 *             V = n_groups * n_ring; n_views is ignored.
 * Sensor (fiesta_hip_view_sensor): min_range <= max_range, tan_h, tan_v, all >= 0 and no NaN (+inf allowed); block_mask, a subset
 *   of FIESTA_HIP_RAY_OCCUPIED | UNKNOWN | OUTSIDE; flags, FIESTA_HIP_VIEW_OMNI or 0; min_clearance (metres; <= 0: no test);
 *   min_visible >= 1.
 * Effective group count: n_groups, in the _dev call min(n_groups, *n_groups_dev).
 * A view is USABLE iff its position is finite with |pos[c] / resolution| < 2^30, its group g satisfies 0 <= g < the effective
 *   group count, the class (fiesta_hip_ray_query's, of the walk voxel floor(pos / resolution): the map voxel of that voxel's centre)
 *   is FREE and, when min_clearance > 0, GetDistance(Vector3i) of that map voxel is >= min_clearance (the frontier call's test).
 * Pairs: a usable view forms one pair with every listed member of its group (a member listed twice makes two pairs).  With
 *   q[c] = p[c] - pos[c], every product and sum rounded once, sums left to right:
 *   in range  d2 = q0*q0 + q1*q1 + q2*q2;  min_range*min_range <= d2 && d2 <= max_range*max_range
 *   in view   without OMNI: fwd = q0*dx + q1*dy, lat = q1*dx - q0*dy;  fwd > 0 && fabs(lat) <= tan_h*fwd && fabs(q2) <= tan_v*fwd
 *             with OMNI:    fabs(q2) <= tan_v * sqrt(q0*q0 + q1*q1)
 *   visible   in range and in view, the ray pos -> p is valid under fiesta_hip_ray_query's rule, and its walk W (exactly that
 *             call's) has no k < |W| - 1 with class(W[k]) & block_mask.  The last voxel of W is the target's own and is never
 *             tested: a frontier voxel borders unknown space, and a target may itself be unknown.
 * Outputs; every pointer of the result struct is nullable:
 *   view_class  uint8 per view: the class of the view's voxel; 0 if the position is invalid
 *   n_in_view   int32 per view: its pairs in range and in view;  n_visible  int32 per view: its visible pairs; both -1 for an
 *               unusable view
 *   cover_count int32 per target entry: the visible pairs that name it;  first_view  int32 per entry: the lowest view index that
 *               sees it, -1 if none
 *   best_view   int64 per group (n_groups entries): among the usable views of the group with n_visible >= min_visible the one with
 *               the largest n_visible, the lowest index among equals; -1 if none.  best_count  int32: its n_visible, 0 if none
 *   info        n_usable views, n_pairs, n_in_view and n_visible pairs in total
 *   Every value is an integer; every decision is an f64 comparison in the order above: the same bits for any launch shape, and the
 *   bits of fiesta_amd.view_coverage_model (the definition in numpy over fiesta_amd.ray_walk).
 * Whole-call errors (FIESTA_HIP_ERR_INVALID, nothing launched, the map stays usable): views, sensor or info NULL; vox NULL with
 *   n > 0; both view forms or neither; ring NULL or n_ring < 0 in ring form; dir NULL without OMNI; a negative count or one above
 *   2^24 (n, n_groups, n_members, V); a NaN or negative range or tangent; min_range > max_range; block_mask outside 0 .. 7; unknown
 *   flag bits; min_visible < 1.  V = 0 or n = 0 writes the identities.  The scratch (O(V + n_groups)) belongs to the map.
 * fiesta_hip_view_coverage      host arrays; stages through the path queries' buffers, runs, synchronises, copies back.
 * fiesta_hip_view_coverage_dev  every array, and info, is a device pointer (the structs themselves are host objects).
 *                               n_groups_dev, nullable: a device int64, e.g. &info_dev->n_clusters of
 *                               fiesta_hip_cluster_voxels_dev -- frontier -> clusters -> coverage needs no host round trip.  Only
 *                               enqueued on the map's stream. */
#define FIESTA_HIP_VIEW_OMNI 1
typedef struct fiesta_hip_view_set {
  const double *pos;      /* explicit form: V x 3 */
  const double *dir;      /* V x 2 */
  const int32_t *group;   /* V, nullable */
  int64_t n_views;        /* V of the explicit form */
  const double *centroid; /* ring form: n_groups x 3 */
  const double *ring;     /* n_ring x 5 */
  int64_t n_ring;
} fiesta_hip_view_set;
typedef struct fiesta_hip_view_sensor {
  double min_range, max_range, tan_h, tan_v, min_clearance;
  int32_t block_mask, flags, min_visible, reserved; /* reserved: ignored */
} fiesta_hip_view_sensor;
typedef struct fiesta_hip_view_result { /* every pointer nullable */
  uint8_t *view_class;                  /* per view */
  int32_t *n_in_view;                   /* per view */
  int32_t *n_visible;                   /* per view */
  int32_t *cover_count;                 /* per target entry */
  int32_t *first_view;                  /* per target entry */
  int64_t *best_view;                   /* per group */
  int32_t *best_count;                  /* per group */
} fiesta_hip_view_result;
typedef struct fiesta_hip_view_info {
  int64_t n_usable;
  int64_t n_pairs;
  int64_t n_in_view;
  int64_t n_visible;
} fiesta_hip_view_info;
int fiesta_hip_view_coverage(fiesta_hip_map *m, const int32_t *vox, int64_t n, const int64_t *offsets, const int64_t *members,
                             int64_t n_groups, int64_t n_members, const fiesta_hip_view_set *views, const fiesta_hip_view_sensor *sensor,
                             const fiesta_hip_view_result *result, fiesta_hip_view_info *info);
int fiesta_hip_view_coverage_dev(fiesta_hip_map *m, const int32_t *vox_dev, int64_t n, const int64_t *offsets_dev, const int64_t *members_dev,
                                 int64_t n_groups, const int64_t *n_groups_dev, int64_t n_members, const fiesta_hip_view_set *views,
                                 const fiesta_hip_view_sensor *sensor, const fiesta_hip_view_result *result, fiesta_hip_view_info *info_dev);

/* ---- whole-field access (tests, visualisation, checkpoints) ----
 * Dense dump in the reference's linear order; each output is nullable.
 *   d2      int32  squared voxel distance to the closest obstacle; -1 never observed; INT32_MAX observed
 *                  but no obstacle reachable. distance_buffer_ == sqrt(d2) * resolution.
 *   coc     3 x int32 closest_obstacle_ (global voxel coordinates; -10000 undefined)
 *   occ     uint8  Exist(idx)
 *   logodds double occupancy_buffer_ */
int fiesta_hip_download_field(fiesta_hip_map *m, int32_t *d2, int32_t *coc, uint8_t *occ, double *logodds);
/* Pending observation counters num_hit_ / num_miss_ (include/ESDFMap.h:89; num_miss_ counts ALL observations
 * since the last UpdateOccupancy), dense order (hash-block maps: the order of fiesta_hip_download_hash); each output
 * nullable. */
int fiesta_hip_download_counts(fiesta_hip_map *m, int32_t *num_hit, int32_t *num_miss);
/* Checkpoint: the whole map state (closest-obstacle field, log-odds, pending observation counters, occupancy bits,
 * insert/delete queues, update ranges; hash-block maps: the page pool, the directory and the window position) written
 * to / read from a raw file, streamed through a pinned buffer.  A file loads only into a map created with the same
 * mode, origin, resolution and grid (array mode: same shard); afterwards the map behaves exactly like the one that
 * was saved.  The reference has no counterpart (its state dies with the node). */
int fiesta_hip_save(fiesta_hip_map *m, const char *path);
int fiesta_hip_load(fiesta_hip_map *m, const char *path);
/* Visualisation exports, compacted / sliced on the device (reference: ESDFMap::GetPointCloud and GetSliceMarker,
 * src/ESDFMap.cpp:544-699, which fill ROS messages -- a ROS adapter wraps these two calls).
 * get_occupied_voxels: map voxel coordinates of every occupied voxel, at most `capacity` triples are written,
 * *n_out is the total (call with vox NULL / capacity 0 to size the buffer). Order is unspecified.
 * get_slice: GetDistance(Vector3i) for every (x, y) of the plane z = z_vox, nx * ny doubles, x-major. */
int fiesta_hip_get_occupied_voxels(fiesta_hip_map *m, int32_t *vox, int64_t capacity, int64_t *n_out);
/* Observed voxels (of the owned box of a shard) whose distance reads +10000, "no obstacle" (src/ESDFMap.cpp:246-249,
 * 306, 328): voxels observed late that no wave has reached yet, everything while the map holds no obstacle -- and, on a
 * grid beyond 1024 voxels per axis ONLY, voxels farther than 512 voxels from every obstacle: the reach of a stored id there
 * (the reference's closest_obstacle_ is a full Vector3i, include/ESDFMap.h:90, but it cannot hold such a grid).  A
 * deployment on a large grid watches this number: it is the count of distances truncated to "none".  Array maps only. */
int fiesta_hip_count_no_obstacle(fiesta_hip_map *m, int64_t *n_out);
int fiesta_hip_get_slice(fiesta_hip_map *m, int32_t z_vox, double *out);
/* The two getters themselves, filtered and converted on the device exactly as the reference fills its messages (array
 * and hash-block maps; the C++ class include/fiesta/ESDFMap.h fills any message type with the reference's field names):
 * get_point_cloud   ESDFMap::GetPointCloud(m, vis_lower_bound, vis_upper_bound), src/ESDFMap.cpp:544-582: voxel centres
 *                   (float xyz, like geometry_msgs::Point32) of the occupied voxels inside the update range whose z
 *                   INDEX lies in [vis_lower_bound, vis_upper_bound];
 * get_slice_marker  ESDFMap::GetSliceMarker(m, slice, id, color, max_dist), :639-699: centres (double xyz) and colours
 *                   (float rgba, the rainbow of :584-636) of the voxels of plane z = slice inside the x/y update range
 *                   that hold a defined, finite distance.
 * At most `capacity` entries are written, *n_out is the total (size the buffers with capacity 0). The reference's
 * message order (x, y, z lexicographic / allocation order) is not reproduced: a point set is unordered. */
int fiesta_hip_get_point_cloud(fiesta_hip_map *m, int32_t vis_lower_bound, int32_t vis_upper_bound, float *xyz,
                               int64_t capacity, int64_t *n_out);
int fiesta_hip_get_slice_marker(fiesta_hip_map *m, int32_t slice, double max_dist, double *xyz, float *rgba,
                                int64_t capacity, int64_t *n_out);
/* Hash mode: allocated voxels in allocation order (vox n x 3); with all outputs NULL only *n_out is set. */
int fiesta_hip_download_hash(fiesta_hip_map *m, int64_t *n_out, int32_t *vox, int32_t *d2, int32_t *coc,
                             uint8_t *occ);

/* Device-side snapshots of the map's state (benchmark repetitions, tests). slot in [0,3].  A snapshot holds everything an
 * update reads or writes: the field, log-odds, occupancy, the pending observation counts and the touched list, both queues,
 * the update range and its predecessor, the gates' bookkeeping.  It does NOT hold the probability parameters (a checkpoint
 * file does): fiesta_hip_set_prob_params after a save survives the restore.  A call with a slot out of range or never saved
 * fails and leaves the map as it was.
 * Hash-block maps: slot 0 only, save + count_updated only (one copy of the state words; restore is an error). */
int fiesta_hip_snapshot_save(fiesta_hip_map *m, int32_t slot);
int fiesta_hip_snapshot_restore(fiesta_hip_map *m, int32_t slot);
/* Number of voxels whose (d2, closest obstacle) differs between snapshot `slot` and the current state,
 * counted as SURVEY.md 8d defines an "updated voxel": d2 differs, or the old closest obstacle is no longer
 * occupied.  A voxel that only names another of several equidistant obstacles is not updated; a shard counts the box it
 * owns, a hash-block map the pages inside its window.  The definition holds for a field that is up to date: a count taken
 * between UpdateOccupancy and UpdateESDF is outside what this call promises. */
int fiesta_hip_snapshot_count_updated(fiesta_hip_map *m, int32_t slot, int64_t *updated);

/* ---- multi-GPU: one map = one SHARD of a larger grid; used by the sharded driver ----
 * Create the shard with cfg.global_grid = the global extents, cfg.shard_lo = the global voxel origin of the box it
 * OWNS, cfg.map_size = the owned extents in metres and cfg.origin = the GLOBAL map origin. The shard allocates a
 * 2-voxel ghost layer (the stencil radius) on every side that has a neighbour; closest-obstacle ids are global.
 * One UpdateESDF of the whole grid is, on every shard (all _dev pointers are on the shard's GPU):
 *     update_occupancy -> export_transitions -> [all-gather] -> apply_transitions          (occupancy in sync)
 *     esdf_seed -> { pack ghosts-to-be / [send,recv] / apply -> relax_pending } until no shard changed anything
 * The [..] steps are RCCL collectives issued by the host driver (fiesta_amd/sharded.py over torch.distributed). */
typedef struct fiesta_hip_shard_info {
  int32_t local_dims[3];    /* extents of the local array (owned box + ghost layers) */
  int32_t local_origin[3];  /* global voxel coordinates of local voxel (0,0,0) */
  int32_t owned_lo[3];      /* owned box in LOCAL coordinates, inclusive */
  int32_t owned_hi[3];
  int32_t global_grid[3];
} fiesta_hip_shard_info;
int fiesta_hip_shard_info_get(fiesta_hip_map *m, fiesta_hip_shard_info *out);
/* Copies the words of the inclusive LOCAL box [lo,hi] into out_dev (dense, z fastest); blocks until done. */
int fiesta_hip_halo_pack_dev(fiesta_hip_map *m, const int32_t box_lo[3], const int32_t box_hi[3], uint32_t *out_dev);
/* Overwrites the ghost cells of the inclusive LOCAL box with a neighbour's words; a cell that changed and carries
 * an obstacle becomes a frontier source and wakes its tile. *n_changed (nullable) = cells that differed. */
int fiesta_hip_halo_apply_dev(fiesta_hip_map *m, const int32_t box_lo[3], const int32_t box_hi[3],
                              const uint32_t *in_dev, int64_t *n_changed);
/* Occupancy transitions queued on this shard: TWO uint32 words per entry, x | y << 16 and z | occupied-now << 31
 * (global voxel coordinates); capacity and *n_out count ENTRIES. out_dev NULL: only the count. Does not consume the
 * queues. */
int fiesta_hip_export_transitions_dev(fiesta_hip_map *m, uint32_t *out_dev, int64_t capacity, int64_t *n_out);
/* Applies transitions (of any shard, own ones included) to this shard's replica of the global occupancy bitmap. */
int fiesta_hip_apply_transitions_dev(fiesta_hip_map *m, const uint32_t *entries_dev, int64_t n);
/* Host-buffer forms of the four calls above (for transports that are not GPU-aware, and for tests). */
int fiesta_hip_halo_pack(fiesta_hip_map *m, const int32_t box_lo[3], const int32_t box_hi[3], uint32_t *out);
int fiesta_hip_halo_apply(fiesta_hip_map *m, const int32_t box_lo[3], const int32_t box_hi[3], const uint32_t *in,
                          int64_t *n_changed);
int fiesta_hip_export_transitions(fiesta_hip_map *m, uint32_t *out, int64_t capacity, int64_t *n_out);
int fiesta_hip_apply_transitions(fiesta_hip_map *m, const uint32_t *entries, int64_t n);
/* The seeding half of UpdateESDF (insert drain + delete invalidation, src/ESDFMap.cpp:278-337): consumes the
 * queues and leaves the seeded tiles pending. */
int fiesta_hip_esdf_seed(fiesta_hip_map *m, fiesta_hip_stats *stats);
/* The relaxation half (src/ESDFMap.cpp:339-392): relaxes every pending tile to quiescence (no queues consumed).
 * *pending_tiles (nullable) = tiles that were pending at entry. */
int fiesta_hip_relax_pending(fiesta_hip_map *m, fiesta_hip_stats *stats, int64_t *pending_tiles);

/* ---- the shard protocol itself, native (fiesta_amd/csrc/shard_group.hip): C++ host code over RCCL ----
 * A group drives UpdateOccupancy / UpdateESDF of ONE map cut into `world` shards (1, 2, 4 or 8: 1x1x1, 2x1x1, 2x2x1,
 * 2x2x2; shard r owns box r of the regular cut, see fiesta_hip_shard_box).  Two set-ups:
 *   - one rank per GPU: n_local = 1, local_ranks[0] = this process's rank, rccl_id = the 128 bytes rank 0 obtained from
 *     fiesta_hip_rccl_unique_id and handed to every rank out of band (e.g. a torch.distributed / MPI broadcast);
 *   - every shard in this process (tests; N shards multiplexed on one GPU): n_local = world, rccl_id = NULL.
 * Per sweep of UpdateESDF each shard sends only the boundary cells that CHANGED since it last sent them
 * ({receiver cell index, word} entries) to its <= 26 neighbours in one ncclGroup; one small all-gather per sweep carries
 * the message sizes and the convergence test. */
typedef struct fiesta_hip_shard_group fiesta_hip_shard_group;
int fiesta_hip_rccl_unique_id(uint8_t id[128]);
int fiesta_hip_shard_box(const int32_t global_grid[3], int32_t world, int32_t rank, int32_t lo[3], int32_t size[3]);
int fiesta_hip_shard_group_create(fiesta_hip_map *const *local_shards, const int32_t *local_ranks, int32_t n_local,
                                  int32_t world, const uint8_t *rccl_id, fiesta_hip_shard_group **out);
/* A third transport for the same protocol: the caller's own messaging, through HOST buffers.  One shard per process (like
 * RCCL); the library stages what it sends and receives through host memory and calls
 *   all_gather(ctx, send, recv, bytes)      every rank contributes `bytes` bytes; recv = world x bytes, in rank order
 *   exchange(ctx, n, peers, send, send_bytes, recv, recv_bytes)   for k < n: send_bytes[k] bytes from send[k] go to rank
 *                                           peers[k], recv_bytes[k] bytes from that rank arrive in recv[k] (either may be 0;
 *                                           a pair of ranks exchanges at most one message each way per call)
 * Both are collective over the group's ranks and return 0 on success.  Slower than RCCL by the staging copies; it exists
 * so that the C++ sweep loop, sparse diff / apply and convergence test can run ACROSS PROCESSES where RCCL cannot (two ranks
 * on one GPU) -- the multi-process tests bind it to torch.distributed over gloo -- or over a fabric RCCL does not know. */
typedef struct fiesta_hip_shard_transport {
  void *ctx;
  int32_t (*all_gather)(void *ctx, const void *send, void *recv, int64_t bytes);
  int32_t (*exchange)(void *ctx, int32_t n, const int32_t *peers, const void *const *send, const int64_t *send_bytes,
                      void *const *recv, const int64_t *recv_bytes);
} fiesta_hip_shard_transport;
int fiesta_hip_shard_group_create_hosted(fiesta_hip_map *local_shard, int32_t local_rank, int32_t world,
                                         const fiesta_hip_shard_transport *transport, fiesta_hip_shard_group **out);
/* The LOCAL half of _create's checks (shard boxes against the regular cut, set-up rules, librccl loadable when
 * use_rccl) without the collective communicator set-up: ranks exchange the outcome of this first (out of band), so that
 * one rank's local failure cannot leave the others blocked inside ncclCommInitRank. */
int fiesta_hip_shard_group_precheck(fiesta_hip_map *const *local_shards, const int32_t *local_ranks, int32_t n_local,
                                    int32_t world, int32_t use_rccl);
/* What the RCCL communicator itself reports: *nranks = ncclCommCount (0: local transport, no communicator),
 * *rank = ncclCommUserRank.  For self-verifying multi-GPU runs (bench.py prints it). */
int fiesta_hip_shard_group_comm_info(fiesta_hip_shard_group *g, int32_t *nranks, int32_t *rank);
int fiesta_hip_shard_group_destroy(fiesta_hip_shard_group *g);
/* ESDFMap::UpdateOccupancy of the whole map: *n_insert / *n_delete are the queue sizes summed over all shards. */
int fiesta_hip_shard_group_update_occupancy(fiesta_hip_shard_group *g, int32_t global_map, int64_t *n_insert,
                                            int64_t *n_delete, int32_t *any);
/* ESDFMap::UpdateESDF of the whole map. stats: summed over this process's shards; *sweeps: ghost exchanges;
 * *entries_sent: boundary entries this process sent (8 bytes each). */
int fiesta_hip_shard_group_update_esdf(fiesta_hip_shard_group *g, fiesta_hip_stats *stats, int32_t *sweeps,
                                       int64_t *entries_sent);

/* Blocks until all device work of the map has finished. */
int fiesta_hip_synchronize(fiesta_hip_map *m);

#ifdef __cplusplus
}
#endif
#endif /* FIESTA_HIP_H */
