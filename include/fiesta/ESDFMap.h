// include/fiesta/ESDFMap.h -- drop-in `fiesta::ESDFMap` backed by the MI355X engine (libfiesta_hip.so).
//
// Same public surface as the reference class (HKUST-Aerial-Robotics/FIESTA include/ESDFMap.h:111-166):
// constructors, SetParameters, CheckUpdate, UpdateOccupancy, UpdateESDF, SetOccupancy x2, GetOccupancy x2,
// GetDistance x2, GetDistWithGradTrilinear, SetUpdateRange, SetOriginalRange, the public data member
// grid_total_size_, CheckConsistency / CheckWithGroundTruth.  The ROS-typed visualisation getters
// (GetPointCloud / GetSliceMarker, :144-145) are templates on the message type -- there is no ROS in this build -- next
// to plain-array equivalents (GetOccupiedVoxels, GetSlice).
//
// Header-only and free of HIP types: everything goes through the C ABI of include/fiesta_hip.h.  Array vs
// hash-block storage is a RUNTIME choice (the constructor overload), not the reference's -DHASH_TABLE macro.
//
// Differences a caller can observe (all documented in INTEGRATION.md):
//   * SetOccupancy calls are buffered on the host and applied as ONE device batch at the next
//     CheckUpdate / UpdateOccupancy / query; return values are computed on the host and are identical.
//   * single-point queries cost one device round trip each -- use the *Batch forms in planners.
//   * closest-obstacle ids are tie-equivalent, not FIFO-order-identical (parity contract).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../fiesta_hip.h"
#include "vec3.h"

namespace fiesta {

class ESDFMap {
 public:
  // dense array: ESDFMap(origin, resolution, map_size) (src/ESDFMap.cpp:171-213)
  ESDFMap(Eigen::Vector3d origin, double resolution, Eigen::Vector3d map_size, int device = 0) {
    fiesta_hip_config c = make_config(origin, resolution, device);
    c.mode = FIESTA_HIP_MODE_ARRAY;
    for (int i = 0; i < 3; ++i) c.map_size[i] = map_size(i);
    open(c);
    for (int i = 0; i < 3; ++i) {
      min_range_[i] = origin(i);
      max_range_[i] = origin(i) + map_size(i);
    }
  }
  // hash blocks: ESDFMap(origin, resolution, reserve_size) (src/ESDFMap.cpp:130-167)
  ESDFMap(Eigen::Vector3d origin, double resolution, int reserve_size = 0, int device = 0) {
    fiesta_hip_config c = make_config(origin, resolution, device);
    c.mode = FIESTA_HIP_MODE_HASH;
    c.reserve_size = reserve_size;
    open(c);
    hash_ = true;
    for (int i = 0; i < 3; ++i) {
      min_range_[i] = -1e30;
      max_range_[i] = 1e30;
    }
  }
  ~ESDFMap() {
    if (h_) fiesta_hip_destroy(h_);
  }
  ESDFMap(const ESDFMap &) = delete;
  ESDFMap &operator=(const ESDFMap &) = delete;

  void SetParameters(double p_hit, double p_miss, double p_min, double p_max, double p_occ) {
    ck(fiesta_hip_set_prob_params(h_, p_hit, p_miss, p_min, p_max, p_occ));
  }
  bool CheckUpdate() {
    Flush();
    int32_t out = 0;
    ck(fiesta_hip_check_update(h_, &out));
    return out != 0;
  }
  bool UpdateOccupancy(bool global_map) {
    Flush();
    int32_t any = 0;
    ck(fiesta_hip_update_occupancy(h_, global_map ? 1 : 0, &last_insert_, &last_delete_, &any));
    return any != 0;
  }
  void UpdateESDF() { ck(fiesta_hip_update_esdf(h_, &last_stats_)); }

  // Occupancy Management (src/ESDFMap.cpp:401-437). Returns what the reference returns.
  int SetOccupancy(Eigen::Vector3d pos, int occ) {
    if (occ != 1 && occ != 0) return FIESTA_HIP_UNDEFINED;  // "occ value error!" (:402-405)
    if (!PosInMap(pos)) return FIESTA_HIP_UNDEFINED;
    Eigen::Vector3i vox;
    Pos2Vox(pos, vox);
    return SetOccupancy(vox, occ);
  }
  int SetOccupancy(Eigen::Vector3i vox, int occ) {
    pend_vox_.push_back(vox(0));
    pend_vox_.push_back(vox(1));
    pend_vox_.push_back(vox(2));
    pend_occ_.push_back(occ);
    if (pend_occ_.size() >= kFlushAt) Flush();
    return Vox2Idx(vox);  // the caller's de-duplication key (include/Fiesta.h:221-232,253-273); unique per voxel
  }
  int GetOccupancy(Eigen::Vector3d pos) {
    Flush();
    int32_t out = 0;
    const double p[3] = {pos(0), pos(1), pos(2)};
    ck(fiesta_hip_get_occupancy_pos(h_, p, 1, &out));
    return out;
  }
  int GetOccupancy(Eigen::Vector3i vox) {
    Flush();
    int32_t out = 0;
    const int32_t v[3] = {vox(0), vox(1), vox(2)};
    ck(fiesta_hip_get_occupancy_vox(h_, v, 1, &out));
    return out;
  }

  // Distance Field Management (src/ESDFMap.cpp:467-540).  Rule for the buffered SetOccupancy calls: whatever can
  // observe them flushes them first (CheckUpdate, UpdateOccupancy, GetOccupancy, the range setters, the exports);
  // distance queries do NOT flush -- distances only change inside UpdateESDF, which only sees what UpdateOccupancy
  // (a flush) fused before it, so pending observations cannot change any answer below.
  double GetDistance(Eigen::Vector3d pos) {
    double out = 0;
    const double p[3] = {pos(0), pos(1), pos(2)};
    ck(fiesta_hip_get_distance_pos(h_, p, 1, &out));
    return out;
  }
  double GetDistance(Eigen::Vector3i vox) {
    double out = 0;
    const int32_t v[3] = {vox(0), vox(1), vox(2)};
    ck(fiesta_hip_get_distance_vox(h_, v, 1, &out));
    return out;
  }
  double GetDistWithGradTrilinear(Eigen::Vector3d pos, Eigen::Vector3d &grad) {
    double d = 0, g[3] = {0, 0, 0};
    const double p[3] = {pos(0), pos(1), pos(2)};
    ck(fiesta_hip_get_dist_grad(h_, p, 1, &d, g));
    for (int i = 0; i < 3; ++i) grad(i) = g[i];
    return d;
  }
  // batch forms (the fast path): pos is n x 3, dist n, grad n x 3 (nullable)
  void GetDistanceBatch(const double *pos, int64_t n, double *dist) { ck(fiesta_hip_get_distance_pos(h_, pos, n, dist)); }
  void GetDistWithGradTrilinearBatch(const double *pos, int64_t n, double *dist, double *grad) {
    ck(fiesta_hip_get_dist_grad(h_, pos, n, dist, grad));
  }

  // Path clearance (fiesta_hip_path_clearance; no reference counterpart -- its callers loop over GetDistWithGradTrilinear).
  // The minimum of GetDistWithGradTrilinear over the samples of the polyline `waypoints` (spacing `step`, the sample rule of
  // include/fiesta_hip.h: PathSample below), and optionally the gradient at the first minimal sample and the first sample whose
  // value is < margin (-1 / NaN position if none).  +inf for no waypoints, NaN for an invalid path (non-finite waypoint, a
  // segment longer than 2^24 steps).  A path of at most 256 samples is answered from the host brick cache.
  double GetMinDistanceAlongPath(const std::vector<Eigen::Vector3d> &waypoints, double step, double margin,
                                 Eigen::Vector3d *grad_at_min = nullptr, int64_t *first_below = nullptr,
                                 Eigen::Vector3d *first_below_pos = nullptr) {
    std::vector<double> w(3 * waypoints.size() + 3);  // (one spare triple: never a null pointer)
    for (size_t i = 0; i < waypoints.size(); ++i)
      for (int c = 0; c < 3; ++c) w[3 * i + c] = waypoints[i](c);
    const int64_t off[2] = {0, (int64_t)waypoints.size()};
    double md = 0, g[3] = {0, 0, 0}, fp[3] = {0, 0, 0};
    int64_t fb = -1;
    const fiesta_hip_path_result r{&md, nullptr, nullptr, g, &fb, fp, nullptr};
    ck(fiesta_hip_path_clearance(h_, w.data(), off[1], off, 1, step, margin, &r));
    if (grad_at_min) *grad_at_min = Eigen::Vector3d(g[0], g[1], g[2]);
    if (first_below) *first_below = fb;
    if (first_below_pos) *first_below_pos = Eigen::Vector3d(fp[0], fp[1], fp[2]);
    return md;
  }
  // The batch form: n_paths polylines in CSR form (path p = waypoints[offsets[p] .. offsets[p+1]-1], n_waypoints x 3), one
  // entry per path in every non-null array of `result` (fiesta_hip_path_result: min_dist, min_index, min_pos, min_grad,
  // first_below, first_below_pos, n_samples).
  void PathClearanceBatch(const double *waypoints, int64_t n_waypoints, const int64_t *offsets, int64_t n_paths, double step,
                          double margin, const fiesta_hip_path_result &result) {
    ck(fiesta_hip_path_clearance(h_, waypoints, n_waypoints, offsets, n_paths, step, margin, &result));
  }
  // Path cost (fiesta_hip_path_cost; no reference counterpart): the penalty (margin - d)^2 of GetDistWithGradTrilinear below
  // `margin`, integrated along the polyline `waypoints` by the trapezoid rule over the samples of PathSample, and optionally its
  // derivative with respect to every waypoint (grad->size() == waypoints.size(): the descent direction of a trajectory
  // optimiser) and the number of samples below the margin.  0 for fewer than two waypoints, NaN for an invalid path.  A path of
  // at most 256 samples is answered from the host brick cache.  The formulas: include/fiesta_hip.h.
  double GetPathCost(const std::vector<Eigen::Vector3d> &waypoints, double step, double margin,
                     std::vector<Eigen::Vector3d> *grad = nullptr, int64_t *n_below = nullptr) {
    std::vector<double> w(3 * waypoints.size() + 3), g(3 * waypoints.size() + 3);  // (one spare triple: never a null pointer)
    for (size_t i = 0; i < waypoints.size(); ++i)
      for (int c = 0; c < 3; ++c) w[3 * i + c] = waypoints[i](c);
    const int64_t off[2] = {0, (int64_t)waypoints.size()};
    double cost = 0;
    int64_t nb = 0;
    const fiesta_hip_path_cost_result r{&cost, g.data(), nullptr, &nb, nullptr};
    ck(fiesta_hip_path_cost(h_, w.data(), off[1], off, 1, step, margin, &r));
    if (grad) {
      grad->resize(waypoints.size());
      for (size_t i = 0; i < waypoints.size(); ++i) (*grad)[i] = Eigen::Vector3d(g[3 * i], g[3 * i + 1], g[3 * i + 2]);
    }
    if (n_below) *n_below = nb;
    return cost;
  }
  // The batch form: CSR polylines as PathClearanceBatch; `result` (fiesta_hip_path_cost_result) holds one entry per path in cost,
  // length, n_below, n_samples and one row per WAYPOINT in grad; every pointer is nullable.
  void PathCostBatch(const double *waypoints, int64_t n_waypoints, const int64_t *offsets, int64_t n_paths, double step, double margin,
                     const fiesta_hip_path_cost_result &result) {
    ck(fiesta_hip_path_cost(h_, waypoints, n_waypoints, offsets, n_paths, step, margin, &result));
  }
  // Body queries (fiesta_hip_body_query; no reference counterpart): the robot as a set of spheres -- body-frame centre cx, cy, cz and
  // radius r each -- checked at a batch of poses: position pos[i] (metres) and rotation rot[i] = qw, qx, qy, qz (it need not be
  // normalised).  Per pose: the minimum of d - r over the spheres (d: GetDistWithGradTrilinear at the sphere's world centre), the
  // lowest sphere that attains it, that sphere's position and gradient, the spheres below `margin`, the penalty sum (margin - (d - r))^2
  // over those, its derivative with respect to the position (grad[0..2]) and to a small world-frame rotation about the body origin
  // (grad[3..5]), and every sphere's clearance (row-major, spheres.size() per pose).  An invalid pose (a non-finite number, a zero
  // quaternion) reads NaN / -1 and a gradient of 0.  Always answered on the device.  The formulas: include/fiesta_hip.h.
  // (The rotation is four plain doubles and a sphere an array of four: the vector types of this header have three components.)
  typedef std::vector<std::array<double, 4>> BodySpheres;
  struct BodyResult {
    std::vector<double> min_clearance;
    std::vector<int32_t> min_sphere;
    std::vector<Eigen::Vector3d> min_pos, min_grad;
    std::vector<int32_t> n_below;
    std::vector<double> cost;
    std::vector<std::array<double, 6>> grad;
    std::vector<double> sphere_clearance;
    size_t count() const { return min_clearance.size(); }
  };
  BodyResult BodyQueryBatch(const BodySpheres &spheres, const std::vector<Eigen::Vector3d> &pos, const std::vector<std::array<double, 4>> &rot,
                            double margin) {
    if (pos.size() != rot.size()) throw std::invalid_argument("BodyQueryBatch: pos and rot differ in length");
    const size_t n = pos.size(), k = spheres.size();
    std::vector<double> sph(4 * k + 4), poses(7 * n + 7), mp(3 * n + 3), mg(3 * n + 3), g(6 * n + 6);  // (spare rows: never a null pointer)
    for (size_t i = 0; i < k; ++i)
      for (int c = 0; c < 4; ++c) sph[4 * i + c] = spheres[i][c];
    for (size_t i = 0; i < n; ++i) {
      for (int c = 0; c < 3; ++c) poses[7 * i + c] = pos[i](c);
      for (int c = 0; c < 4; ++c) poses[7 * i + 3 + c] = rot[i][c];
    }
    BodyResult out;
    out.min_clearance.resize(n + 1), out.min_sphere.resize(n + 1), out.n_below.resize(n + 1), out.cost.resize(n + 1);
    out.sphere_clearance.resize(n * k + 1);
    const fiesta_hip_body_result r{out.min_clearance.data(), out.min_sphere.data(), mp.data(), mg.data(), out.n_below.data(), out.cost.data(),
                                   g.data(), out.sphere_clearance.data()};
    ck(fiesta_hip_body_query(h_, sph.data(), (int32_t)k, poses.data(), (int64_t)n, margin, &r));
    out.min_clearance.resize(n), out.min_sphere.resize(n), out.n_below.resize(n), out.cost.resize(n), out.sphere_clearance.resize(n * k);
    out.min_pos.resize(n), out.min_grad.resize(n), out.grad.resize(n);
    for (size_t i = 0; i < n; ++i) {
      out.min_pos[i] = Eigen::Vector3d(mp[3 * i], mp[3 * i + 1], mp[3 * i + 2]);
      out.min_grad[i] = Eigen::Vector3d(mg[3 * i], mg[3 * i + 1], mg[3 * i + 2]);
      for (int c = 0; c < 6; ++c) out.grad[i][c] = g[6 * i + c];
    }
    return out;
  }
  // The scalar convenience: does the body keep `margin` from every obstacle at this pose?  (false for an invalid pose)
  bool IsPoseFree(const BodySpheres &spheres, const Eigen::Vector3d &pos, const std::array<double, 4> &rot, double margin) {
    return BodyQueryBatch(spheres, {pos}, {rot}, margin).min_clearance[0] >= margin;
  }
  // Articulated body queries (fiesta_hip_articulated_query; no reference counterpart): spheres on FRAMES -- the links of an arm, a
  // drone and its slung load, the robots of a formation.  sphere_frame[i] is the frame of sphere i, non-decreasing over the table
  // (the spheres are grouped by frame; a frame may own none), a sphere's centre is given in the frame of its own link.  frame_poses
  // holds one pose per configuration and frame, configuration-major, seven doubles each: px, py, pz, qw, qx, qy, qz (it need not be
  // normalised); the number of configurations is frame_poses.size() / (7 * n_frames).  Forward kinematics is the caller's.  Per
  // configuration: BodyQueryBatch's minimum, sphere, position, gradient, count and cost over all spheres.  Per configuration and
  // frame (row-major, n_frames per configuration): the minimum clearance of the frame's spheres (+inf without spheres), their cost,
  // and its derivative with respect to the frame's position (frame_grad[..][0..2]) and to a small world-frame rotation about the
  // frame's origin (frame_grad[..][3..5]) -- what a caller multiplies with its geometric Jacobian.  An invalid configuration (a
  // non-finite number or a zero quaternion in ANY of its frame poses) reads NaN / -1 and gradients of 0.  Self-collision between
  // the links is not checked.  Always answered on the device.  The formulas: include/fiesta_hip.h.
  struct ArticulatedResult {
    std::vector<double> min_clearance;
    std::vector<int32_t> min_sphere;
    std::vector<Eigen::Vector3d> min_pos, min_grad;
    std::vector<int32_t> n_below;
    std::vector<double> cost;
    std::vector<double> frame_clearance, frame_cost;
    std::vector<std::array<double, 6>> frame_grad;
    std::vector<double> sphere_clearance;
    size_t count() const { return min_clearance.size(); }
  };
  ArticulatedResult ArticulatedQueryBatch(const BodySpheres &spheres, const std::vector<int32_t> &sphere_frame, int n_frames,
                                          const std::vector<double> &frame_poses, double margin) {
    if (sphere_frame.size() != spheres.size()) throw std::invalid_argument("ArticulatedQueryBatch: spheres and sphere_frame differ in length");
    if (n_frames < 1 || frame_poses.size() % (7 * (size_t)n_frames)) throw std::invalid_argument("ArticulatedQueryBatch: frame_poses is not n x n_frames x 7");
    const size_t k = spheres.size(), f = (size_t)n_frames, n = frame_poses.size() / (7 * f);
    std::vector<double> sph(4 * k + 4), poses(frame_poses), mp(3 * n + 3), mg(3 * n + 3), g(6 * n * f + 6);  // (spare rows: never a null pointer)
    std::vector<int32_t> frm(sphere_frame);
    poses.resize(7 * n * f + 7), frm.resize(k + 1);
    for (size_t i = 0; i < k; ++i)
      for (int c = 0; c < 4; ++c) sph[4 * i + c] = spheres[i][c];
    ArticulatedResult out;
    out.min_clearance.resize(n + 1), out.min_sphere.resize(n + 1), out.n_below.resize(n + 1), out.cost.resize(n + 1);
    out.frame_clearance.resize(n * f + 1), out.frame_cost.resize(n * f + 1), out.sphere_clearance.resize(n * k + 1);
    const fiesta_hip_articulated_result r{out.min_clearance.data(), out.min_sphere.data(), mp.data(), mg.data(), out.n_below.data(), out.cost.data(),
                                          out.frame_clearance.data(), out.frame_cost.data(), g.data(), out.sphere_clearance.data()};
    ck(fiesta_hip_articulated_query(h_, sph.data(), frm.data(), (int32_t)k, (int32_t)n_frames, poses.data(), (int64_t)n, margin, &r));
    out.min_clearance.resize(n), out.min_sphere.resize(n), out.n_below.resize(n), out.cost.resize(n), out.sphere_clearance.resize(n * k);
    out.frame_clearance.resize(n * f), out.frame_cost.resize(n * f);
    out.min_pos.resize(n), out.min_grad.resize(n), out.frame_grad.resize(n * f);
    for (size_t i = 0; i < n; ++i) {
      out.min_pos[i] = Eigen::Vector3d(mp[3 * i], mp[3 * i + 1], mp[3 * i + 2]);
      out.min_grad[i] = Eigen::Vector3d(mg[3 * i], mg[3 * i + 1], mg[3 * i + 2]);
    }
    for (size_t i = 0; i < n * f; ++i)
      for (int c = 0; c < 6; ++c) out.frame_grad[i][c] = g[6 * i + c];
    return out;
  }
  // The scalar convenience: does the body keep `margin` from every obstacle in this ONE configuration (frame_poses: n_frames x 7)?
  // (false for an invalid configuration)
  bool IsConfigurationFree(const BodySpheres &spheres, const std::vector<int32_t> &sphere_frame, int n_frames,
                           const std::vector<double> &frame_poses, double margin) {
    if (n_frames < 1 || frame_poses.size() != 7 * (size_t)n_frames) throw std::invalid_argument("IsConfigurationFree: frame_poses is not n_frames x 7");
    return ArticulatedQueryBatch(spheres, sphere_frame, n_frames, frame_poses, margin).min_clearance[0] >= margin;
  }

  // Body sweeps (fiesta_hip_body_sweep; no reference counterpart): the body of BodyQueryBatch moved along polylines of waypoint poses
  // (px, py, pz, qw, qx, qy, qz each) -- path p is the poses offsets[p] .. offsets[p + 1] - 1.  The poses between two waypoints are sampled on the
  // device (positions as PathSample's, rotations along the shorter arc, `step` metres of travel of any sphere centre per sample for
  // turns up to 90 degrees) and each is evaluated as BodyQueryBatch evaluates a pose.  Per path: the minimum of d - r over all samples
  // and spheres with its sample index, sphere, pose (position, then qw, qx, qy, qz), sphere position and gradient; the first sample
  // with a sphere below `margin`, that sphere and that pose (-1 / NaN if none); the number of such samples; the sample count (0: an
  // empty path, -1: an invalid one -- an invalid waypoint pose, a segment of more than 2^24 samples).  A sampled check, as
  // PathClearanceBatch is.  Always answered on the device.  The formulas: include/fiesta_hip.h.
  struct SweepResult {
    std::vector<double> min_clearance;
    std::vector<int64_t> min_sample;
    std::vector<int32_t> min_sphere;
    std::vector<std::array<double, 7>> min_pose;
    std::vector<Eigen::Vector3d> min_pos, min_grad;
    std::vector<int64_t> first_below;
    std::vector<int32_t> first_below_sphere;
    std::vector<std::array<double, 7>> first_below_pose;
    std::vector<int64_t> n_below, n_samples;
    size_t count() const { return min_clearance.size(); }
  };
  typedef std::vector<std::array<double, 7>> BodyPoses;
  SweepResult BodySweepBatch(const BodySpheres &spheres, const BodyPoses &waypoints, const std::vector<int64_t> &offsets, double step,
                             double margin) {
    if (offsets.empty()) throw std::invalid_argument("BodySweepBatch: offsets needs n_paths + 1 entries");
    const size_t n = offsets.size() - 1, np = waypoints.size(), k = spheres.size();
    std::vector<double> sph(4 * k + 4), poses(7 * np + 7), mq(7 * n + 7), mp(3 * n + 3), mg(3 * n + 3), fq(7 * n + 7);  // (spare rows: never a null pointer)
    for (size_t i = 0; i < k; ++i)
      for (int c = 0; c < 4; ++c) sph[4 * i + c] = spheres[i][c];
    for (size_t i = 0; i < np; ++i)
      for (int c = 0; c < 7; ++c) poses[7 * i + c] = waypoints[i][c];
    SweepResult out;
    out.min_clearance.resize(n + 1), out.min_sample.resize(n + 1), out.min_sphere.resize(n + 1), out.first_below.resize(n + 1);
    out.first_below_sphere.resize(n + 1), out.n_below.resize(n + 1), out.n_samples.resize(n + 1);
    const fiesta_hip_sweep_result r{out.min_clearance.data(), out.min_sample.data(),         out.min_sphere.data(), mq.data(),
                                    mp.data(),                mg.data(),                     out.first_below.data(), out.first_below_sphere.data(),
                                    fq.data(),                out.n_below.data(),            out.n_samples.data()};
    ck(fiesta_hip_body_sweep(h_, sph.data(), (int32_t)k, poses.data(), (int64_t)np, offsets.data(), (int64_t)n, step, margin, &r));
    out.min_clearance.resize(n), out.min_sample.resize(n), out.min_sphere.resize(n), out.first_below.resize(n);
    out.first_below_sphere.resize(n), out.n_below.resize(n), out.n_samples.resize(n);
    out.min_pose.resize(n), out.min_pos.resize(n), out.min_grad.resize(n), out.first_below_pose.resize(n);
    for (size_t i = 0; i < n; ++i) {
      out.min_pos[i] = Eigen::Vector3d(mp[3 * i], mp[3 * i + 1], mp[3 * i + 2]);
      out.min_grad[i] = Eigen::Vector3d(mg[3 * i], mg[3 * i + 1], mg[3 * i + 2]);
      for (int c = 0; c < 7; ++c) out.min_pose[i][c] = mq[7 * i + c], out.first_below_pose[i][c] = fq[7 * i + c];
    }
    return out;
  }
  // The scalar convenience: does the body keep `margin` from every obstacle along this ONE polyline of poses, sampled every `step`?
  // (false for an empty or an invalid polyline)
  bool IsMotionFree(const BodySpheres &spheres, const BodyPoses &waypoints, double step, double margin) {
    const SweepResult r = BodySweepBatch(spheres, waypoints, {0, (int64_t)waypoints.size()}, step, margin);
    return r.n_samples[0] > 0 && r.first_below[0] < 0;
  }

  // Sample `index` of the polyline by the header's rule, on the host (bit for bit what the library evaluates there); NaN if the
  // path has no such sample or is invalid.  Header-only, so compiled with the includer's flags: the exactness include/fiesta_hip.h
  // promises holds only without floating-point contraction -- build the including file with -ffp-contract=off.  g++'s default
  // for C++ is "fast": on an FMA target (-march=native, -mfma, ...) it may fuse d0*d0 + d1*d1 or a + d*t, which can change S by
  // one and move every later sample.
  static Eigen::Vector3d PathSample(const std::vector<Eigen::Vector3d> &waypoints, double step, int64_t index) {
    const double nan = std::nan("");
    Eigen::Vector3d out(nan, nan, nan);
    if (waypoints.empty() || index < 0) return out;
    for (size_t i = 0; i < waypoints.size(); ++i) {
      const Eigen::Vector3d &a = waypoints[i];
      if (!std::isfinite(a(0)) || !std::isfinite(a(1)) || !std::isfinite(a(2))) return Eigen::Vector3d(nan, nan, nan);
      if (i + 1 == waypoints.size()) {
        if (index == 0) out = a;  // the final sample: the last waypoint itself
        break;
      }
      const Eigen::Vector3d &b = waypoints[i + 1];
      const double d0 = b(0) - a(0), d1 = b(1) - a(1), d2 = b(2) - a(2);
      const double L = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      const double q = L / step;
      if (!(q <= 16777216.0)) return Eigen::Vector3d(nan, nan, nan);  // L / step > 2^24 (or NaN): an invalid path
      const int64_t S = std::max<int64_t>(1, (int64_t)std::ceil(q));
      if (index >= 0 && index < S) {
        const double t = (double)index / (double)S;
        out = Eigen::Vector3d(a(0) + d0 * t, a(1) + d1 * t, a(2) + d2 * t);
      }
      index -= S;
    }
    return out;
  }

  // Local Range (src/ESDFMap.cpp:792-824)
  void SetUpdateRange(Eigen::Vector3d min_pos, Eigen::Vector3d max_pos, bool new_vec = true) {
    Flush();  // pending observations were made under the old window
    const double a[3] = {min_pos(0), min_pos(1), min_pos(2)}, b[3] = {max_pos(0), max_pos(1), max_pos(2)};
    ck(fiesta_hip_set_update_range(h_, a, b, new_vec ? 1 : 0));
  }
  void SetOriginalRange() {
    Flush();
    ck(fiesta_hip_set_original_range(h_));
  }

  // Visualisation, as plain arrays (reference: GetPointCloud / GetSliceMarker, src/ESDFMap.cpp:544-699)
  void GetOccupiedVoxels(std::vector<Eigen::Vector3d> *centres) {
    Flush();
    centres->clear();
    int64_t n = 0;
    ck(fiesta_hip_get_occupied_voxels(h_, nullptr, 0, &n));
    std::vector<int32_t> vox((size_t)3 * n);
    if (n) ck(fiesta_hip_get_occupied_voxels(h_, vox.data(), n, &n));
    for (int64_t i = 0; i < n; ++i)  // voxel centres, as GetPointCloud emits them (src/ESDFMap.cpp:560-575)
      centres->push_back(Eigen::Vector3d((vox[3 * i] + 0.5) * res_ + origin_[0], (vox[3 * i + 1] + 0.5) * res_ + origin_[1],
                                         (vox[3 * i + 2] + 0.5) * res_ + origin_[2]));
  }
  // Frontier voxels (fiesta_hip_get_frontier_voxels, include/fiesta_hip.h): the observed, unoccupied voxels with a never-observed
  // 6-neighbour inside the inclusive voxel box [lo, hi], optionally only those with GetDistance >= min_clearance; `mask` receives
  // the unknown-neighbour bits (bit 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z) of out[i].  Order unspecified.  An exploration planner calls
  // it with the bounding box of the last sensor frame.
  void GetFrontierVoxels(const Eigen::Vector3i &lo, const Eigen::Vector3i &hi, double min_clearance, std::vector<Eigen::Vector3i> &out,
                         std::vector<uint8_t> *mask = nullptr) {
    const int32_t a[3] = {lo(0), lo(1), lo(2)}, b[3] = {hi(0), hi(1), hi(2)};
    FrontierVoxels(a, b, min_clearance, out, mask);
  }
  // ... of the whole map
  void GetFrontierVoxels(double min_clearance, std::vector<Eigen::Vector3i> &out, std::vector<uint8_t> *mask = nullptr) {
    FrontierVoxels(nullptr, nullptr, min_clearance, out, mask);
  }
  // Skeleton voxels (fiesta_hip_get_skeleton_voxels, include/fiesta_hip.h): the free voxels on the distance field's ridge -- a
  // 6-neighbour names a closest obstacle at least sqrt(min_sep2) voxels from the voxel's own, and the bisector of the two passes
  // between them -- inside the inclusive voxel box [lo, hi] (both null: the whole map), optionally only those with GetDistance >=
  // min_clearance.  Entry i of every vector describes vox[i]: the ridge-neighbour bits (bit 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z), the
  // voxel's own squared distance in voxels, the largest separation (squared) over the mask's bits.  Order unspecified.  min_sep2 up
  // to 4 marks the neighbourhood of every flat surface; prune by angle from sep2 and d2.  ClusterVoxels with d2 as the key names each
  // cluster's narrowest member: the bottleneck of the passage.
  struct SkeletonVoxels {
    std::vector<Eigen::Vector3i> vox;
    std::vector<uint8_t> mask;
    std::vector<int32_t> d2, sep2;
    size_t count() const { return vox.size(); }
  };
  SkeletonVoxels GetSkeletonVoxels(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, int32_t min_sep2, double min_clearance = 0.0) {
    if ((lo == nullptr) != (hi == nullptr)) throw std::invalid_argument("GetSkeletonVoxels: lo and hi must both be given or both be null");
    Flush();
    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    for (int c = 0; lo && c < 3; ++c) a[c] = (*lo)(c), b[c] = (*hi)(c);
    const int32_t *pa = lo ? a : nullptr, *pb = lo ? b : nullptr;
    int64_t n = 0;
    const fiesta_hip_skeleton_result none{nullptr, nullptr, nullptr, nullptr};
    ck(fiesta_hip_get_skeleton_voxels(h_, pa, pb, min_sep2, min_clearance, 0, &none, &n));  // sizes the buffers
    SkeletonVoxels out;
    std::vector<int32_t> vox((size_t)3 * n + 1);  // (one spare entry in every array: never a null pointer)
    out.mask.assign((size_t)n + 1, 0), out.d2.assign((size_t)n + 1, 0), out.sep2.assign((size_t)n + 1, 0);
    const fiesta_hip_skeleton_result r{vox.data(), out.mask.data(), out.d2.data(), out.sep2.data()};
    if (n) ck(fiesta_hip_get_skeleton_voxels(h_, pa, pb, min_sep2, min_clearance, n, &r, &n));
    out.mask.resize((size_t)n), out.d2.resize((size_t)n), out.sep2.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) out.vox.push_back(Eigen::Vector3i(vox[3 * i], vox[3 * i + 1], vox[3 * i + 2]));
    return out;
  }
  // Ray queries (fiesta_hip_ray_query, include/fiesta_hip.h): what a sensor ray from `start` to `end` would cross, read-only.  The
  // walk is the ray cast's; a voxel is FREE, OCCUPIED, UNKNOWN (never observed) or OUTSIDE (dense maps), and the query stops at
  // the first voxel whose class is in stop_mask (FIESTA_HIP_RAY_OCCUPIED | _UNKNOWN | _OUTSIDE).  Line of sight through known free
  // space: stop_mask 7 and no hit; the gain of a view: stop_mask 1, counts[2]; expected depth: stop_mask 1 or 3, hit_dist.
  // Every call is one kernel launch and one synchronisation, whatever the number of rays: batch them.
  struct RayHit {
    int32_t n_visited = -1, hit_index = -1;  // n_visited -1: an invalid ray (non-finite, too far out, more than 4095 voxel steps)
    uint8_t hit_class = 0;
    Eigen::Vector3i hit_vox = Eigen::Vector3i(INT32_MIN, INT32_MIN, INT32_MIN);
    double hit_dist = std::nan("");
    int32_t counts[4] = {0, 0, 0, 0};        // free, occupied, unknown, outside voxels before the hit
    bool valid() const { return n_visited >= 0; }
    bool hit() const { return hit_index >= 0; }
  };
  // n rays, start / end n x 3 doubles (metres); `result` (fiesta_hip_ray_result) holds one entry per ray, every pointer nullable
  void RayQueryBatch(const double *start, const double *end, int64_t n, int32_t stop_mask, const fiesta_hip_ray_result &result) {
    ck(fiesta_hip_ray_query(h_, start, end, n, stop_mask, &result));
  }
  RayHit RayQuery(const Eigen::Vector3d &start, const Eigen::Vector3d &end, int32_t stop_mask) {
    const double a[3] = {start(0), start(1), start(2)}, b[3] = {end(0), end(1), end(2)};
    RayHit h;
    int32_t v[3];
    const fiesta_hip_ray_result r{&h.n_visited, &h.hit_index, &h.hit_class, v, &h.hit_dist, h.counts};
    ck(fiesta_hip_ray_query(h_, a, b, 1, stop_mask, &r));
    h.hit_vox = Eigen::Vector3i(v[0], v[1], v[2]);
    return h;
  }
  // true iff the segment is a valid ray and crosses nothing but voxels observed free (no occupied, unknown or outside voxel)
  bool IsSegmentFree(const Eigen::Vector3d &a, const Eigen::Vector3d &b) {
    const RayHit h = RayQuery(a, b, FIESTA_HIP_RAY_OCCUPIED | FIESTA_HIP_RAY_UNKNOWN | FIESTA_HIP_RAY_OUTSIDE);
    return h.valid() && !h.hit();
  }
  // Reachability (fiesta_hip_reach_field, include/fiesta_hip.h): the travel cost from `seeds` through the traversable voxels of the
  // inclusive voxel box [lo, hi] (both null: a dense map's whole array) -- observed free, with GetDistance >= min_clearance if that
  // is > 0, with flags = FIESTA_HIP_REACH_THROUGH_UNKNOWN the never-observed ones too -- by moves of weight 3 / 4 / 5 (connectivity
  // 26; 6: only 3), so metres ~ cost * resolution / 3.  target_cost (nullable) receives one cost per target: -1 not traversable or
  // outside the box, INT32_MAX traversable and out of reach.  cost (nullable) receives the whole field of the clipped box, x-major,
  // z fastest, from info.box_lo.  The frontier call's voxels are the usual targets: which of them can the robot reach, and how far?
  fiesta_hip_reach_info ReachField(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, const std::vector<Eigen::Vector3i> &seeds,
                                   const std::vector<Eigen::Vector3i> &targets, double min_clearance, int32_t connectivity, int32_t flags,
                                   std::vector<int32_t> *target_cost, std::vector<int32_t> *cost = nullptr) {
    Flush();
    if ((lo == nullptr) != (hi == nullptr)) throw std::invalid_argument("ReachField: lo and hi must both be given or both be null");
    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    int64_t nvox = 1;  // of the box as the library clips it (a dense map: its array; a hash-block map: +-2^30)
    for (int c = 0; c < 3; ++c) {
      if (lo) a[c] = (*lo)(c), b[c] = (*hi)(c);
      const int64_t l = hash_ ? std::max<int64_t>(a[c], -(1ll << 30)) : (lo ? std::max<int64_t>(a[c], 0) : 0);
      const int64_t h = hash_ ? std::min<int64_t>(b[c], 1ll << 30) : (lo ? std::min<int64_t>(b[c], gs_[c] - 1) : gs_[c] - 1);
      nvox = (l > h || nvox == 0) ? 0 : std::min<int64_t>(nvox * (h - l + 1), (1ll << 28) + 1);
    }
    std::vector<int32_t> sv, tv;
    for (const auto &v : seeds) sv.insert(sv.end(), {v(0), v(1), v(2)});
    for (const auto &v : targets) tv.insert(tv.end(), {v(0), v(1), v(2)});
    if (target_cost) target_cost->assign(targets.size(), -1);
    if (cost) cost->assign(nvox <= (1ll << 28) ? (size_t)nvox : 0, -1);
    const fiesta_hip_reach_result r{cost && !cost->empty() ? cost->data() : nullptr,
                                    target_cost && !targets.empty() ? target_cost->data() : nullptr};
    fiesta_hip_reach_info info{};
    ck(fiesta_hip_reach_field(h_, lo ? a : nullptr, lo ? b : nullptr, sv.empty() ? nullptr : sv.data(), (int64_t)seeds.size(),
                              tv.empty() ? nullptr : tv.data(), (int64_t)targets.size(), min_clearance, connectivity, flags, &r, &info));
    return info;
  }
  // Reach matrix (fiesta_hip_reach_matrix, include/fiesta_hip.h): the travel cost from every source -- each a flood of its own from
  // that one voxel, ReachField's box, clearance, flags and connectivity -- to every target; an empty `targets` selects the square
  // form (the columns are the sources), the cost matrix a tour solver takes.  *cost (nullable) receives sources x columns values,
  // row-major: ReachField's target cost, or -1 along the whole row of a source that is outside the box or not traversable
  // (*source_status, nullable: FIESTA_HIP_REACH_SITE_*), so the square form is symmetric.  The floods share one traversability
  // bitmap and run side by side, at most max_fields at a time (0: as many as fit); the field ReachPaths retains is left alone.
  fiesta_hip_reach_matrix_info ReachMatrix(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, const std::vector<Eigen::Vector3i> &sources,
                                           const std::vector<Eigen::Vector3i> &targets, double min_clearance, int32_t connectivity, int32_t flags,
                                           std::vector<int32_t> *cost, std::vector<int32_t> *source_status = nullptr, int32_t max_fields = 0) {
    Flush();
    if ((lo == nullptr) != (hi == nullptr)) throw std::invalid_argument("ReachMatrix: lo and hi must both be given or both be null");
    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    for (int c = 0; c < 3 && lo; ++c) a[c] = (*lo)(c), b[c] = (*hi)(c);
    std::vector<int32_t> sv, tv;
    for (const auto &v : sources) sv.insert(sv.end(), {v(0), v(1), v(2)});
    for (const auto &v : targets) tv.insert(tv.end(), {v(0), v(1), v(2)});
    const size_t n = sources.size(), n_cols = targets.empty() ? n : targets.size();
    if (n && n_cols > ((size_t)1 << 28) / n) throw std::invalid_argument("ReachMatrix: the matrix holds more than 2^28 entries");
    if (cost) cost->assign(n * n_cols, -1);
    if (source_status) source_status->assign(n, FIESTA_HIP_REACH_SITE_OUTSIDE);
    const fiesta_hip_reach_matrix_result r{cost && !cost->empty() ? cost->data() : nullptr,
                                           source_status && n ? source_status->data() : nullptr, nullptr};
    fiesta_hip_reach_matrix_info info{};
    ck(fiesta_hip_reach_matrix(h_, lo ? a : nullptr, lo ? b : nullptr, sv.empty() ? nullptr : sv.data(), (int64_t)n,
                               tv.empty() ? nullptr : tv.data(), (int64_t)targets.size(), min_clearance, connectivity, flags, max_fields, &r, &info));
    return info;
  }
  // Site tour (fiesta_hip_site_tour, include/fiesta_hip.h): the order in which to visit every site that `start` can reach through the
  // symmetric n x n matrix `cost` (ReachMatrix's square form, row-major; ld: its leading dimension, 0 for n), as an open path from
  // the start or a closed tour back to it: `restarts` local searches side by side (2-opt and Or-opt, best improvement), restart 0 from
  // the nearest-neighbour tour, the others from shuffles seeded by `seed`, each applying at most max_moves moves (0: 8 per visited
  // site).  order / leg_cost hold the info.n_visited visited sites, the start first; site_status: FIESTA_HIP_TOUR_SITE_* per site.
  struct SiteTourResult {
    std::vector<int32_t> order, leg_cost, site_status;
    std::vector<int64_t> restart_length;
    fiesta_hip_tour_info info;
  };
  SiteTourResult SiteTour(const std::vector<int32_t> &cost, int32_t n, int32_t start = 0, bool closed = false, int32_t restarts = 64,
                          uint64_t seed = 0, int32_t max_moves = 0, int64_t ld = 0) {
    if (ld == 0) ld = n;
    if (n < 1 || ld < n || cost.size() < (size_t)(n - 1) * (size_t)ld + (size_t)n) throw std::invalid_argument("SiteTour: cost does not hold n rows of ld entries");
    if (restarts < 1 || restarts > FIESTA_HIP_TOUR_MAX_RESTARTS) throw std::invalid_argument("SiteTour: restarts must be 1 .. 4096");
    SiteTourResult out;
    out.order.assign((size_t)n, -1), out.leg_cost.assign((size_t)n, -1), out.site_status.assign((size_t)n, FIESTA_HIP_TOUR_SITE_SKIPPED);
    out.restart_length.assign((size_t)restarts, 0);
    out.info = fiesta_hip_tour_info{};
    const fiesta_hip_tour_result r{out.order.data(), out.site_status.data(), out.leg_cost.data(), out.restart_length.data()};
    ck(fiesta_hip_site_tour(h_, cost.data(), n, ld, start, closed ? FIESTA_HIP_TOUR_CLOSED : 0, restarts, seed, max_moves, &r, &out.info));
    out.order.resize((size_t)out.info.n_visited), out.leg_cost.resize((size_t)out.info.n_visited);
    return out;
  }
  // Reach paths (fiesta_hip_reach_paths, include/fiesta_hip.h): per target voxel the path down a cost-to-go field, from the seed it was
  // reached from to the target.  The field is the one the map retained from the last ReachField call (cost null), or *cost with its
  // inclusive voxel box [box_lo, box_hi] (ReachField's info.box_lo / box_hi) and the connectivity it was flooded with.  shortcut: the
  // staircase pulled tight by line of sight through the field's traversable voxels, at most max_span moves per segment.  offsets is
  // CSR over the waypoints; pos (metres, 3 doubles per waypoint) and offsets are exactly what PathCostBatch and PathClearanceBatch
  // take.  status: FIESTA_HIP_REACH_PATH_*; a target that is not OK has no waypoints and n_moves -1.
  struct ReachPathSet {
    std::vector<int64_t> offsets;  // n_targets + 1
    std::vector<int32_t> vox;      // 3 per waypoint, map voxel coordinates
    std::vector<double> pos;       // 3 per waypoint, metres
    std::vector<int32_t> status, n_moves;
    std::vector<Eigen::Vector3d> Path(size_t p) const {  // the waypoints of target p, seed first
      std::vector<Eigen::Vector3d> out;
      for (int64_t i = offsets[p]; i < offsets[p + 1]; ++i) out.push_back(Eigen::Vector3d(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]));
      return out;
    }
  };
  ReachPathSet ReachPaths(const std::vector<Eigen::Vector3i> &targets, int32_t connectivity = 26, bool shortcut = false, int32_t max_span = 4096,
                          const std::vector<int32_t> *cost = nullptr, const Eigen::Vector3i *box_lo = nullptr,
                          const Eigen::Vector3i *box_hi = nullptr) {
    Flush();
    if ((cost == nullptr) != (box_lo == nullptr) || (cost == nullptr) != (box_hi == nullptr))
      throw std::invalid_argument("ReachPaths: cost, box_lo and box_hi must all be given or all be null");
    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    if (cost) {
      int64_t nvox = 1;
      for (int c = 0; c < 3; ++c) {
        a[c] = (*box_lo)(c), b[c] = (*box_hi)(c);
        nvox = a[c] > b[c] ? 0 : std::min<int64_t>(nvox * ((int64_t)b[c] - a[c] + 1), (1ll << 28) + 1);
      }
      if (nvox != (int64_t)cost->size()) throw std::invalid_argument("ReachPaths: cost does not have the box's number of voxels");
    }
    std::vector<int32_t> tv;
    for (const auto &v : targets) tv.insert(tv.end(), {v(0), v(1), v(2)});
    const int64_t n = (int64_t)targets.size();
    const int32_t flags = shortcut ? FIESTA_HIP_REACH_PATHS_SHORTCUT : 0;
    ReachPathSet out;
    out.offsets.assign((size_t)n + 1, 0);
    out.status.assign((size_t)n + 1, 0), out.n_moves.assign((size_t)n + 1, -1);  // (one spare entry: never a null pointer)
    fiesta_hip_reach_paths_result r{out.offsets.data(), nullptr, nullptr, out.status.data(), out.n_moves.data()};
    ck(fiesta_hip_reach_paths(h_, cost ? cost->data() : nullptr, cost ? a : nullptr, cost ? b : nullptr, tv.empty() ? nullptr : tv.data(), n,
                              connectivity, flags, max_span, 0, &r));  // sizes the buffers (and uploads an explicit field: it is retained)
    out.status.resize((size_t)n), out.n_moves.resize((size_t)n);
    const int64_t total = out.offsets[(size_t)n];
    out.vox.assign((size_t)total * 3, 0), out.pos.assign((size_t)total * 3, 0.0);
    if (total > 0) {
      r = fiesta_hip_reach_paths_result{out.offsets.data(), out.vox.data(), out.pos.data(), nullptr, nullptr};
      ck(fiesta_hip_reach_paths(h_, nullptr, nullptr, nullptr, tv.data(), n, connectivity, flags, max_span, total, &r));
    }
    return out;
  }
  // Leg paths (fiesta_hip_leg_paths, include/fiesta_hip.h): per leg the path from site from[k] -- an index into the sources of the
  // last ReachMatrix call, whose floods the map retains while they fitted one batch (info.batches == 1) -- to site to[k], with nothing
  // flooded again; `to_vox` (non-null: `to` is ignored) names map voxels as targets instead.  shortcut / max_span as in ReachPaths; the
  // connectivity is the retained batch's.  The set is ReachPaths' (each leg from its source to its target: consecutive legs of a
  // tour concatenate) plus cost, the matrix entry of every leg, and info, what is retained.  status: FIESTA_HIP_REACH_PATH_*,
  // FIESTA_HIP_LEG_NO_SOURCE, FIESTA_HIP_LEG_BAD_INDEX.
  struct LegPathsResult {
    ReachPathSet paths;
    std::vector<int32_t> cost;
    fiesta_hip_leg_paths_info info;
  };
  LegPathsResult LegPaths(const std::vector<int32_t> &from, const std::vector<int32_t> &to, bool shortcut = false, int32_t max_span = 4096,
                          const std::vector<Eigen::Vector3i> *to_vox = nullptr) {
    Flush();
    const int64_t n = (int64_t)from.size();
    if ((to_vox ? to_vox->size() : to.size()) != from.size()) throw std::invalid_argument("LegPaths: from and to differ in length");
    std::vector<int32_t> tv;
    for (size_t k = 0; to_vox && k < to_vox->size(); ++k) tv.insert(tv.end(), {(*to_vox)[k](0), (*to_vox)[k](1), (*to_vox)[k](2)});
    const int32_t *pf = n ? from.data() : nullptr, *pt = n && !to_vox ? to.data() : nullptr, *pv = n && to_vox ? tv.data() : nullptr;
    const int32_t flags = shortcut ? FIESTA_HIP_REACH_PATHS_SHORTCUT : 0;
    LegPathsResult out;
    ReachPathSet &p = out.paths;
    p.offsets.assign((size_t)n + 1, 0);
    p.status.assign((size_t)n + 1, 0), p.n_moves.assign((size_t)n + 1, -1), out.cost.assign((size_t)n + 1, -1);  // (one spare entry: never null)
    out.info = fiesta_hip_leg_paths_info{};
    fiesta_hip_leg_paths_result r{p.offsets.data(), nullptr, nullptr, p.status.data(), p.n_moves.data(), out.cost.data()};
    ck(fiesta_hip_leg_paths(h_, pf, pt, pv, n, flags, max_span, 0, &r, &out.info));  // sizes the buffers
    p.status.resize((size_t)n), p.n_moves.resize((size_t)n), out.cost.resize((size_t)n);
    const int64_t total = p.offsets[(size_t)n];
    p.vox.assign((size_t)total * 3, 0), p.pos.assign((size_t)total * 3, 0.0);
    if (total > 0) {
      r = fiesta_hip_leg_paths_result{p.offsets.data(), p.vox.data(), p.pos.data(), nullptr, nullptr, nullptr};
      ck(fiesta_hip_leg_paths(h_, pf, pt, pv, n, flags, max_span, total, &r, nullptr));
    }
    return out;
  }
  // Tour route: ReachMatrix -> SiteTour -> LegPaths.  The order in which to visit `sites` from sites[start] and the way along every
  // leg, the box flooded once per site and never again.  Leg k runs from order[k] to order[k + 1]; a closed tour gets the wrap-around
  // leg order[m - 1] -> order[0] as its last.  All sites must fit one batch of floods (else std::runtime_error).
  struct TourRouteResult {
    std::vector<int32_t> matrix, source_status;  // ReachMatrix: n x n, row-major
    SiteTourResult tour;
    std::vector<int32_t> leg_from, leg_to;
    LegPathsResult legs;
  };
  TourRouteResult TourRoute(const std::vector<Eigen::Vector3i> &sites, int32_t start = 0, bool closed = false, const Eigen::Vector3i *lo = nullptr,
                            const Eigen::Vector3i *hi = nullptr, double min_clearance = 0.0, int32_t connectivity = 26, int32_t flags = 0,
                            int32_t restarts = 64, uint64_t seed = 0, int32_t max_moves = 0, bool shortcut = false, int32_t max_span = 4096) {
    TourRouteResult out;
    const fiesta_hip_reach_matrix_info mi = ReachMatrix(lo, hi, sites, {}, min_clearance, connectivity, flags, &out.matrix, &out.source_status);
    if (mi.batches != 1) throw std::runtime_error("TourRoute: the sites' floods do not fit one batch (or the box is empty)");
    out.tour = SiteTour(out.matrix, (int32_t)sites.size(), start, closed, restarts, seed, max_moves);
    const std::vector<int32_t> &order = out.tour.order;
    const size_t m = order.size();
    for (size_t k = 0; k + 1 < m; ++k) out.leg_from.push_back(order[k]), out.leg_to.push_back(order[k + 1]);
    if (closed && m >= 2) out.leg_from.push_back(order[m - 1]), out.leg_to.push_back(order[0]);
    out.legs = LegPaths(out.leg_from, out.leg_to, shortcut, max_span);
    return out;
  }
  // Free boxes (fiesta_hip_free_boxes, include/fiesta_hip.h): around every seed voxel the axis-aligned box of traversable voxels
  // (ReachField's traversability; flags: FIESTA_HIP_CORRIDOR_THROUGH_UNKNOWN) grown face by face, at most max_grow <= 256 steps per
  // face, inside the inclusive voxel window [lo, hi] (both null: a dense map's whole array, everything on a hash-block map).  box:
  // lo xyz, hi xyz per seed; pos: the box's two corners in metres; stop: FIESTA_HIP_CORRIDOR_STOP_* per face; status:
  // FIESTA_HIP_FREE_BOX_*.
  struct FreeBoxSet {
    std::vector<int32_t> box;  // 6 per seed
    std::vector<double> pos;   // 6 per seed
    std::vector<uint8_t> stop;  // 6 per seed
    std::vector<int64_t> volume;
    std::vector<int32_t> status;
  };
  FreeBoxSet FreeBoxes(const std::vector<Eigen::Vector3i> &seeds, int32_t max_grow = 16, double min_clearance = 0.0, int32_t flags = 0,
                       const Eigen::Vector3i *lo = nullptr, const Eigen::Vector3i *hi = nullptr) {
    Flush();
    if ((lo == nullptr) != (hi == nullptr)) throw std::invalid_argument("FreeBoxes: lo and hi must both be given or both be null");
    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    if (lo)
      for (int c = 0; c < 3; ++c) a[c] = (*lo)(c), b[c] = (*hi)(c);
    std::vector<int32_t> sv;
    for (const auto &v : seeds) sv.insert(sv.end(), {v(0), v(1), v(2)});
    const size_t n = seeds.size();
    FreeBoxSet out;
    out.box.assign(6 * n + 1, 0), out.pos.assign(6 * n + 1, 0.0), out.stop.assign(6 * n + 1, 0);  // (one spare entry: never a null pointer)
    out.volume.assign(n + 1, 0), out.status.assign(n + 1, 0);
    const fiesta_hip_free_boxes_result r{out.box.data(), out.pos.data(), out.stop.data(), out.volume.data(), out.status.data()};
    ck(fiesta_hip_free_boxes(h_, lo ? a : nullptr, lo ? b : nullptr, sv.empty() ? nullptr : sv.data(), (int64_t)n, min_clearance, max_grow, flags, &r));
    out.box.resize(6 * n), out.pos.resize(6 * n), out.stop.resize(6 * n), out.volume.resize(n), out.status.resize(n);
    return out;
  }
  // Path corridors (fiesta_hip_path_corridor, include/fiesta_hip.h): for every voxel polyline of a CSR batch -- ReachPathSet's vox and
  // offsets as they come -- the safe flight corridor: overlapping boxes inflated as by FreeBoxes along the path's voxel chain, a new
  // box wherever the chain leaves the last one.  offsets is CSR over the boxes; status: FIESTA_HIP_CORRIDOR_*; a BLOCKED path keeps
  // the boxes made so far and names the segment and the voxel.
  struct CorridorSet {
    std::vector<int64_t> offsets;  // n_paths + 1
    std::vector<int32_t> boxes;    // 6 per box: lo xyz, hi xyz
    std::vector<double> pos;       // 6 per box, metres
    std::vector<uint8_t> stop;     // 6 per box
    std::vector<int32_t> entry;    // per box: the chain index at which it was made
    std::vector<int32_t> status, n_chain, blocked_segment, blocked_vox;  // per path (blocked_vox: 3 per path)
  };
  CorridorSet PathCorridor(const std::vector<int32_t> &waypoints_vox, const std::vector<int64_t> &offsets, int32_t max_grow = 16,
                           double min_clearance = 0.0, int32_t flags = 0, const Eigen::Vector3i *lo = nullptr, const Eigen::Vector3i *hi = nullptr) {
    Flush();
    if ((lo == nullptr) != (hi == nullptr)) throw std::invalid_argument("PathCorridor: lo and hi must both be given or both be null");
    if (offsets.empty() || waypoints_vox.size() % 3 != 0) throw std::invalid_argument("PathCorridor: offsets needs n_paths + 1 entries, waypoints 3 each");
    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    if (lo)
      for (int c = 0; c < 3; ++c) a[c] = (*lo)(c), b[c] = (*hi)(c);
    const size_t n = offsets.size() - 1;
    const int64_t nw = (int64_t)(waypoints_vox.size() / 3);
    CorridorSet out;
    out.offsets.assign(n + 1, 0);
    out.status.assign(n + 1, 0), out.n_chain.assign(n + 1, 0), out.blocked_segment.assign(n + 1, -1), out.blocked_vox.assign(3 * n + 1, 0);
    fiesta_hip_corridor_result r{out.offsets.data(), nullptr, nullptr, nullptr, nullptr, out.status.data(), out.n_chain.data(),
                                 out.blocked_segment.data(), out.blocked_vox.data()};
    const int32_t *wp = waypoints_vox.empty() ? nullptr : waypoints_vox.data();
    ck(fiesta_hip_path_corridor(h_, lo ? a : nullptr, lo ? b : nullptr, wp, nw, offsets.data(), (int64_t)n, min_clearance, max_grow, flags, 0, &r));
    out.status.resize(n), out.n_chain.resize(n), out.blocked_segment.resize(n), out.blocked_vox.resize(3 * n);
    const int64_t total = out.offsets[n];
    out.boxes.assign((size_t)total * 6, 0), out.pos.assign((size_t)total * 6, 0.0), out.stop.assign((size_t)total * 6, 0);
    out.entry.assign((size_t)total, 0);
    if (total > 0) {
      r = fiesta_hip_corridor_result{out.offsets.data(), out.boxes.data(), out.pos.data(), out.stop.data(), out.entry.data(), nullptr, nullptr, nullptr, nullptr};
      ck(fiesta_hip_path_corridor(h_, lo ? a : nullptr, lo ? b : nullptr, wp, nw, offsets.data(), (int64_t)n, min_clearance, max_grow, flags, total, &r));
    }
    return out;
  }
  // Corridor bounds (fiesta_hip_corridor_bounds, include/fiesta_hip.h): the `bounds` of RefinePaths for the voxel polylines of a CSR
  // batch and the CorridorSet PathCorridor returned for them -- per waypoint its corridor box, intersected with the next one where
  // the path changes boxes, `inset` metres taken off every upper face (negative: resolution * 2^-20, so that a waypoint clamped onto
  // an upper face stays in the box's last voxel).  ok says per path whether the corridor is whole and no box is skipped: every
  // refined segment of such a path stays in traversable space.  With void_broken the rows of the other paths are NaN, which
  // RefinePaths reports INVALID and leaves alone.  box: per waypoint the index of its box in the CorridorSet, -1 if it has none.
  struct BoundsSet {
    std::vector<double> bounds;  // 6 per waypoint: lo xyz, hi xyz, metres
    std::vector<int32_t> ok;     // per path
    std::vector<int64_t> box;    // per waypoint
  };
  BoundsSet CorridorBounds(const std::vector<int32_t> &waypoints_vox, const std::vector<int64_t> &offsets, const CorridorSet &corridor, double inset = -1 /* resolution·2⁻²⁰ */, bool void_broken = false) {
    Flush();
    if (offsets.empty() || waypoints_vox.size() % 3 != 0) throw std::invalid_argument("CorridorBounds: offsets needs n_paths + 1 entries, waypoints 3 each");
    const size_t n = offsets.size() - 1, nw = waypoints_vox.size() / 3, nb = corridor.entry.size();
    if (corridor.offsets.size() != n + 1 || corridor.status.size() != n || corridor.boxes.size() != 6 * nb || corridor.pos.size() != 6 * nb)
      throw std::invalid_argument("CorridorBounds: the corridor does not describe this batch");
    BoundsSet out;
    out.bounds.assign(6 * nw + 1, 0.0), out.ok.assign(n + 1, 0), out.box.assign(nw + 1, -1);
    const fiesta_hip_bounds_result r{out.bounds.data(), out.ok.data(), out.box.data()};
    ck(fiesta_hip_corridor_bounds(h_, nw ? waypoints_vox.data() : nullptr, (int64_t)nw, offsets.data(), (int64_t)n, corridor.offsets.data(),
                                  nb ? corridor.boxes.data() : nullptr, nb ? corridor.pos.data() : nullptr, nb ? corridor.entry.data() : nullptr,
                                  corridor.status.data(), (int64_t)nb, inset < 0 ? res_ * 0x1p-20 : inset, void_broken ? FIESTA_HIP_BOUNDS_VOID_BROKEN : 0, &r));
    out.bounds.resize(6 * nw), out.ok.resize(n), out.box.resize(nw);
    return out;
  }
  // Path refinement (fiesta_hip_path_refine, include/fiesta_hip.h): every path of the CSR batch (waypoints: 3 doubles each, metres,
  // e.g. ReachPathSet::pos and ::offsets) takes p.iterations projected-gradient steps on p.w_obstacle * sum (margin - d)^2 +
  // p.w_smooth * sum |second difference|^2 over its interior waypoints, each clamped to its row of `bounds` (6 doubles per waypoint:
  // lo xyz, hi xyz, e.g. the corridor box it lies in; empty: every waypoint free).  The ends never move; a path stops once an
  // iteration moved it by at most p.tolerance.  The whole loop runs on the device.
  struct RefineParams {
    double margin = 0.5, w_obstacle = 1.0, w_smooth = 1.0, alpha = 0.02, max_step = 0.05, tolerance = 0.0;
    int32_t iterations = 16;
  };
  struct RefineSet {
    std::vector<double> pos;         // 3 per waypoint: the refined positions
    std::vector<double> cost;        // 2 per path: J before, J after
    std::vector<double> last_move;   // per path from here on
    std::vector<int32_t> iterations;
    std::vector<int64_t> n_below;
    std::vector<double> min_dist;
    std::vector<int32_t> status;     // FIESTA_HIP_REFINE_*
  };
  RefineSet RefinePaths(const std::vector<double> &waypoints, const std::vector<int64_t> &offsets, const std::vector<double> &bounds, const RefineParams &p) {
    Flush();
    if (offsets.empty() || waypoints.size() % 3 != 0) throw std::invalid_argument("RefinePaths: offsets needs n_paths + 1 entries, waypoints 3 doubles each");
    if (!bounds.empty() && bounds.size() != 2 * waypoints.size()) throw std::invalid_argument("RefinePaths: bounds needs 6 doubles per waypoint, or none");
    const size_t n = offsets.size() - 1;
    RefineSet out;
    out.pos.assign(waypoints.size() + 1, 0.0), out.cost.assign(2 * n + 1, 0.0), out.last_move.assign(n + 1, 0.0), out.iterations.assign(n + 1, 0);
    out.n_below.assign(n + 1, 0), out.min_dist.assign(n + 1, 0.0), out.status.assign(n + 1, 0);
    const fiesta_hip_refine_params par{p.margin, p.w_obstacle, p.w_smooth, p.alpha, p.max_step, p.tolerance, p.iterations, 0};
    const fiesta_hip_refine_result r{out.pos.data(), out.cost.data(), out.last_move.data(), out.iterations.data(), out.n_below.data(),
                                     out.min_dist.data(), out.status.data()};
    const std::vector<double> none(1, 0.0);  // (the call wants a waypoint pointer even for no waypoints)
    ck(fiesta_hip_path_refine(h_, waypoints.empty() ? none.data() : waypoints.data(), (int64_t)(waypoints.size() / 3), offsets.data(), (int64_t)n,
                              bounds.empty() ? nullptr : bounds.data(), &par, &r));
    out.pos.resize(waypoints.size()), out.cost.resize(2 * n), out.last_move.resize(n), out.iterations.resize(n), out.n_below.resize(n);
    out.min_dist.resize(n), out.status.resize(n);
    return out;
  }
  // Path timing (fiesta_hip_path_timing, include/fiesta_hip.h): how long every path of the CSR batch (waypoints: 3 doubles each,
  // metres, e.g. ReachPathSet::pos and ::offsets, or RefineSet::pos) takes.  Per sample (spacing p.step, the sample rule of
  // PathSample) the speed is limited to the one from which the robot still stops within its free distance d - p.margin (never below
  // p.v_min, never above p.v_max), at every bend by the junction deviation p.corner_dev (metres; infinity: no corner rule), at the
  // ends by p.v_start / p.v_end, and it changes no faster than p.a_max allows.  The whole computation runs on the device.
  struct TimingParams {
    double step = 0.1, margin = 0.3, v_max = 2.0, v_min = 0.1, a_max = 2.0, corner_dev = 0.05, v_start = 0.0, v_end = 0.0;
  };
  struct TimingSet {
    std::vector<double> duration;    // per path from here on: the travel time, seconds
    std::vector<double> length;      // metres
    std::vector<int64_t> n_samples;
    std::vector<int64_t> n_below;    // samples with d < margin (they run at v_min)
    std::vector<double> min_speed;
    std::vector<int64_t> min_index;  // the first sample that runs at min_speed
    std::vector<int32_t> status;     // FIESTA_HIP_TIMING_*
    std::vector<double> time;        // per waypoint: its time stamp
    std::vector<double> speed;       // per waypoint: the speed there
  };
  TimingSet PathTiming(const std::vector<double> &waypoints, const std::vector<int64_t> &offsets, const TimingParams &p) {
    Flush();
    if (offsets.empty() || waypoints.size() % 3 != 0) throw std::invalid_argument("PathTiming: offsets needs n_paths + 1 entries, waypoints 3 doubles each");
    const size_t n = offsets.size() - 1, nw = waypoints.size() / 3;
    TimingSet out;
    out.duration.assign(n + 1, 0.0), out.length.assign(n + 1, 0.0), out.n_samples.assign(n + 1, 0), out.n_below.assign(n + 1, 0);
    out.min_speed.assign(n + 1, 0.0), out.min_index.assign(n + 1, 0), out.status.assign(n + 1, 0);
    out.time.assign(nw + 1, 0.0), out.speed.assign(nw + 1, 0.0);
    const fiesta_hip_timing_params par{p.step, p.margin, p.v_max, p.v_min, p.a_max, p.corner_dev, p.v_start, p.v_end};
    const fiesta_hip_path_timing_result r{out.duration.data(),  out.length.data(), out.n_samples.data(), out.n_below.data(), out.min_speed.data(),
                                          out.min_index.data(), out.status.data(), out.time.data(),      out.speed.data()};
    const std::vector<double> none(1, 0.0);  // (the call wants a waypoint pointer even for no waypoints)
    ck(fiesta_hip_path_timing(h_, waypoints.empty() ? none.data() : waypoints.data(), (int64_t)nw, offsets.data(), (int64_t)n, &par, &r));
    out.duration.resize(n), out.length.resize(n), out.n_samples.resize(n), out.n_below.resize(n), out.min_speed.resize(n);
    out.min_index.resize(n), out.status.resize(n), out.time.resize(nw), out.speed.resize(nw);
    return out;
  }
  // One polyline: its travel time (0 for fewer than two waypoints, NaN for a path the call does not time: a non-finite waypoint, a
  // segment longer than 2^24 steps, more than 1024 waypoints or 4096 samples), optionally every waypoint's time stamp and speed.
  double GetPathDuration(const std::vector<Eigen::Vector3d> &waypoints, const TimingParams &p, std::vector<double> *time = nullptr,
                         std::vector<double> *speed = nullptr) {
    std::vector<double> w(3 * waypoints.size());
    for (size_t i = 0; i < waypoints.size(); ++i)
      for (int c = 0; c < 3; ++c) w[3 * i + c] = waypoints[i](c);
    const TimingSet t = PathTiming(w, {0, (int64_t)waypoints.size()}, p);
    if (time) *time = t.time;
    if (speed) *speed = t.speed;
    return t.duration[0];
  }
  // Voxel clusters (fiesta_hip_cluster_voxels, include/fiesta_hip.h): the connected groups (connectivity 6, 18 or 26) of a voxel list
  // -- typically GetFrontierVoxels' -- with those below min_size distinct voxels dropped and the rest numbered by their lowest entry
  // index.  mask (nullable): the frontier call's unknown-neighbour bits; key (nullable): one int32 per entry, e.g. ReachField's
  // target_cost -- key_min / key_argmin then name each cluster's cheapest reachable member (negative keys are ignored; INT32_MAX
  // and -1: none).  members / offsets: CSR over the entry indices of each cluster's distinct voxels, unordered inside a cluster.
  struct VoxelClusters {
    std::vector<int32_t> label;  // per entry; -1: invalid entry or dropped cluster
    std::vector<int32_t> size;   // per cluster from here on
    std::vector<int64_t> root;
    std::vector<Eigen::Vector3i> box_lo, box_hi;  // inclusive
    std::vector<Eigen::Vector3d> centroid;        // metres
    std::vector<uint8_t> mask_or;
    std::vector<int32_t> key_min;
    std::vector<int64_t> key_argmin;
    std::vector<int64_t> offsets, members;
    fiesta_hip_cluster_info info{};
    size_t count() const { return size.size(); }
  };
  VoxelClusters ClusterVoxels(const std::vector<Eigen::Vector3i> &vox, const std::vector<uint8_t> *mask = nullptr,
                              const std::vector<int32_t> *key = nullptr, int32_t connectivity = 26, int32_t min_size = 1) {
    Flush();
    const int64_t n = (int64_t)vox.size();
    if ((mask && (int64_t)mask->size() != n) || (key && (int64_t)key->size() != n))
      throw std::invalid_argument("ClusterVoxels: mask and key need one value per entry");
    std::vector<int32_t> v;
    for (const auto &p : vox) v.insert(v.end(), {p(0), p(1), p(2)});
    const int32_t *vp = v.empty() ? nullptr : v.data();
    const uint8_t *mp = mask && n ? mask->data() : nullptr;
    const int32_t *kp = key && n ? key->data() : nullptr;
    VoxelClusters out;
    ck(fiesta_hip_cluster_voxels(h_, vp, mp, kp, n, connectivity, min_size, 0, 0, nullptr, &out.info));  // sizes the buffers
    const size_t k = (size_t)out.info.n_clusters;
    out.label.assign((size_t)n + 1, -1);  // (one spare entry in every array: never a null pointer)
    out.size.assign(k + 1, 0), out.root.assign(k + 1, 0), out.mask_or.assign(k + 1, 0), out.key_min.assign(k + 1, 0);
    out.key_argmin.assign(k + 1, 0), out.offsets.assign(k + 1, 0), out.members.assign((size_t)out.info.n_members + 1, 0);
    std::vector<int32_t> lo(3 * k + 1), hi(3 * k + 1);
    std::vector<double> cen(3 * k + 1);
    const fiesta_hip_cluster_result r{out.label.data(), out.size.data(), out.root.data(), lo.data(), hi.data(), cen.data(), out.mask_or.data(),
                                      out.key_min.data(), out.key_argmin.data(), out.offsets.data(), out.members.data()};
    ck(fiesta_hip_cluster_voxels(h_, vp, mp, kp, n, connectivity, min_size, (int64_t)k, out.info.n_members, &r, &out.info));
    out.label.resize((size_t)n), out.size.resize(k), out.root.resize(k), out.mask_or.resize(k), out.key_min.resize(k);
    out.key_argmin.resize(k), out.members.resize((size_t)out.info.n_members);
    for (size_t c = 0; c < k; ++c) {
      out.box_lo.push_back(Eigen::Vector3i(lo[3 * c], lo[3 * c + 1], lo[3 * c + 2]));
      out.box_hi.push_back(Eigen::Vector3i(hi[3 * c], hi[3 * c + 1], hi[3 * c + 2]));
      out.centroid.push_back(Eigen::Vector3d(cen[3 * c], cen[3 * c + 1], cen[3 * c + 2]));
    }
    return out;
  }
  // Cluster splitting (fiesta_hip_split_clusters, include/fiesta_hip.h): every part of a cluster that holds more than max_size members
  // or spans more than max_extent voxels (0: criterion off) is cut at the middle of its box's longest axis, at most max_depth levels
  // deep -- view-sized pieces of a large frontier.  offsets / members: the CSR pair of ClusterVoxels over the same `vox`; the parts
  // come cluster-major, low before high.  Parts need not be connected.
  struct ClusterParts {
    std::vector<int32_t> parent;  // per part from here on: the cluster it was cut from
    std::vector<uint8_t> depth;
    std::vector<int32_t> size;
    std::vector<int64_t> root;
    std::vector<Eigen::Vector3i> box_lo, box_hi;  // inclusive
    std::vector<Eigen::Vector3d> centroid;        // metres
    std::vector<uint8_t> mask_or;
    std::vector<int32_t> key_min;
    std::vector<int64_t> key_argmin;
    std::vector<int64_t> offsets, members;
    std::vector<int32_t> label;  // per entry: the last part that lists it; -1: none
    fiesta_hip_split_info info{};
    size_t count() const { return size.size(); }
  };
  ClusterParts SplitClusters(const std::vector<Eigen::Vector3i> &vox, const std::vector<int64_t> &offsets, const std::vector<int64_t> &members,
                             const std::vector<uint8_t> *mask = nullptr, const std::vector<int32_t> *key = nullptr, int32_t max_size = 0,
                             int32_t max_extent = 0, int32_t max_depth = FIESTA_HIP_SPLIT_MAX_DEPTH) {
    Flush();
    const int64_t n = (int64_t)vox.size(), K = offsets.empty() ? 0 : (int64_t)offsets.size() - 1, M = (int64_t)members.size();
    if ((mask && (int64_t)mask->size() != n) || (key && (int64_t)key->size() != n))
      throw std::invalid_argument("SplitClusters: mask and key need one value per entry");
    std::vector<int32_t> v;
    for (const auto &p : vox) v.insert(v.end(), {p(0), p(1), p(2)});
    const int32_t *vp = v.empty() ? nullptr : v.data();
    const uint8_t *mp = mask && n ? mask->data() : nullptr;
    const int32_t *kp = key && n ? key->data() : nullptr;
    const int64_t *op = K ? offsets.data() : nullptr, *bp = M ? members.data() : nullptr;
    ClusterParts out;
    ck(fiesta_hip_split_clusters(h_, vp, mp, kp, n, op, bp, K, M, max_size, max_extent, max_depth, 0, nullptr, &out.info));  // sizes the buffers
    const size_t k = (size_t)out.info.n_parts;
    out.label.assign((size_t)n + 1, -1);  // (one spare entry in every array: never a null pointer)
    out.parent.assign(k + 1, 0), out.depth.assign(k + 1, 0), out.size.assign(k + 1, 0), out.root.assign(k + 1, 0), out.mask_or.assign(k + 1, 0);
    out.key_min.assign(k + 1, 0), out.key_argmin.assign(k + 1, 0), out.offsets.assign(k + 1, 0), out.members.assign((size_t)M + 1, 0);
    std::vector<int32_t> lo(3 * k + 1), hi(3 * k + 1);
    std::vector<double> cen(3 * k + 1);
    const fiesta_hip_split_result r{out.parent.data(), out.depth.data(),   out.size.data(),       out.root.data(),    lo.data(),          hi.data(),       cen.data(),
                                    out.mask_or.data(), out.key_min.data(), out.key_argmin.data(), out.offsets.data(), out.members.data(), out.label.data()};
    ck(fiesta_hip_split_clusters(h_, vp, mp, kp, n, op, bp, K, M, max_size, max_extent, max_depth, (int64_t)k, &r, &out.info));
    out.label.resize((size_t)n), out.parent.resize(k), out.depth.resize(k), out.size.resize(k), out.root.resize(k), out.mask_or.resize(k);
    out.key_min.resize(k), out.key_argmin.resize(k), out.members.resize((size_t)out.info.n_members);
    for (size_t c = 0; c < k; ++c) {
      out.box_lo.push_back(Eigen::Vector3i(lo[3 * c], lo[3 * c + 1], lo[3 * c + 2]));
      out.box_hi.push_back(Eigen::Vector3i(hi[3 * c], hi[3 * c + 1], hi[3 * c + 2]));
      out.centroid.push_back(Eigen::Vector3d(cen[3 * c], cen[3 * c + 1], cen[3 * c + 2]));
    }
    return out;
  }
  // GetFrontierVoxels and ClusterVoxels composed (both null: the whole map): the frontier voxels, their masks and their clusters
  VoxelClusters GetFrontierClusters(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, double min_clearance, int32_t connectivity,
                                    int32_t min_size, std::vector<Eigen::Vector3i> &vox, std::vector<uint8_t> *mask = nullptr) {
    if ((lo == nullptr) != (hi == nullptr)) throw std::invalid_argument("GetFrontierClusters: lo and hi must both be given or both be null");
    std::vector<uint8_t> own;
    std::vector<uint8_t> &mk = mask ? *mask : own;
    if (lo)
      GetFrontierVoxels(*lo, *hi, min_clearance, vox, &mk);
    else
      GetFrontierVoxels(min_clearance, vox, &mk);
    return ClusterVoxels(vox, &mk, nullptr, connectivity, min_size);
  }
  // View coverage (fiesta_hip_view_coverage, include/fiesta_hip.h): candidate viewpoints against the target voxels of their group --
  // per view how many targets lie in the sensor's range and field of view and how many of those it sees (no voxel of
  // sensor.block_mask before the target), per target how many views see it and the first of them, per group the best view.
  // offsets / members (both nullable): the CSR pair of ClusterVoxels; without them all targets are one group.
  struct ViewPose {
    Eigen::Vector3d pos;  // metres
    double dx, dy;        // the horizontal unit forward vector: cos / sin of the yaw
    int32_t group;
  };
  typedef std::array<double, 5> RingRow;  // ox, oy, oz, dx, dy
  struct ViewCoverageResult {
    std::vector<uint8_t> view_class;            // per view from here on
    std::vector<int32_t> n_in_view, n_visible;  // -1: unusable view
    std::vector<int32_t> cover_count, first_view;  // per target
    std::vector<int64_t> best_view;                // per group; -1: none
    std::vector<int32_t> best_count;
    fiesta_hip_view_info info{};
  };
  static fiesta_hip_view_sensor ViewSensor(double min_range, double max_range, double tan_h, double tan_v, int32_t block_mask = FIESTA_HIP_RAY_OCCUPIED,
                                           bool omni = false, double min_clearance = 0.0, int32_t min_visible = 1) {
    return fiesta_hip_view_sensor{min_range, max_range, tan_h, tan_v, min_clearance, block_mask, omni ? FIESTA_HIP_VIEW_OMNI : 0, min_visible, 0};
  }
  // a ring of view offsets around a centre, looking back at it: per radius, height and angle (r cos phi, r sin phi, h, -cos phi, -sin phi)
  static std::vector<RingRow> ViewRing(const std::vector<double> &radii, int n_angles, const std::vector<double> &heights) {
    std::vector<RingRow> ring;
    for (double r : radii)
      for (double h : heights)
        for (int i = 0; i < n_angles; ++i) {
          const double phi = 2.0 * 3.141592653589793 * i / n_angles, c = std::cos(phi), s = std::sin(phi);
          ring.push_back(RingRow{r * c, r * s, h, -c, -s});
        }
    return ring;
  }
  ViewCoverageResult ViewCoverage(const std::vector<Eigen::Vector3i> &vox, const std::vector<ViewPose> &views, const fiesta_hip_view_sensor &sensor,
                                  const std::vector<int64_t> *offsets = nullptr, const std::vector<int64_t> *members = nullptr) {
    std::vector<double> pos(3 * views.size() + 1), dir(2 * views.size() + 1);  // (one spare entry: never a null pointer)
    std::vector<int32_t> group(views.size() + 1);
    for (size_t i = 0; i < views.size(); ++i) {
      for (int c = 0; c < 3; ++c) pos[3 * i + c] = views[i].pos(c);
      dir[2 * i] = views[i].dx, dir[2 * i + 1] = views[i].dy, group[i] = views[i].group;
    }
    const fiesta_hip_view_set set{pos.data(), dir.data(), group.data(), (int64_t)views.size(), nullptr, nullptr, 0};
    return view_coverage(vox, set, (int64_t)views.size(), sensor, offsets, members);
  }
  // ring form: view k * ring.size() + j stands at centroid[k] + ring[j]'s offset, looks along ring[j]'s direction and belongs to group k
  ViewCoverageResult ViewCoverage(const std::vector<Eigen::Vector3i> &vox, const std::vector<Eigen::Vector3d> &centroid, const std::vector<RingRow> &ring,
                                  const fiesta_hip_view_sensor &sensor, const std::vector<int64_t> *offsets = nullptr,
                                  const std::vector<int64_t> *members = nullptr) {
    if (centroid.size() != (offsets ? offsets->size() - 1 : 1)) throw std::invalid_argument("ViewCoverage: one centroid per group");
    std::vector<double> cen(3 * centroid.size() + 1), rg(5 * ring.size() + 1);
    for (size_t k = 0; k < centroid.size(); ++k)
      for (int c = 0; c < 3; ++c) cen[3 * k + c] = centroid[k](c);
    for (size_t j = 0; j < ring.size(); ++j)
      for (int c = 0; c < 5; ++c) rg[5 * j + c] = ring[j][c];
    const fiesta_hip_view_set set{nullptr, nullptr, nullptr, 0, cen.data(), rg.data(), (int64_t)ring.size()};
    return view_coverage(vox, set, (int64_t)(centroid.size() * ring.size()), sensor, offsets, members);
  }
  // GetFrontierClusters and the ring form of ViewCoverage composed: the clusters of the frontier, and for every cluster the best of
  // the ring's poses around its centroid against its own members (best_pos / best_dx / best_dy; coverage.best_view -1: none)
  struct FrontierViewSet {
    VoxelClusters clusters;
    ViewCoverageResult coverage;
    std::vector<Eigen::Vector3d> best_pos;
    std::vector<double> best_dx, best_dy;
  };
  FrontierViewSet GetFrontierViews(const Eigen::Vector3i *lo, const Eigen::Vector3i *hi, double min_clearance, int32_t connectivity, int32_t min_size,
                                   const std::vector<RingRow> &ring, const fiesta_hip_view_sensor &sensor, std::vector<Eigen::Vector3i> &vox,
                                   std::vector<uint8_t> *mask = nullptr) {
    FrontierViewSet out;
    out.clusters = GetFrontierClusters(lo, hi, min_clearance, connectivity, min_size, vox, mask);
    out.coverage = ViewCoverage(vox, out.clusters.centroid, ring, sensor, &out.clusters.offsets, &out.clusters.members);
    for (size_t k = 0; k < out.clusters.count(); ++k) {
      const int64_t b = out.coverage.best_view[k];
      const double nan = std::nan("");
      if (b < 0) {
        out.best_pos.push_back(Eigen::Vector3d(nan, nan, nan)), out.best_dx.push_back(nan), out.best_dy.push_back(nan);
        continue;
      }
      const RingRow &r = ring[(size_t)b % ring.size()];
      const Eigen::Vector3d &c = out.clusters.centroid[k];
      out.best_pos.push_back(Eigen::Vector3d(c(0) + r[0], c(1) + r[1], c(2) + r[2])), out.best_dx.push_back(r[3]), out.best_dy.push_back(r[4]);
    }
    return out;
  }
  // The reference's own getters (include/ESDFMap.h:144-145, src/ESDFMap.cpp:544-699).  The message types are template
  // parameters so that this header builds without ROS; sensor_msgs::PointCloud and visualization_msgs::Marker fit as
  // they are (fields used: header.frame_id, points[i].x/y/z, and for the marker id, type, action, scale, pose.orientation,
  // colors[i].r/g/b/a).  Filtering, Vox2Pos and the rainbow run on the device; the order of the points is unspecified.
  template <class PointCloudMsg>
  void GetPointCloud(PointCloudMsg &m, int vis_lower_bound, int vis_upper_bound) {
    Flush();
    m.header.frame_id = "world";
    m.points.clear();
    int64_t n = 0;
    ck(fiesta_hip_get_point_cloud(h_, vis_lower_bound, vis_upper_bound, nullptr, 0, &n));
    std::vector<float> xyz((size_t)3 * n);
    if (n) ck(fiesta_hip_get_point_cloud(h_, vis_lower_bound, vis_upper_bound, xyz.data(), n, &n));
    m.points.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) m.points[i].x = xyz[3 * i], m.points[i].y = xyz[3 * i + 1], m.points[i].z = xyz[3 * i + 2];
  }
  template <class MarkerMsg, class Color /* Eigen::Vector4d; the reference ignores it too */>
  void GetSliceMarker(MarkerMsg &m, int slice, int id, Color /*color*/, double max_dist) {
    Flush();
    m.header.frame_id = "world";
    m.id = id;
    m.type = MarkerMsg::POINTS;
    m.action = MarkerMsg::MODIFY;
    m.scale.x = m.scale.y = m.scale.z = res_;
    m.pose.orientation.w = 1;
    m.pose.orientation.x = m.pose.orientation.y = m.pose.orientation.z = 0;
    m.points.clear();
    m.colors.clear();
    int64_t n = 0;
    ck(fiesta_hip_get_slice_marker(h_, slice, max_dist, nullptr, nullptr, 0, &n));
    std::vector<double> xyz((size_t)3 * n);
    std::vector<float> rgba((size_t)4 * n);
    if (n) ck(fiesta_hip_get_slice_marker(h_, slice, max_dist, xyz.data(), rgba.data(), n, &n));
    m.points.resize((size_t)n);
    m.colors.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      m.points[i].x = xyz[3 * i], m.points[i].y = xyz[3 * i + 1], m.points[i].z = xyz[3 * i + 2];
      m.colors[i].r = rgba[4 * i], m.colors[i].g = rgba[4 * i + 1], m.colors[i].b = rgba[4 * i + 2], m.colors[i].a = rgba[4 * i + 3];
    }
  }
  // distances of the plane z = z_vox, nx * ny values, x-major (the data behind GetSliceMarker)
  void GetSlice(int z_vox, std::vector<double> *dist) {
    dist->resize((size_t)gs_[0] * gs_[1]);
    ck(fiesta_hip_get_slice(h_, z_vox, dist->data()));
  }

  // DEBUG checkers (src/ESDFMap.cpp:856-1054). The doubly-linked lists they walk do not exist here; the
  // equivalent invariant is: every finite voxel's closest obstacle is occupied and sits at the stored distance.
  bool CheckConsistency() {
    Flush();
    if (hash_) return CheckConsistencyHash();
    const size_t n = (size_t)grid_total_size_;
    std::vector<int32_t> d2(n), coc(3 * n);
    std::vector<uint8_t> occ(n);
    ck(fiesta_hip_download_field(h_, d2.data(), coc.data(), occ.data(), nullptr));
    for (size_t i = 0; i < n; ++i) {
      if (d2[i] < 0 || d2[i] == INT32_MAX) continue;
      const int64_t z = i % gs_[2], y = (i / gs_[2]) % gs_[1], x = i / ((int64_t)gs_[2] * gs_[1]);
      const int64_t cx = coc[3 * i], cy = coc[3 * i + 1], cz = coc[3 * i + 2];
      if (cx < 0 || cy < 0 || cz < 0 || cx >= gs_[0] || cy >= gs_[1] || cz >= gs_[2]) return false;
      if (!occ[(cx * gs_[1] + cy) * gs_[2] + cz]) return false;
      if ((x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz) != d2[i]) return false;
    }
    return true;
  }
  bool CheckWithGroundTruth() { return CheckConsistency(); }

  const fiesta_hip_stats &LastStats() const { return last_stats_; }
  int64_t LastInsertCount() const { return last_insert_; }
  int64_t LastDeleteCount() const { return last_delete_; }
  fiesta_hip_map *Handle() { return h_; }

  // Apply the buffered SetOccupancy calls now (called implicitly where the result could be observed).
  void Flush() {
    if (pend_occ_.empty()) return;
    ck(fiesta_hip_set_occupancy_vox(h_, pend_vox_.data(), pend_occ_.data(), (int64_t)pend_occ_.size(), nullptr));
    pend_vox_.clear();
    pend_occ_.clear();
  }

  int grid_total_size_ = 0;  // public in the reference's array build (include/ESDFMap.h:115)

 private:
  static constexpr size_t kFlushAt = 1u << 20;
  void FrontierVoxels(const int32_t *lo, const int32_t *hi, double min_clearance, std::vector<Eigen::Vector3i> &out,
                      std::vector<uint8_t> *mask) {
    Flush();
    int64_t n = 0;
    ck(fiesta_hip_get_frontier_voxels(h_, lo, hi, min_clearance, nullptr, nullptr, 0, &n));
    std::vector<int32_t> vox((size_t)3 * n);
    if (mask) mask->assign((size_t)n, 0);
    if (n) ck(fiesta_hip_get_frontier_voxels(h_, lo, hi, min_clearance, vox.data(), mask ? mask->data() : nullptr, n, &n));
    out.clear();
    for (int64_t i = 0; i < n; ++i) out.push_back(Eigen::Vector3i(vox[3 * i], vox[3 * i + 1], vox[3 * i + 2]));
  }
  fiesta_hip_map *h_ = nullptr;
  bool hash_ = false;
  double origin_[3], res_ = 0, min_range_[3], max_range_[3];
  int32_t gs_[3] = {0, 0, 0};
  int64_t last_insert_ = 0, last_delete_ = 0;
  fiesta_hip_stats last_stats_{};
  std::vector<int32_t> pend_vox_, pend_occ_;

  fiesta_hip_config make_config(const Eigen::Vector3d &origin, double resolution, int device) {
    fiesta_hip_config c{};
    c.device = device;
    c.resolution = resolution;
    res_ = resolution;
    for (int i = 0; i < 3; ++i) c.origin[i] = origin_[i] = origin(i);
    return c;
  }
  void open(const fiesta_hip_config &c) {
    if (fiesta_hip_create(&c, &h_) != FIESTA_HIP_OK)
      throw std::runtime_error(std::string("fiesta::ESDFMap: ") + fiesta_hip_last_error());
    int64_t n = 0;
    ck(fiesta_hip_grid_size(h_, gs_));
    ck(fiesta_hip_grid_total_size(h_, &n));
    grid_total_size_ = (int)n;
  }

  ViewCoverageResult view_coverage(const std::vector<Eigen::Vector3i> &vox, const fiesta_hip_view_set &set, int64_t n_views,
                                   const fiesta_hip_view_sensor &sensor, const std::vector<int64_t> *offsets, const std::vector<int64_t> *members) {
    Flush();
    if (offsets && offsets->empty()) throw std::invalid_argument("ViewCoverage: offsets needs n_groups + 1 entries");
    const int64_t n = (int64_t)vox.size(), groups = offsets ? (int64_t)offsets->size() - 1 : 1;
    std::vector<int32_t> v;
    for (const auto &p : vox) v.insert(v.end(), {p(0), p(1), p(2)});
    ViewCoverageResult out;
    out.view_class.assign((size_t)n_views + 1, 0), out.n_in_view.assign((size_t)n_views + 1, 0), out.n_visible.assign((size_t)n_views + 1, 0);
    out.cover_count.assign((size_t)n + 1, 0), out.first_view.assign((size_t)n + 1, 0);
    out.best_view.assign((size_t)groups + 1, 0), out.best_count.assign((size_t)groups + 1, 0);
    const fiesta_hip_view_result r{out.view_class.data(), out.n_in_view.data(), out.n_visible.data(), out.cover_count.data(), out.first_view.data(),
                                   out.best_view.data(), out.best_count.data()};
    const int64_t none = 0;  // (an empty member list is still a member list: never a null pointer)
    ck(fiesta_hip_view_coverage(h_, v.empty() ? nullptr : v.data(), n, offsets ? offsets->data() : nullptr,
                                members ? (members->empty() ? &none : members->data()) : nullptr, groups, members ? (int64_t)members->size() : 0, &set, &sensor,
                                &r, &out.info));
    out.view_class.resize((size_t)n_views), out.n_in_view.resize((size_t)n_views), out.n_visible.resize((size_t)n_views);
    out.cover_count.resize((size_t)n), out.first_view.resize((size_t)n), out.best_view.resize((size_t)groups), out.best_count.resize((size_t)groups);
    return out;
  }
  static void ck(int status) {
    if (status != FIESTA_HIP_OK) throw std::runtime_error(std::string("fiesta::ESDFMap: ") + fiesta_hip_last_error());
  }
  bool PosInMap(const Eigen::Vector3d &p) const {  // src/ESDFMap.cpp:46-61
    for (int i = 0; i < 3; ++i)
      if (p(i) < min_range_[i] || p(i) > max_range_[i]) return false;
    return true;
  }
  void Pos2Vox(const Eigen::Vector3d &p, Eigen::Vector3i &v) const {  // :74-77
    for (int i = 0; i < 3; ++i) v(i) = (int)std::floor((p(i) - origin_[i]) / res_);
  }
  int Vox2Idx(const Eigen::Vector3i &v) const {  // :84-93; hash flavour: see fiesta_hip_voxel_key
    if (!hash_) return v(0) * gs_[1] * gs_[2] + v(1) * gs_[2] + v(2);
    const int32_t vox[3] = {v(0), v(1), v(2)};
    int32_t key = FIESTA_HIP_UNDEFINED;
    ck(fiesta_hip_voxel_key(h_, vox, 1, &key));
    return key;
  }
  bool CheckConsistencyHash() {  // the same invariant over the allocated voxels of a hash-block map
    int64_t n = 0;
    ck(fiesta_hip_download_hash(h_, &n, nullptr, nullptr, nullptr, nullptr));
    std::vector<int32_t> vox(3 * (size_t)n), d2((size_t)n), coc(3 * (size_t)n);
    std::vector<uint8_t> occ((size_t)n);
    if (n) ck(fiesta_hip_download_hash(h_, &n, vox.data(), d2.data(), coc.data(), occ.data()));
    auto key = [](int64_t x, int64_t y, int64_t z) { return ((x + (1 << 20)) << 42) | ((y + (1 << 20)) << 21) | (z + (1 << 20)); };
    std::vector<int64_t> occupied;
    for (int64_t i = 0; i < n; ++i)
      if (occ[i]) occupied.push_back(key(vox[3 * i], vox[3 * i + 1], vox[3 * i + 2]));
    std::sort(occupied.begin(), occupied.end());
    for (int64_t i = 0; i < n; ++i) {
      if (d2[i] < 0 || d2[i] == INT32_MAX) continue;
      const int64_t dx = vox[3 * i] - coc[3 * i], dy = vox[3 * i + 1] - coc[3 * i + 1], dz = vox[3 * i + 2] - coc[3 * i + 2];
      if (dx * dx + dy * dy + dz * dz != d2[i]) return false;
      if (!std::binary_search(occupied.begin(), occupied.end(), key(coc[3 * i], coc[3 * i + 1], coc[3 * i + 2]))) return false;
    }
    return true;
  }
};

// Raycast(start, end, min, max, &output) (include/raycast.h:16-18, src/raycast.cpp:56-158); voxel units.
inline void Raycast(const Eigen::Vector3d &start, const Eigen::Vector3d &end, const Eigen::Vector3d &min,
                    const Eigen::Vector3d &max, std::vector<Eigen::Vector3d> *output, int device = 0) {
  const double a[3] = {start(0), start(1), start(2)}, b[3] = {end(0), end(1), end(2)};
  const double lo[3] = {min(0), min(1), min(2)}, hi[3] = {max(0), max(1), max(2)};
  std::vector<double> buf(3 * 1502);
  int32_t n = 0;
  if (fiesta_hip_raycast_single(a, b, lo, hi, buf.data(), 1502, &n, device) != FIESTA_HIP_OK)
    throw std::out_of_range("Too many RaycasMultithread voxels");  // src/raycast.cpp:127-130
  output->clear();
  for (int i = 0; i < n; ++i) output->push_back(Eigen::Vector3d(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]));
}


// One sensor frame for a -DSIGNED_NEEDED pair (include/Fiesta.h:39-41, 216-218, 249-251, 515-518): what
// Fiesta::RaycastMultithread does to esdf_map_ and inv_esdf_map_ -- the inverse map sees the end points as free and the
// crossed voxels as occupied.  points: n x 3 floats in the sensor frame, transform row-major 4x4.  Both maps must have
// the same geometry; the caller then runs UpdateOccupancy / UpdateESDF on both (:507-518).
inline void RaycastFrameSigned(ESDFMap &esdf_map, ESDFMap &inv_esdf_map, const float *points, int64_t n,
                               const double transform[16], const Eigen::Vector3d &raycast_origin, double min_ray_length,
                               double max_ray_length, const Eigen::Vector3d &l_cornor, const Eigen::Vector3d &r_cornor) {
  const double o[3] = {raycast_origin(0), raycast_origin(1), raycast_origin(2)};
  esdf_map.Flush();  // buffered SetOccupancy calls come BEFORE the frame, as they would in the reference
  inv_esdf_map.Flush();
  fiesta_hip_raycast_params p{min_ray_length, max_ray_length, {l_cornor(0), l_cornor(1), l_cornor(2)},
                              {r_cornor(0), r_cornor(1), r_cornor(2)}, /*dedup=*/1, /*inverse=*/0};
  if (fiesta_hip_raycast_frame(esdf_map.Handle(), points, n, transform, o, &p) != FIESTA_HIP_OK)
    throw std::runtime_error(fiesta_hip_last_error());
  p.inverse = 1;
  if (fiesta_hip_raycast_frame(inv_esdf_map.Handle(), points, n, transform, o, &p) != FIESTA_HIP_OK)
    throw std::runtime_error(fiesta_hip_last_error());
}
// ... and the quantity the pair exists for (the reference leaves it as a TODO): distance to the nearest obstacle minus
// distance to the nearest voxel observed free -- positive in free space, negative inside obstacles.
// NaN where either map holds no distance there (-10000 outside the map / +10000 unobserved or no obstacle), like the
// Python helper fiesta_amd.signed_distance.
inline double SignedDistance(ESDFMap &esdf_map, ESDFMap &inv_esdf_map, const Eigen::Vector3d &pos) {
  const double d = esdf_map.GetDistance(pos), di = inv_esdf_map.GetDistance(pos);
  if (!(std::fabs(d) < 10000.0) || !(std::fabs(di) < 10000.0)) return std::nan("");
  return d - di;
}

}  // namespace fiesta
