// Host-side C++ mirror of the reference's corridor generator on top of the C-ABI (include/direct_cluster.h).
//
// The reference class is `polyhedronGenerator` (global_planner/include/global_planner/utils/poly_utils.h:27-118,
// global_planner/src/utils/poly_utils.cpp): paramSet -> map -> corridorGeneration(gridPath) walks a grid path and
// asks getConvexPoly(seed) for a new polytope whenever the path leaves the latest one (:508-557).  This header keeps
// those names and that walk (coord2Index / index2Coord :3-40, isOutsidePolytope with its 0.01 margin :42-52, the pop of
// the last polytope when the path re-enters the last but one :526-530) and replaces what getConvexPoly, Polyhedron::hrep
// and polyHrep2Utils do per seed (:127-206, 282-389: voxel clustering, quickhull, cdd) by ONE device call for all the
// seeds that are due:
//   * corridorGeneration(gridPath, corridor)       the reference's single-path walk (one seed per device call)
//   * corridorInsertGeneration(coordSet, corridor) the walk the LIVE caller uses (teach_repeat_planner.cpp:172, 228;
//     poly_utils.cpp:391-449): continues the corridor it is given (isOutsideLatestPolytope against the last existing
//     polytope), never pops, works on a copy and returns 0 / 1 - on 0 (no map, cdd error) the corridor is untouched
//   * corridorGenerationBatch(gridPaths, corridors) many paths in lock step: every round collects the seed each
//     unfinished walk is waiting for and runs them as one batch - the form the device wants.  A walk's result does not
//     depend on the other walks (getConvexPoly is a function of the seed voxel and the map), so both give the same
//     corridors.
//   * cubeCorridorBatch(gridPaths, corridors, pop_back) the corridors of is_cluster_on == false (every polytope the inflated
//     cube of its seed voxel) for many paths in ONE device call, direct_cluster_cube_corridor_batch: no rounds at all
//   * cubeCorridorClearBatch(gridPaths, corridors, min_d2, pop_back) the same on the resident distance field: cubes stop at voxels
//     closer to an obstacle than the floor (direct_cluster_cube_corridor_clear_batch)
//   * clusterCorridorBatch(gridPaths, corridors, pop_back) the corridors of corridorGenerationBatch / corridorInsertGenerationBatch
//     from empty corridors with the walk itself on the device (direct_cluster_corridor_batch): due seeds de-duplicated per round,
//     no plane read back between rounds
//   * buildFreeComponents(min_d2) / reachable(starts, goals) which goals can be reached at all, before any path call runs
//     (direct_cluster_free_components, direct_cluster_reachable_batch)
//   * integrateScan(..., track_known) / frontiers(min_size, min_d2, capacity) where the goals of a vehicle that maps as it flies
//     come from: the boundary between what its scans have observed and what they have not (direct_cluster_frontier)
//   * viewGain(voxels, dirs, n_sets, range_vox, sets) which of those goals is worth flying to: the unknown voxels an ideal sensor
//     would see from each of them (direct_cluster_view_gain_batch)
// Corridor / Polytope types are template parameters read through the member names of
// global_planner/include/global_planner/utils/data_type.h:124-245 (polyhedrons, planes, center, seed_coord,
// appendPlane, setSeed / setCenter where they exist); direct::PlainCorridor of ddp_optimizer.hpp fits.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/direct_cluster.h"
#include "ddp_optimizer.hpp"

namespace direct {

class polyhedronGenerator {
 public:
  // paramSet (poly_utils.h:60-85): resolution, map origin and size in voxels, clustering limits; max_batch seeds per device call
  polyhedronGenerator(double resolution, const std::array<double, 3>& map_lower, int max_x_id, int max_y_id, int max_z_id,
                      int itr_inflate_max = 1000, int itr_cluster_max = 50, int max_batch = 64, int cluster_capacity = 50000,
                      int candidate_capacity = 10000, int device = 0)
      : res_(resolution), inv_res_(1.0 / resolution), lower_(map_lower), mx_(max_x_id), my_(max_y_id), mz_(max_z_id),
        itr_inflate_(itr_inflate_max), itr_cluster_(itr_cluster_max), max_batch_(max_batch) {
    direct_cluster_config_t cfg{device, max_x_id, max_y_id, max_z_id, max_batch, cluster_capacity, candidate_capacity, 0};
    if (direct_cluster_create(&cfg, &h_) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
  }
  ~polyhedronGenerator() { direct_cluster_destroy(h_); }
  polyhedronGenerator(const polyhedronGenerator&) = delete;
  polyhedronGenerator& operator=(const polyhedronGenerator&) = delete;

  // the occupancy grid, [x][y][z], 0 free / 1 obstacle (what setObs / mapUpload build, cluster_server_cpu.cpp:83-120)
  void setMap(const uint8_t* map_data) {
    if (direct_cluster_set_map(h_, DIRECT_MEM_HOST, map_data) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    has_map_ = true;
  }
  // the same grid from the sensor's points, built on the device: what rcvPointCloudCallBack does for this class
  // (teach_repeat_planner.cpp:523-581: every point shifted by the box of voxel steps of cloud_margin, setObs(coord2gridIndex(...)),
  // i.e. the CLAMPING border convention).  xyz[n][stride] host floats, stride 3 or 4 (a pcl::PointXYZ buffer); add = false is
  // mapClear first.  Returns the number of occupied voxels.
  int64_t setCloud(const float* xyz, int64_t n, int stride, double cloud_margin, bool add = false) {
    direct_map_cloud_t p{};
    for (int a = 0; a < 3; a++) {
      p.map_lower[a] = lower_[a];
      p.map_upper[a] = lower_[a] + (a == 0 ? mx_ : (a == 1 ? my_ : mz_)) * res_;
    }
    p.resolution = res_;
    p.cloud_margin = cloud_margin;
    p.border = DIRECT_MAP_BORDER_CLAMP;
    p.mode = add ? DIRECT_MAP_ADD : DIRECT_MAP_REPLACE;
    p.stride = stride;
    int64_t stats[4];
    if (direct_cluster_map_from_cloud(h_, &p, n, DIRECT_MEM_HOST, xyz, stats) != DIRECT_OK)
      throw std::runtime_error(direct_cluster_last_error());
    has_map_ = true;
    return stats[3];
  }

  // One sensor scan folded into the map the generator holds (direct_cluster_map_integrate_scan): every ray from origin to a point
  // carves the scan grid free, every return within max_range marks its voxel, and the map is the scan grid dilated by the voxel
  // box inflate (zeros for the radius-aware calls; the radius in voxels for the corridors, which have no floor).  mode:
  // DIRECT_SCAN_RESET, DIRECT_SCAN_CONTINUE, or DIRECT_SCAN_ADOPT after setMap / setCloud.  Unlike setCloud(add = true) a voxel
  // that a later ray passes leaves the map again.  changed() == false: the distance field and the free components still serve.
  // track_known: the scan also records every voxel it carves or marks in the resident known grid, which frontiers() reads; an
  // untracked scan drops a known grid the generator holds.
  struct ScanResult {
    long long points = 0, skipped_nonfinite = 0, truncated = 0, outside = 0, raw_occupied = 0, occupied = 0, set = 0, cleared = 0;
    bool changed() const { return set + cleared > 0; }
  };
  ScanResult integrateScan(const float* xyz, int64_t n, int stride, const std::array<double, 3>& origin, double max_range,
                           const std::array<int, 3>& inflate = {{0, 0, 0}}, int mode = DIRECT_SCAN_CONTINUE, bool track_known = false) {
    direct_map_scan_t p{};
    for (int a = 0; a < 3; a++) {
      p.map_lower[a] = lower_[a];
      p.map_upper[a] = lower_[a] + (a == 0 ? mx_ : (a == 1 ? my_ : mz_)) * res_;
      p.origin[a] = origin[a];
      p.inflate[a] = inflate[a];
    }
    p.resolution = res_;
    p.max_range = max_range;
    p.mode = mode;
    p.stride = stride;
    p.flags = track_known ? DIRECT_SCAN_TRACK_KNOWN : 0;
    int64_t s[8];
    if (direct_cluster_map_integrate_scan(h_, &p, n, DIRECT_MEM_HOST, xyz, s) != DIRECT_OK)
      throw std::runtime_error(direct_cluster_last_error());
    has_map_ = true;
    ScanResult r;
    r.points = s[0]; r.skipped_nonfinite = s[1]; r.truncated = s[2]; r.outside = s[3];
    r.raw_occupied = s[4]; r.occupied = s[5]; r.set = s[6]; r.cleared = s[7];
    return r;
  }
  // One sensor scan folded into the resident EVIDENCE grid (direct_cluster_map_integrate_scan_evidence), for a sensor that is
  // sometimes wrong: every voxel a ray passes loses `miss`, every voxel a return lies in gains `hit` (a return beats a pass), once
  // per voxel and scan, clamped to [ev_min, ev_max]; the scan grid is (evidence >= occ) and the map is the scan grid dilated by
  // inflate.  The defaults are OctoMap's 0.85 / -0.4 / [-2, 3.5] / 0 log-odds in units of 0.05.  mode as in integrateScan (ADOPT:
  // ev_max where the map is occupied).  n == 0 with DIRECT_SCAN_CONTINUE re-thresholds the evidence as it stands.  A plain
  // integrateScan drops the evidence grid; setMap and setCloud keep it.
  struct EvidenceParams {
    int hit, miss, ev_min, ev_max, occ;
    EvidenceParams() : hit(17), miss(8), ev_min(-40), ev_max(70), occ(1) {}
  };
  struct EvidenceResult : ScanResult {
    long long touched_hit = 0, touched_pass = 0, positive = 0, negative = 0;
  };
  EvidenceResult integrateScanEvidence(const float* xyz, int64_t n, int stride, const std::array<double, 3>& origin, double max_range,
                                       const EvidenceParams& ev = EvidenceParams(), const std::array<int, 3>& inflate = {{0, 0, 0}},
                                       int mode = DIRECT_SCAN_CONTINUE, bool track_known = false) {
    direct_map_evidence_t p{};
    for (int a = 0; a < 3; a++) {
      p.scan.map_lower[a] = lower_[a];
      p.scan.map_upper[a] = lower_[a] + (a == 0 ? mx_ : (a == 1 ? my_ : mz_)) * res_;
      p.scan.origin[a] = origin[a];
      p.scan.inflate[a] = inflate[a];
    }
    p.scan.resolution = res_;
    p.scan.max_range = max_range;
    p.scan.mode = mode;
    p.scan.stride = stride;
    p.scan.flags = track_known ? DIRECT_SCAN_TRACK_KNOWN : 0;
    p.hit = ev.hit; p.miss = ev.miss; p.ev_min = ev.ev_min; p.ev_max = ev.ev_max; p.occ = ev.occ;
    int64_t s[12];
    if (direct_cluster_map_integrate_scan_evidence(h_, &p, n, DIRECT_MEM_HOST, xyz, s) != DIRECT_OK)
      throw std::runtime_error(direct_cluster_last_error());
    has_map_ = true;
    EvidenceResult r;
    r.points = s[0]; r.skipped_nonfinite = s[1]; r.truncated = s[2]; r.outside = s[3];
    r.raw_occupied = s[4]; r.occupied = s[5]; r.set = s[6]; r.cleared = s[7];
    r.touched_hit = s[8]; r.touched_pass = s[9]; r.positive = s[10]; r.negative = s[11];
    return r;
  }
  // the evidence grid as the generator holds it, [x][y][z] (direct_cluster_get_evidence); setEvidence(nullptr) empties it.  Map
  // and scan grid follow at the next integrateScanEvidence.
  std::vector<int8_t> evidence() {
    std::vector<int8_t> m((size_t)mx_ * my_ * mz_);
    if (direct_cluster_get_evidence(h_, DIRECT_MEM_HOST, m.data()) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    return m;
  }
  void setEvidence(const int8_t* ev) {
    if (direct_cluster_set_evidence(h_, DIRECT_MEM_HOST, ev) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
  }
  // Goal voxels on the boundary between observed and unobserved space (direct_cluster_frontier): the 26-connected components of
  // the known, enterable voxels with an unknown face neighbour inside the map; those of at least min_size voxels in ascending
  // label order, the first `capacity` of them.  rep[k] is a member of component k - known, enterable under the floor min_d2 - and
  // goes straight into reachable() and the path calls as a voxel index.  kept > capacity: call again with more room.
  struct Frontiers {
    std::vector<int32_t> label, size;                      // [written]
    std::vector<std::array<int32_t, 3>> centroid, rep;     // [written]
    long long known = 0, frontier = 0, components = 0, kept = 0, written = 0, largest = 0;
  };
  Frontiers frontiers(int min_size = 1, int min_d2 = 0, int capacity = 1024) {
    Frontiers f;
    const size_t cap = capacity > 0 ? (size_t)capacity : 0;
    f.label.resize(cap); f.size.resize(cap); f.centroid.resize(cap); f.rep.resize(cap);
    const direct_frontier_in_t in{min_d2, min_size, capacity, DIRECT_MEM_HOST};
    int64_t s[6];
    const direct_frontier_out_t out{cap ? f.label.data() : nullptr, cap ? f.size.data() : nullptr, cap ? &f.centroid[0][0] : nullptr,
                                    cap ? &f.rep[0][0] : nullptr, nullptr, s};
    if (direct_cluster_frontier(h_, &in, &out) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    f.known = s[0]; f.frontier = s[1]; f.components = s[2]; f.kept = s[3]; f.written = s[4]; f.largest = s[5];
    f.label.resize((size_t)s[4]); f.size.resize((size_t)s[4]); f.centroid.resize((size_t)s[4]); f.rep.resize((size_t)s[4]);
    return f;
  }
  // How much unknown space an ideal sensor would see from each candidate voxel (direct_cluster_view_gain_batch): the rays of a
  // direction set are walked from the centre of the voxel through the map the generator holds, range_vox voxels far at most, until
  // they hit an occupied voxel or leave the map.  dirs holds n_sets sets of dirs.size() / n_sets directions each (map frame, any
  // length); sets[c] says which one candidate c uses (nullptr: set 0).  gain[c]: distinct visited voxels the known grid does not
  // hold; seen[c]: distinct visited voxels; ends[c]: rays blocked, left, out of range, skipped; code[c]: DIRECT_VIEW_*.
  struct ViewGain {
    std::vector<int32_t> code, gain, seen;     // [n]
    std::vector<std::array<int32_t, 4>> ends;  // [n]
  };
  ViewGain viewGain(const std::vector<std::array<int32_t, 3>>& voxels, const std::vector<std::array<float, 3>>& dirs, int n_sets,
                    double range_vox, const std::vector<int32_t>* sets = nullptr) {
    if (n_sets < 1 || dirs.size() % (size_t)n_sets != 0) throw std::runtime_error("viewGain: dirs must hold n_sets sets of one size");
    if (sets && sets->size() != voxels.size()) throw std::runtime_error("viewGain: one set index per voxel");
    const size_t n = voxels.size();
    ViewGain r;
    r.code.resize(n); r.gain.resize(n); r.seen.resize(n); r.ends.resize(n);
    const direct_view_gain_in_t in{range_vox, (int32_t)n, (int32_t)(dirs.size() / (size_t)n_sets), n_sets, DIRECT_MEM_HOST, DIRECT_MEM_HOST};
    const direct_view_gain_io_t io{n ? &voxels[0][0] : nullptr, sets && n ? sets->data() : nullptr, dirs.empty() ? nullptr : &dirs[0][0],
                                   n ? r.code.data() : nullptr, n ? r.gain.data() : nullptr, n ? r.seen.data() : nullptr,
                                   n ? &r.ends[0][0] : nullptr};
    if (direct_cluster_view_gain_batch(h_, &in, &io) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    return r;
  }
  // the known grid as the generator holds it, [x][y][z] (direct_cluster_get_known); setKnown(nullptr) empties it
  std::vector<uint8_t> getKnown() {
    std::vector<uint8_t> m((size_t)mx_ * my_ * mz_);
    if (direct_cluster_get_known(h_, DIRECT_MEM_HOST, m.data()) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    return m;
  }
  void setKnown(const uint8_t* known) {
    if (direct_cluster_set_known(h_, DIRECT_MEM_HOST, known) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
  }
  // What the scans make of voxels nobody has observed (direct_cluster_set_unknown_policy): DIRECT_UNKNOWN_FREE (the default: their
  // map byte is 0) or DIRECT_UNKNOWN_OCCUPIED - every integrateScan / integrateScanEvidence, which must then be tracked, keeps
  // two grids: the open map (what it derives under FREE) and the map, the open map with every unobserved voxel closed.  The
  // planning calls read the map, viewGain the open map, frontiers gives the same goals on both.  Takes effect at the next scan.
  void setUnknownPolicy(int policy) {
    if (direct_cluster_set_unknown_policy(h_, policy) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
  }
  struct UnknownPolicy {
    int policy = DIRECT_UNKNOWN_FREE;
    long long closed = 0, open_ones = 0;   // of the last successful scan under OCCUPIED: map 1 and open 0; the open map's ones
  };
  UnknownPolicy unknownPolicy() {
    int32_t p = 0;
    int64_t s[2] = {0, 0};
    if (direct_cluster_get_unknown_policy(h_, &p, s) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    UnknownPolicy r;
    r.policy = p; r.closed = s[0]; r.open_ones = s[1];
    return r;
  }
  // the open map as the generator holds it, [x][y][z] (direct_cluster_get_open_map); throws unless the last writer of the map was
  // a successful scan under DIRECT_UNKNOWN_OCCUPIED
  std::vector<uint8_t> openMap() {
    std::vector<uint8_t> m((size_t)mx_ * my_ * mz_);
    if (direct_cluster_get_open_map(h_, DIRECT_MEM_HOST, m.data()) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    return m;
  }
  // the map as the generator holds it, [x][y][z] (direct_cluster_get_map)
  std::vector<uint8_t> getMap() {
    std::vector<uint8_t> m((size_t)mx_ * my_ * mz_);
    if (direct_cluster_get_map(h_, DIRECT_MEM_HOST, m.data()) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    return m;
  }

  // One plan against the map the generator holds NOW (direct_cluster_plan_check_batch): polyCoeff(k, q) and time(k) as
  // getPolyCoeff() / getPolyTime() give them (Eigen matrices or anything with the same call operators and time.size()).  Conservative:
  // a blocked verdict means that a piece of the curve of duration T_i / 2^depth has a bounding box touching an occupied voxel, not
  // that the curve enters it.  t_from < 0 judges the whole plan.
  struct PlanCheck {
    int verdict = DIRECT_PLAN_CHECK_INVALID;   // 0 clear; 1 occupied, 2 leaves the map, 3 both: the first blocked piece
    double t_free = 0;                         // certified clear before this time on the plan's clock (t_total when clear)
    int segment = -1, leaf = -1;               // the first blocked piece
    int box[6] = {-1, -1, -1, -1, -1, -1};     // its voxel-index box, lo xyz, hi xyz
    bool clear() const { return verdict == 0; }
  };
  template <class Mat, class Vec>
  PlanCheck checkTrajectory(const Mat& polyCoeff, const Vec& time, int depth = 8, double margin = 0.0, double t_from = -1.0,
                            bool outside_blocks = false) {
    const int N = (int)time.size();
    std::vector<double> poly((size_t)N * 18), T(N);
    for (int k = 0; k < N; k++) {
      T[k] = time(k);
      for (int q = 0; q < 18; q++) poly[(size_t)k * 18 + q] = polyCoeff(k, q);
    }
    int32_t n_seg = N, status = 0, verdict = 0, first[2] = {-1, -1};
    PlanCheck c;
    direct_plan_check_in_t in{};
    in.batch = 1; in.n_seg_max = N; in.mem = DIRECT_MEM_HOST; in.dtype = DIRECT_F64;
    in.n_seg = &n_seg; in.T = T.data(); in.poly = poly.data();
    for (int a = 0; a < 3; a++) in.map_lower[a] = lower_[a];
    in.resolution = res_; in.margin = margin; in.depth = depth; in.outside_blocks = outside_blocks ? 1 : 0;
    in.t_from = t_from < 0.0 ? nullptr : &t_from;
    direct_plan_check_out_t out{};
    out.status = &status; out.verdict = &verdict; out.t_free = &c.t_free; out.first = first; out.hit_box = c.box;
    if (direct_cluster_plan_check_batch(h_, &in, &out) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    c.verdict = verdict; c.segment = first[0]; c.leaf = first[1];
    return c;
  }

  // The exact squared Euclidean distance field of the map the generator holds NOW (direct_cluster_distance_field), resident
  // until the map changes: call it after every map update and before trajectoryClearance.  cap_vox > 0 stores min(D2, cap_vox^2).
  // -> the number of voxels with a stored value below the cap
  long long buildDistanceField(int cap_vox = 0) {
    int64_t stats[2] = {0, -1};
    if (direct_cluster_distance_field(h_, cap_vox, stats) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    return (long long)stats[0];
  }

  // The 26-connected components of the enterable voxels of the map the generator holds NOW (direct_cluster_free_components):
  // byte 0 and, for min_d2 > 1, stored D2 >= min_d2 (buildDistanceField after the last change of the map).  Resident until the
  // map - with a floor also the field - changes: call it before reachable.
  struct FreeComponents {
    long long enterable = 0, components = 0, largest = 0, largest_label = -1;
  };
  FreeComponents buildFreeComponents(int min_d2 = 0) {
    int64_t stats[4] = {0, 0, 0, -1};
    if (direct_cluster_free_components(h_, min_d2, stats) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    comp_min_d2_ = min_d2;
    FreeComponents c;
    c.enterable = stats[0]; c.components = stats[1]; c.largest = stats[2]; c.largest_label = stats[3];
    return c;
  }
  // Which code the path calls would return for each pair (direct_cluster_reachable_batch), coordinates through coord2Index:
  // DIRECT_GRID_PATH_OK, _NO_PATH or _BAD_ENDPOINT (coord2Index clamps, so the last cannot occur), from the labels of the last
  // buildFreeComponents and with its floor.  goal_size (may be null): the voxel count of each goal's component, 0 for a goal that
  // is not enterable - to drop goals in pockets too small to matter before the path calls run.
  std::vector<int32_t> reachable(const std::vector<std::array<double, 3>>& starts, const std::vector<std::array<double, 3>>& goals,
                                 std::vector<int32_t>* goal_size = nullptr) {
    if (starts.size() != goals.size() || starts.empty()) throw std::runtime_error("reachable: starts and goals must pair up");
    const size_t n = starts.size();
    std::vector<int32_t> s(n * 3), g(n * 3), rtn(n);
    for (size_t i = 0; i < n; i++) {
      const std::array<int, 3> a = coord2Index(starts[i]), b = coord2Index(goals[i]);
      for (int k = 0; k < 3; k++) { s[3 * i + k] = a[k]; g[3 * i + k] = b[k]; }
    }
    if (goal_size) goal_size->assign(n, 0);
    direct_reachable_in_t in{};
    in.n = (int64_t)n; in.mem_in = DIRECT_MEM_HOST; in.min_d2 = comp_min_d2_; in.starts = s.data(); in.goals = g.data();
    direct_reachable_out_t out{};
    out.mem = DIRECT_MEM_HOST; out.rtn = rtn.data(); out.goal_size = goal_size ? goal_size->data() : nullptr;
    if (direct_cluster_reachable_batch(h_, &in, &out) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    return rtn;
  }

  // One plan's certified distance to the occupied voxels (direct_cluster_plan_clearance_batch), arguments as checkTrajectory's.
  // A lower bound from the distance field and the bounding boxes of pieces of duration T_i / 2^depth: a negative value certifies
  // nothing.  radius: the vehicle's, on a map that is NOT inflated.  t_from < 0 judges the whole plan.
  struct PlanClearance {
    int verdict = DIRECT_PLAN_CHECK_INVALID;   // 0: every judged piece keeps `radius`; 1: not
    double clearance = 0;                      // metres, the minimum over the judged pieces (+inf on an empty map)
    double t_min = 0;                          // start time of the piece that attains it
    double t_free = 0;                         // certified to keep `radius` before this time (t_total when the verdict is 0)
    int segment = -1, leaf = -1;               // the piece that attains the minimum
    bool clear() const { return verdict == 0; }
  };
  template <class Mat, class Vec>
  PlanClearance trajectoryClearance(const Mat& polyCoeff, const Vec& time, int depth = 6, double radius = 0.0, double t_from = -1.0) {
    const int N = (int)time.size();
    std::vector<double> poly((size_t)N * 18), T(N);
    for (int k = 0; k < N; k++) {
      T[k] = time(k);
      for (int q = 0; q < 18; q++) poly[(size_t)k * 18 + q] = polyCoeff(k, q);
    }
    int32_t n_seg = N, status = 0, verdict = 0, where[2] = {-1, -1};
    PlanClearance c;
    direct_plan_clear_in_t in{};
    in.batch = 1; in.n_seg_max = N; in.mem = DIRECT_MEM_HOST; in.dtype = DIRECT_F64;
    in.n_seg = &n_seg; in.T = T.data(); in.poly = poly.data();
    for (int a = 0; a < 3; a++) in.map_lower[a] = lower_[a];
    in.resolution = res_; in.radius = radius; in.depth = depth;
    in.t_from = t_from < 0.0 ? nullptr : &t_from;
    direct_plan_clear_out_t out{};
    out.status = &status; out.verdict = &verdict; out.clearance = &c.clearance; out.t_min = &c.t_min; out.t_free = &c.t_free; out.where = where;
    if (direct_cluster_plan_clearance_batch(h_, &in, &out) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    c.verdict = verdict; c.segment = where[0]; c.leaf = where[1];
    return c;
  }

  std::array<int, 3> coord2Index(const std::array<double, 3>& c) const {  // :10-18
    auto f = [&](double v, double lo, int mx) {
      int i = (int)((v - lo) * inv_res_);
      return i < 0 ? 0 : (i > mx - 1 ? mx - 1 : i);
    };
    return {{f(c[0], lower_[0], mx_), f(c[1], lower_[1], my_), f(c[2], lower_[2], mz_)}};
  }
  std::array<double, 3> index2Coord(const std::array<int, 3>& i) const {  // :20-29
    return {{i[0] * res_ + 0.5 * res_ + lower_[0], i[1] * res_ + 0.5 * res_ + lower_[1], i[2] * res_ + 0.5 * res_ + lower_[2]}};
  }
  template <class Polytope>
  static bool isOutsidePolytope(const std::array<double, 3>& c, const Polytope& p) {  // :42-52
    for (const auto& pl : p.planes)
      if (c[0] * elem(pl, 0) + c[1] * elem(pl, 1) + c[2] * elem(pl, 2) + elem(pl, 3) > 0.01) return true;
    return false;
  }

  template <class Corridor>
  static bool isOutsideLatestPolytope(const std::array<double, 3>& c, const Corridor& cor) {  // :59-62
    return isOutsidePolytope(c, cor.polyhedrons.back());
  }
  template <class Corridor>
  static bool isInsideLastSecondPolytope(const std::array<double, 3>& c, const Corridor& cor) {  // :64-70
    const size_t n = cor.polyhedrons.size();
    return n > 1 ? !isOutsidePolytope(c, cor.polyhedrons[n - 2]) : false;
  }

  // corridorInsertGeneration (:391-449), the walk of the live caller (teach_repeat_planner.cpp:172, 228): new polytopes
  // are appended behind the ones `corridor` already holds; a point inside the latest polytope adds nothing; there is no
  // pop.  Returns 1 and replaces `corridor` when the whole path went through, 0 (corridor untouched) without a map or
  // where the reference's cdd call fails (:437-439).  The reference's second argument, the visualisation message, has
  // no counterpart here (RViz is out of scope).
  template <class Corridor>
  int corridorInsertGeneration(const std::vector<std::array<double, 3>>& coordSet, Corridor& corridor) {
    if (!has_map_) return 0;  // :394
    std::vector<Corridor*> cs{&corridor};
    return corridorInsertGenerationBatch(std::vector<std::vector<std::array<double, 3>>>{coordSet}, cs)[0];
  }
  // the same for many (path, corridor) pairs in lock step (one device batch per round of due seeds)
  template <class Corridor>
  std::vector<int> corridorInsertGenerationBatch(const std::vector<std::vector<std::array<double, 3>>>& coordSets,
                                                 const std::vector<Corridor*>& corridors) {
    std::vector<int> rc(coordSets.size(), 0);
    if (!has_map_) return rc;
    std::vector<Corridor> beg;  // beg_corridor (:399-403): the copy the walk extends
    for (Corridor* c : corridors) beg.push_back(*c);
    std::vector<Corridor*> ptr;
    for (Corridor& c : beg) ptr.push_back(&c);
    const std::vector<bool> ok = walk(coordSets, ptr, false);
    for (size_t p = 0; p < coordSets.size(); p++)
      if (ok[p]) {
        *corridors[p] = beg[p];  // :447
        rc[p] = 1;
      }
    return rc;
  }

  // corridorGeneration (:508-557) for one path.  Returns false where the reference prints "corridor generation broke".
  template <class Corridor>
  bool corridorGeneration(const std::vector<std::array<double, 3>>& gridPath, Corridor& corridor) {
    std::vector<Corridor*> cs{&corridor};
    return corridorGenerationBatch(std::vector<std::vector<std::array<double, 3>>>{gridPath}, cs)[0];
  }

  // The same walk for many paths in lock step; corridors[p] is extended like the reference's member `corridor`.
  template <class Corridor>
  std::vector<bool> corridorGenerationBatch(const std::vector<std::vector<std::array<double, 3>>>& gridPaths,
                                            const std::vector<Corridor*>& corridors) {
    if (!has_map_) throw std::runtime_error("polyhedronGenerator: no map");
    return walk(gridPaths, corridors, true);
  }

  // The corridors of is_cluster_on == false - paramSet's (itr_inflate_max, itr_cluster_max) = (1000, 0), every polytope the
  // inflated cube of its seed voxel - for many paths in ONE device call (direct_cluster_cube_corridor_batch) instead of one
  // round trip per polytope of the longest corridor: coordinates go through coord2Index, the call walks every path from an empty
  // corridor, and corridors[p] is filled as walk() fills it (planes, center, seed_coord).  pop_back: corridorGeneration's walk
  // (true) or corridorInsertGeneration's (false).  Returns, per path, whether its corridor was generated; a path that is
  // empty is left without polytopes and reported false.  The generator's itr_cluster_max plays no part.
  template <class Corridor>
  std::vector<bool> cubeCorridorBatch(const std::vector<std::vector<std::array<double, 3>>>& gridPaths,
                                      const std::vector<Corridor*>& corridors, bool pop_back = true) {
    return cubeCorridors(gridPaths, corridors, pop_back, [this](const direct_cube_corridor_in_t* in, direct_cube_corridor_out_t* out) {
      return direct_cluster_cube_corridor_batch(h_, in, out);
    });
  }

  // cubeCorridorBatch on the distance field the generator holds (buildDistanceField after the last change of the map;
  // direct_cluster_cube_corridor_clear_batch): a cube stops at voxels whose stored D2 is below min_d2 (voxel^2, the floor of the
  // clearance-aware path calls), so every voxel of a cube but its seed has D2 >= min_d2.  min_d2 <= 1 is cubeCorridorBatch and
  // needs no field.  Fills corridors[p] the same way; lastTableBuilt() says whether the call built a floor table.
  template <class Corridor>
  std::vector<bool> cubeCorridorClearBatch(const std::vector<std::vector<std::array<double, 3>>>& gridPaths,
                                           const std::vector<Corridor*>& corridors, int32_t min_d2, bool pop_back = true) {
    return cubeCorridors(gridPaths, corridors, pop_back, [this, min_d2](const direct_cube_corridor_in_t* in, direct_cube_corridor_out_t* out) {
      int64_t info[2] = {0, 0};
      const direct_status_t st = direct_cluster_cube_corridor_clear_batch(h_, in, min_d2, out, info);
      table_built_ = st == DIRECT_OK && info[0] == 1;
      return st;
    });
  }
  bool lastTableBuilt() const { return table_built_; }

  // corridorGenerationBatch / corridorInsertGenerationBatch from empty corridors with the WALK ON THE DEVICE
  // (direct_cluster_corridor_batch): the generator's own itr_inflate_max / itr_cluster_max, the due seeds of a round
  // de-duplicated by voxel, no plane read back between rounds.  corridors[p] is filled as walk() fills it (planes, center,
  // seed_coord), bit for bit, also where the walk stops early (the polytopes held so far); the plane capacity is
  // getConvexPolyBatch's 128.  Returns, per path, whether the walk completed; an empty path is left without polytopes and
  // reported false.  lastRounds() / lastPolytopes() / lastUniqueSeeds() describe the call afterwards.
  template <class Corridor>
  std::vector<bool> clusterCorridorBatch(const std::vector<std::vector<std::array<double, 3>>>& gridPaths,
                                         const std::vector<Corridor*>& corridors, bool pop_back = true) {
    if (!has_map_) throw std::runtime_error("polyhedronGenerator: no map");
    const size_t np = gridPaths.size();
    std::vector<bool> ok(np, false);
    if (np == 0) return ok;
    size_t cap = 1;
    for (const auto& p : gridPaths) cap = std::max(cap, p.size());
    std::vector<int32_t> xyz(np * cap * 3, 0), len(np);
    for (size_t p = 0; p < np; p++) {
      len[p] = (int32_t)gridPaths[p].size();
      for (size_t i = 0; i < gridPaths[p].size(); i++) {
        const std::array<int, 3> idx = coord2Index(gridPaths[p][i]);
        for (int a = 0; a < 3; a++) xyz[(p * cap + i) * 3 + a] = idx[a];
      }
    }
    const int pcap = 128;
    direct_cluster_corridor_in_t in{};
    in.batch = (int32_t)np; in.path_capacity = (int32_t)cap; in.mem_in = DIRECT_MEM_HOST;
    in.itr_inflate_max = itr_inflate_; in.itr_cluster_max = itr_cluster_;
    in.path_xyz = xyz.data(); in.path_len = len.data(); in.pop_back = pop_back ? 1 : 0;
    in.seg_capacity = (int32_t)cap;  // a corridor has at most one polytope per path point: no row can overflow
    in.p_max = pcap; in.plane_dtype = DIRECT_F64; in.resolution = res_;
    for (int a = 0; a < 3; a++) in.map_lower[a] = lower_[a];
    const size_t segs = np * cap;
    std::vector<int32_t> n_seg(np), n_planes(segs), rtn(np);
    std::vector<double> planes(segs * pcap * 4), seeds(segs * 3), centers(segs * 3);
    direct_cluster_corridor_out_t out{};
    out.mem = DIRECT_MEM_HOST; out.n_seg = n_seg.data(); out.n_planes = n_planes.data(); out.planes = planes.data();
    out.seeds = seeds.data(); out.centers = centers.data(); out.rtn = rtn.data();
    int64_t stats[4] = {0, 0, 0, 0};
    if (direct_cluster_corridor_batch(h_, &in, &out, stats) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    rounds_ = (int)stats[0];
    polytopes_ = (int)stats[1];
    unique_seeds_ = (int)stats[2];
    for (size_t p = 0; p < np; p++) {
      ok[p] = rtn[p] == DIRECT_CORRIDOR_OK;
      Corridor& cor = *corridors[p];
      for (int k = 0; k < n_seg[p]; k++) {
        const size_t at = p * cap + (size_t)k;
        typename std::decay<decltype(cor.polyhedrons[0])>::type pt{};
        for (int j = 0; j < n_planes[at]; j++) {
          const double* pl = &planes[(at * pcap + j) * 4];
          pt.appendPlane({pl[0], pl[1], pl[2], pl[3]});
        }
        for (int a = 0; a < 3; a++) {
          set_elem(pt.center, a, centers[at * 3 + a]);
          set_elem(pt.seed_coord, a, seeds[at * 3 + a]);
        }
        cor.polyhedrons.push_back(pt);
      }
    }
    return ok;
  }
  int lastUniqueSeeds() const { return unique_seeds_; }  // seeds the last clusterCorridorBatch generated (lastPolytopes(): those due)

 private:
  // The two cube corridor calls: call(in, out) is the device call.
  template <class Corridor, class Call>
  std::vector<bool> cubeCorridors(const std::vector<std::vector<std::array<double, 3>>>& gridPaths, const std::vector<Corridor*>& corridors,
                                  bool pop_back, Call call) {
    if (!has_map_) throw std::runtime_error("polyhedronGenerator: no map");
    const size_t np = gridPaths.size();
    std::vector<bool> ok(np, false);
    if (np == 0) return ok;
    size_t cap = 1;
    for (const auto& p : gridPaths) cap = std::max(cap, p.size());
    std::vector<int32_t> xyz(np * cap * 3, 0), len(np);
    for (size_t p = 0; p < np; p++) {
      len[p] = (int32_t)gridPaths[p].size();
      for (size_t i = 0; i < gridPaths[p].size(); i++) {
        const std::array<int, 3> idx = coord2Index(gridPaths[p][i]);
        for (int a = 0; a < 3; a++) xyz[(p * cap + i) * 3 + a] = idx[a];
      }
    }
    direct_cube_corridor_in_t in{};
    in.batch = (int32_t)np; in.path_capacity = (int32_t)cap; in.mem_in = DIRECT_MEM_HOST; in.itr_inflate_max = itr_inflate_;
    in.path_xyz = xyz.data(); in.path_len = len.data(); in.pop_back = pop_back ? 1 : 0;
    in.seg_capacity = (int32_t)cap;  // a corridor has at most one polytope per path point: no row can overflow
    in.p_max = 6; in.plane_dtype = DIRECT_F64; in.resolution = res_;
    for (int a = 0; a < 3; a++) in.map_lower[a] = lower_[a];
    const size_t segs = np * cap;
    std::vector<int32_t> n_seg(np), rtn(np);
    std::vector<double> planes(segs * 24), seeds(segs * 3), centers(segs * 3);
    direct_cube_corridor_out_t out{};
    out.mem = DIRECT_MEM_HOST; out.n_seg = n_seg.data(); out.planes = planes.data(); out.seeds = seeds.data();
    out.centers = centers.data(); out.rtn = rtn.data();
    if (call(&in, &out) != DIRECT_OK) throw std::runtime_error(direct_cluster_last_error());
    rounds_ = 1;
    polytopes_ = 0;
    for (size_t p = 0; p < np; p++) {
      if (rtn[p] != DIRECT_CUBE_CORRIDOR_OK) continue;
      ok[p] = true;
      Corridor& cor = *corridors[p];
      for (int k = 0; k < n_seg[p]; k++) {
        const size_t at = p * cap + (size_t)k;
        typename std::decay<decltype(cor.polyhedrons[0])>::type pt{};
        for (int j = 0; j < 6; j++) {
          const double* pl = &planes[(at * 6 + j) * 4];
          pt.appendPlane({pl[0], pl[1], pl[2], pl[3]});
        }
        for (int a = 0; a < 3; a++) {
          set_elem(pt.center, a, centers[at * 3 + a]);
          set_elem(pt.seed_coord, a, seeds[at * 3 + a]);
        }
        cor.polyhedrons.push_back(pt);
        polytopes_++;
      }
    }
    return ok;
  }

  // The walk all entry points share.  pop_back: corridorGeneration's return into the last but one polytope (:524-528);
  // corridorInsertGeneration has none.
  template <class Corridor>
  std::vector<bool> walk(const std::vector<std::vector<std::array<double, 3>>>& gridPaths, const std::vector<Corridor*>& corridors,
                         bool pop_back) {
    const size_t np = gridPaths.size();
    struct Walk { size_t next = 0; std::array<double, 3> lst{{-INFINITY, -INFINITY, -INFINITY}}; bool done = false, ok = true; };
    std::vector<Walk> w(np);
    std::vector<size_t> due;          // walks waiting for a polytope
    std::vector<int32_t> seeds;
    std::vector<std::array<double, 3>> due_coord;
    rounds_ = 0;
    polytopes_ = 0;
    for (;;) {
      due.clear(); seeds.clear(); due_coord.clear();
      for (size_t p = 0; p < np; p++) {
        Walk& s = w[p];
        Corridor& cor = *corridors[p];
        while (!s.done && s.next < gridPaths[p].size()) {
          const std::array<int, 3> idx = coord2Index(gridPaths[p][s.next]);
          const std::array<double, 3> cur = index2Coord(idx);
          if (cur == s.lst) { s.next++; continue; }
          if (pop_back && isInsideLastSecondPolytope(cur, cor)) cor.polyhedrons.pop_back();  // :524-528
          if (cor.polyhedrons.empty() || isOutsideLatestPolytope(cur, cor)) {  // :413, :530
            due.push_back(p);
            seeds.insert(seeds.end(), idx.begin(), idx.end());
            due_coord.push_back(cur);
            break;  // resumes behind this point once the polytope is there
          }
          s.lst = cur;
          s.next++;
        }
        if (s.next >= gridPaths[p].size()) s.done = true;
      }
      if (due.empty()) break;
      rounds_++;
      for (size_t b0 = 0; b0 < due.size(); b0 += (size_t)max_batch_) {
        const int nb = (int)std::min((size_t)max_batch_, due.size() - b0);
        std::vector<PlainPolytope> poly;
        std::vector<int32_t> rtn;
        getConvexPolyBatch(nb, &seeds[3 * b0], poly, rtn);
        for (int b = 0; b < nb; b++) {
          Walk& s = w[due[b0 + b]];
          if (rtn[b] != DIRECT_HULL_OK) {  // the reference's cdd error branch (:548-552): the walk stops
            s.ok = false;
            s.done = true;
            continue;
          }
          Corridor& cor = *corridors[due[b0 + b]];
          typename std::decay<decltype(cor.polyhedrons[0])>::type pt{};
          for (const auto& pl : poly[b].planes) pt.appendPlane({pl[0], pl[1], pl[2], pl[3]});
          for (int a = 0; a < 3; a++) {
            set_elem(pt.center, a, poly[b].center[a]);
            set_elem(pt.seed_coord, a, due_coord[b0 + b][a]);
          }
          cor.polyhedrons.push_back(pt);
          polytopes_++;
          s.lst = due_coord[b0 + b];
          s.next++;
        }
      }
    }
    std::vector<bool> ok(np);
    for (size_t p = 0; p < np; p++) ok[p] = w[p].ok;
    return ok;
  }

 public:

  // getConvexPoly + hrep + polyHrep2Utils for `batch` seed voxels: clusters and planes never leave the device in between
  void getConvexPolyBatch(int batch, const int32_t* seed_idx, std::vector<PlainPolytope>& out, std::vector<int32_t>& rtn) {
    const int pcap = 128;  // clusters of a few thousand voxels have 20 - 50 facets
    std::vector<double> planes((size_t)batch * pcap * 4), center((size_t)batch * 3);
    std::vector<int32_t> npl(batch), crtn(batch);
    rtn.assign(batch, 0);
    if (direct_cluster_polygon_generation_batch(h_, batch, seed_idx, itr_inflate_, itr_cluster_, DIRECT_MEM_HOST, nullptr, nullptr,
                                                nullptr, nullptr, crtn.data()) != DIRECT_OK)
      throw std::runtime_error(direct_cluster_last_error());
    if (direct_cluster_hull_planes_batch(h_, batch, DIRECT_MEM_HOST, nullptr, nullptr, res_, lower_.data(), pcap, 1, DIRECT_MEM_HOST,
                                         planes.data(), nullptr, npl.data(), nullptr, nullptr, center.data(), nullptr,
                                         rtn.data()) != DIRECT_OK)
      throw std::runtime_error(direct_cluster_last_error());
    out.assign(batch, PlainPolytope());
    for (int b = 0; b < batch; b++) {
      if (crtn[b] != DIRECT_CLUSTER_OK) rtn[b] = DIRECT_HULL_OVERFLOW;
      if (rtn[b] != DIRECT_HULL_OK) continue;
      for (int k = 0; k < npl[b]; k++) {
        const double* p = &planes[((size_t)b * pcap + k) * 4];
        out[b].appendPlane({{p[0], p[1], p[2], p[3]}});
      }
      for (int a = 0; a < 3; a++) out[b].center[a] = center[(size_t)b * 3 + a];
    }
  }

  int lastRounds() const { return rounds_; }        // device batches of the last corridorGenerationBatch
  int lastPolytopes() const { return polytopes_; }  // polytopes it generated (popped ones included)
  direct_cluster_handle_t handle() const { return h_; }

 private:
  double res_, inv_res_;
  std::array<double, 3> lower_;
  int mx_, my_, mz_, itr_inflate_, itr_cluster_, max_batch_;
  direct_cluster_handle_t h_ = nullptr;
  bool has_map_ = false, table_built_ = false;
  int rounds_ = 0, polytopes_ = 0, unique_seeds_ = 0;
  int comp_min_d2_ = 0;  // the floor of the last buildFreeComponents
};

}  // namespace direct
