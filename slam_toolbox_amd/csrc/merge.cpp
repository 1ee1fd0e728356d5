// Merging mapping sessions into one occupancy map (slam_toolbox's merge_maps_kinematic, src/merge_maps_kinematic.cpp):
//
//   addSubmapCallback           :66-160    kh_merge_add_session / kh_merge_add_mapper (+ kh_merge_build_submap for the submap's own grid)
//   processInteractiveFeedback  :313-352   kh_merge_move_submap (the MOUSE_UP branch: the release of the marker)
//   transformScan               :195-248   kh_merge_get_scan (what it leaves on one scan), and the trace kernel for the readings
//   mergeMapCallback            :251-291   kh_merge_build
//   (no counterpart)                       kh_merge_fit, kh_merge_align: how well a correction places a submap among the others, and
//                                          corrections proposed by relocalizing probe scans ("Fit and alignment")
//
// The reference rewrites every scan with the correction and hands the rewritten scans to OccupancyGrid::CreateFromScans.  Here the
// scans stay as their mapper holds them -- resident in HBM, untransformed -- and the correction goes to the trace kernel as one
// record per submap (occupancy.hip, k_occ_trace_merged); the host transforms what is per scan, not per beam: the four corners of the
// box (ComputeDimensions) and the corrected pose (sensor position).  The arithmetic is stated in DESIGN.md section 7a and restated
// in numpy by tests/merge_rule.py; every operation below is in that order, and the library is built without FMA contraction.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "host_common.hpp"
#include "map_localize_plan.hpp"     // merge_fit_check: the walk-length guard of the fit
#include "mapper_internal.hpp"

namespace kh
{
namespace
{
// cos and sin of the correction's yaw are libm's cos() and sin(), each called on its own: a compiler that merges the pair into one
// sincos() call would change the last bit for some angles (mapper_pose.hpp, ref_sincos), hence the calls through volatile pointers
double (* volatile libm_cos)(double) = ::cos;
double (* volatile libm_sin)(double) = ::sin;

struct Rigid
{
  double x = 0.0, y = 0.0, yaw = 0.0;
  double c = 1.0, s = 0.0;                 // cos / sin of yaw
  Rigid() = default;
  Rigid(double x_, double y_, double yaw_) : x(x_), y(y_), yaw(yaw_), c(libm_cos(yaw_)), s(libm_sin(yaw_)) {}
  void point(double px, double py, double * ox, double * oy) const
  {
    *ox = (c * px - s * py) + x;
    *oy = (s * px + c * py) + y;
  }
  void pose(const double in[3], double out[3]) const
  {
    point(in[0], in[1], &out[0], &out[1]);
    out[2] = karto_normalize_angle(in[2] + yaw);
  }
};

Rigid compose(const Rigid & a, const Rigid & b)
{
  return Rigid(a.x + (a.c * b.x - a.s * b.y), a.y + (a.s * b.x + a.c * b.y), karto_normalize_angle(a.yaw + b.yaw));
}

// the B with B . A = identity: yaw' = NormalizeAngle(-A.yaw), position = -(R(yaw') A.position)
Rigid inverse(const Rigid & a)
{
  const double yaw = karto_normalize_angle(-a.yaw);
  const double c = libm_cos(yaw), s = libm_sin(yaw);
  return Rigid(-(c * a.x - s * a.y), -(s * a.x + c * a.y), yaw);
}

// transformScan's box: the axis-aligned box of the four transformed corners of the scan's own box
void loose_box(const Rigid & t, const double bbox[4], Box * out)
{
  const double corners[4][2] = {{bbox[0], bbox[1]}, {bbox[2], bbox[3]}, {bbox[2], bbox[1]}, {bbox[0], bbox[3]}};
  for (const auto & corner : corners) {
    double x, y;
    t.point(corner[0], corner[1], &x, &y);
    out->add(x, y);
  }
}

struct Submap
{
  int32_t id = -1;
  kh_mapper * mapper = nullptr;
  bool owned = false;
  kh_laser laser;
  Rigid correction;
  double location[3] = {0.0, 0.0, 0.0};
};

}  // namespace
}  // namespace kh

using namespace kh;

struct kh_merge
{
  int32_t device = 0;
  double resolution = 0.05;
  int32_t next_id = 0;
  std::vector<Submap> submaps;               // ascending id
  int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int64_t fit_stats[4] = {0, 0, 0, 0};       // kh_merge_fit_stats
};

namespace kh
{
namespace
{
bool finite3(const double * t) {return std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]);}

Submap * find_submap(kh_merge * g, int32_t id, const char * who)
{
  for (Submap & s : g->submaps) {if (s.id == id) {return &s;}}
  set_error(std::string(who) + ": no submap with id " + std::to_string(id));
  return nullptr;
}
const Submap * find_submap(const kh_merge * g, int32_t id, const char * who) {return find_submap(const_cast<kh_merge *>(g), id, who);}

int add_submap(kh_merge * g, kh_mapper * m, bool owned, int32_t * submap_id)
{
  Submap s;
  s.id = g->next_id++;
  s.mapper = m; s.owned = owned; s.laser = mapper_laser(m);
  // the centre of the submap's own grid (addSubmapCallback :115-122): ComputeDimensions over its untransformed boxes
  std::vector<ScanView> views;
  mapper_alive_scans(m, views);
  if (!views.empty()) {
    Box box;
    for (const ScanView & v : views) {box.add(v.bbox[0], v.bbox[1]); box.add(v.bbox[2], v.bbox[3]);}
    int32_t width, height;
    double offset[2];
    grid_dimensions(box, g->resolution, &width, &height, offset);
    s.location[0] = offset[0] + static_cast<double>(width) * g->resolution / 2.0;
    s.location[1] = offset[1] + static_cast<double>(height) * g->resolution / 2.0;
  }
  g->submaps.push_back(s);
  if (submap_id) {*submap_id = s.id;}
  return KH_OK;
}
}  // namespace
}  // namespace kh

extern "C" {

int kh_merge_create(int32_t device, double resolution, kh_merge ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (!(resolution > 0)) {kh::set_error("kh_merge_create: the resolution must be positive"); return KH_ERR_INVALID_ARG;}
  if (kh::require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_merge * g = new kh_merge();
  g->device = device; g->resolution = resolution;
  *out = g;
  return KH_OK;
}

void kh_merge_destroy(kh_merge * g)
{
  if (!g) {return;}
  for (Submap & s : g->submaps) {if (s.owned) {kh_mapper_destroy(s.mapper);}}
  delete g;
}

int kh_merge_add_mapper(kh_merge * g, kh_mapper * m, int32_t * submap_id)
{
  if (!g || !m) {return KH_ERR_INVALID_ARG;}
  if (kh::mapper_device(m) != g->device) {
    kh::set_error("kh_merge_add_mapper: the mapper is on device " + std::to_string(kh::mapper_device(m)) + ", the merger on device " +
      std::to_string(g->device));
    return KH_ERR_INVALID_ARG;
  }
  for (const Submap & s : g->submaps) {
    if (s.mapper == m) {kh::set_error("kh_merge_add_mapper: the mapper is already a submap"); return KH_ERR_INVALID_ARG;}
  }
  return kh::add_submap(g, m, false, submap_id);
}

int kh_merge_add_session(kh_merge * g, const char * path, int32_t * submap_id)
{
  if (!g || !path) {return KH_ERR_INVALID_ARG;}
  kh_mapper * m = nullptr;
  // (a mapper loaded to be merged matches nothing: the smallest candidate batch)
  const int rc = kh_mapper_load(path, &g->device, 1, 1, &m);
  if (rc) {return rc;}
  return kh::add_submap(g, m, true, submap_id);
}

int kh_merge_remove_submap(kh_merge * g, int32_t submap_id)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  Submap * s = kh::find_submap(g, submap_id, "kh_merge_remove_submap");
  if (!s) {return KH_ERR_NOT_FOUND;}
  if (s->owned) {kh_mapper_destroy(s->mapper);}
  g->submaps.erase(g->submaps.begin() + (s - g->submaps.data()));
  return KH_OK;
}

int32_t kh_merge_num_submaps(const kh_merge * g) {return g ? static_cast<int32_t>(g->submaps.size()) : 0;}

int kh_merge_submap_info(const kh_merge * g, int32_t submap_id, int32_t out[2])
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  const Submap * s = kh::find_submap(g, submap_id, "kh_merge_submap_info");
  if (!s) {return KH_ERR_NOT_FOUND;}
  out[0] = kh_mapper_num_alive(s->mapper); out[1] = s->laser.n_beams;
  return KH_OK;
}

int kh_merge_set_transform(kh_merge * g, int32_t submap_id, const double t[3])
{
  if (!g || !t) {return KH_ERR_INVALID_ARG;}
  Submap * s = kh::find_submap(g, submap_id, "kh_merge_set_transform");
  if (!s) {return KH_ERR_NOT_FOUND;}
  if (!kh::finite3(t)) {kh::set_error("kh_merge_set_transform: the correction is not finite"); return KH_ERR_INVALID_ARG;}
  s->correction = Rigid(t[0], t[1], t[2]);
  return KH_OK;
}

int kh_merge_get_transform(const kh_merge * g, int32_t submap_id, double t[3])
{
  if (!g || !t) {return KH_ERR_INVALID_ARG;}
  const Submap * s = kh::find_submap(g, submap_id, "kh_merge_get_transform");
  if (!s) {return KH_ERR_NOT_FOUND;}
  t[0] = s->correction.x; t[1] = s->correction.y; t[2] = s->correction.yaw;
  return KH_OK;
}

int kh_merge_move_submap(kh_merge * g, int32_t submap_id, const double marker_pose[3])
{
  if (!g || !marker_pose) {return KH_ERR_INVALID_ARG;}
  Submap * s = kh::find_submap(g, submap_id, "kh_merge_move_submap");
  if (!s) {return KH_ERR_NOT_FOUND;}
  if (!kh::finite3(marker_pose)) {kh::set_error("kh_merge_move_submap: the marker pose is not finite"); return KH_ERR_INVALID_ARG;}
  // processInteractiveFeedback :327-351: correction * previous_submap_correction.inverse() * new_submap_location, left to right
  const Rigid previous(s->location[0], s->location[1], 0.0);
  const Rigid marker(marker_pose[0], marker_pose[1], marker_pose[2]);
  s->correction = compose(compose(s->correction, inverse(previous)), marker);
  s->location[0] = marker_pose[0]; s->location[1] = marker_pose[1]; s->location[2] = s->location[2] + marker_pose[2];
  return KH_OK;
}

int kh_merge_get_location(const kh_merge * g, int32_t submap_id, double location[3])
{
  if (!g || !location) {return KH_ERR_INVALID_ARG;}
  const Submap * s = kh::find_submap(g, submap_id, "kh_merge_get_location");
  if (!s) {return KH_ERR_NOT_FOUND;}
  std::copy(s->location, s->location + 3, location);
  return KH_OK;
}

int kh_merge_get_scan(const kh_merge * g, int32_t submap_id, int32_t index, double corrected_pose[3], double odometric_pose[3],
  double barycenter_pose[3], double box[4], double * points_xy)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  const Submap * s = kh::find_submap(g, submap_id, "kh_merge_get_scan");
  if (!s) {return KH_ERR_NOT_FOUND;}
  std::vector<ScanView> views;
  kh::mapper_alive_scans(s->mapper, views);
  if (index < 0 || static_cast<size_t>(index) >= views.size()) {
    kh::set_error("kh_merge_get_scan: submap " + std::to_string(submap_id) + " has no scan " + std::to_string(index));
    return KH_ERR_NOT_FOUND;
  }
  const ScanView & v = views[static_cast<size_t>(index)];
  const Rigid & t = s->correction;
  if (corrected_pose) {t.pose(v.corrected, corrected_pose);}
  if (odometric_pose) {t.pose(v.odometric, odometric_pose);}
  if (barycenter_pose) {t.pose(v.barycenter, barycenter_pose);}
  if (box) {
    Box b;
    loose_box(t, v.bbox, &b);
    box[0] = b.min_x; box[1] = b.min_y; box[2] = b.max_x; box[3] = b.max_y;
  }
  if (points_xy) {
    for (int32_t i = 0; i < s->laser.n_beams; ++i) {t.point(v.points[2 * i], v.points[2 * i + 1], &points_xy[2 * i], &points_xy[2 * i + 1]);}
  }
  return KH_OK;
}

int kh_merge_build_submap(kh_merge * g, int32_t submap_id, uint32_t min_pass_through, double occupancy_threshold, kh_occupancy ** out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  Submap * s = kh::find_submap(g, submap_id, "kh_merge_build_submap");
  if (!s) {return KH_ERR_NOT_FOUND;}
  return kh_mapper_build_map(s->mapper, g->resolution, min_pass_through, occupancy_threshold, out);
}

}  // extern "C"

namespace kh
{
namespace
{
// What kh_merge_build does, over every submap but `skip` (-1: none): the grid, traced and updated.  uploads[0], [1] = point-reading
// and range uploads made, [2] = bytes of the two tables.
int build_grid(kh_merge * g, int32_t skip, const char * who, uint32_t min_pass_through, double occupancy_threshold, kh_occupancy ** out,
  int64_t * n_scans_out, int64_t * n_beams_out, int64_t uploads[3])
{
  const std::string name(who);
  // ComputeDimensions (Karto.h:6086-6112) over the boxes transformScan leaves
  std::vector<const Submap *> subs;
  for (const Submap & s : g->submaps) {if (s.id != skip) {subs.push_back(&s);}}
  if (subs.empty()) {set_error(name + (skip < 0 ? ": no submap" : ": no other submap")); return KH_ERR_INVALID_ARG;}
  std::vector<std::vector<ScanView>> views(subs.size());
  Box box;
  int64_t n_scans = 0, n_beams = 0;
  int32_t max_beams = 0;
  for (size_t k = 0; k < subs.size(); ++k) {
    const Submap & s = *subs[k];
    mapper_alive_scans(s.mapper, views[k]);
    for (const ScanView & v : views[k]) {loose_box(s.correction, v.bbox, &box);}
    n_scans += static_cast<int64_t>(views[k].size());
    n_beams += static_cast<int64_t>(views[k].size()) * s.laser.n_beams;
    if (!views[k].empty()) {max_beams = std::max(max_beams, s.laser.n_beams);}
  }
  if (n_scans == 0) {set_error(name + (skip < 0 ? ": no scan in any submap" : ": no scan in any other submap")); return KH_ERR_INVALID_ARG;}
  if (n_scans > INT32_MAX) {set_error(name + ": too many scans"); return KH_ERR_INVALID_ARG;}
  int32_t width, height;
  double offset[2];
  grid_dimensions(box, g->resolution, &width, &height, offset);
  kh_occupancy * grid = nullptr;
  int rc = kh_occupancy_create(width, height, offset[0], offset[1], g->resolution, g->device, &grid);
  if (rc) {return rc;}
  void * stream = occupancy_stream(grid);
  auto fail = [&](int code) {stream_synchronize(stream); kh_occupancy_destroy(grid); return code;};
  std::vector<MergeScan> scan_table;
  std::vector<MergeSubmap> submap_table;
  std::vector<ResidentScan> resident;
  scan_table.reserve(static_cast<size_t>(n_scans));
  int64_t up_points = 0, up_ranges = 0;
  for (size_t k = 0; k < subs.size(); ++k) {
    const Submap & s = *subs[k];
    const Rigid & t = s.correction;
    MergeSubmap rec = {};                          // (value-initialised: the pad words are uploaded too)
    rec.c = t.c; rec.s = t.s; rec.tx = t.x; rec.ty = t.y;
    rec.range_threshold = s.laser.range_threshold; rec.min_range = s.laser.minimum_range; rec.max_range = s.laser.maximum_range;
    rec.n_beams = s.laser.n_beams;
    submap_table.push_back(rec);
    // the residency loop kh_mapper_build_map runs: the correction is no reason to upload
    int64_t up_p = 0, up_r = 0;
    rc = mapper_resident_table(s.mapper, stream, who, resident, &up_p, &up_r);
    if (rc) {return fail(rc);}
    up_points += up_p; up_ranges += up_r;
    if (resident.size() != views[k].size()) {set_error(name + ": a submap changed during the merge"); return fail(KH_ERR_INVALID_ARG);}
    for (size_t i = 0; i < views[k].size(); ++i) {
      // GetSensorPose() of the transformed scan = GetSensorAt(transformed corrected pose), Karto.h:5566-5569
      double corrected[3], sensor[3];
      t.pose(views[k][i].corrected, corrected);
      laser_sensor_at(s.laser, corrected, sensor);
      MergeScan scan = {};
      scan.points = resident[i].points; scan.ranges = resident[i].ranges;
      scan.sx = sensor[0]; scan.sy = sensor[1]; scan.submap = static_cast<int32_t>(k);
      scan_table.push_back(scan);
    }
  }
  rc = occupancy_add_merged(grid, static_cast<int32_t>(n_scans), scan_table.data(), static_cast<int32_t>(subs.size()), submap_table.data(),
      max_beams, n_beams);
  if (rc == KH_OK) {rc = kh_occupancy_update(grid, min_pass_through, occupancy_threshold);}
  if (rc) {return fail(rc);}
  *n_scans_out = n_scans; *n_beams_out = n_beams;
  uploads[0] = up_points; uploads[1] = up_ranges;
  uploads[2] = static_cast<int64_t>(scan_table.size() * sizeof(MergeScan) + submap_table.size() * sizeof(MergeSubmap));
  *out = grid;
  return KH_OK;
}

// The fit of n candidate corrections of submap `moving` against the merge of all the others: the reference
// grid once, then one launch of k_occ_fit_merged.  times_ms[0] = the reference grid (wall), [1] = the fit kernel (events).
int fit_candidates(kh_merge * g, const Submap & moving, const char * who, int32_t n, const double * corrections, uint32_t min_pass_through,
  double occupancy_threshold, kh_merge_fit_t * out, double times_ms[2])
{
  const auto t_begin = std::chrono::steady_clock::now();
  kh_occupancy * grid = nullptr;
  int64_t n_ref_scans = 0, n_ref_beams = 0, uploads[3];
  int rc = build_grid(g, moving.id, who, min_pass_through, occupancy_threshold, &grid, &n_ref_scans, &n_ref_beams, uploads);
  if (rc) {return rc;}
  times_ms[0] = ms_since(t_begin);
  void * stream = occupancy_stream(grid);
  auto done = [&](int code) {stream_synchronize(stream); kh_occupancy_destroy(grid); return code;};
  std::vector<ScanView> views;
  std::vector<ResidentScan> resident;
  mapper_alive_scans(moving.mapper, views);
  int64_t up_p = 0, up_r = 0;
  rc = mapper_resident_table(moving.mapper, stream, who, resident, &up_p, &up_r);
  if (rc) {return done(rc);}
  if (resident.size() != views.size()) {set_error(std::string(who) + ": the submap changed during the fit"); return done(KH_ERR_INVALID_ARG);}
  const size_t n_scans = views.size();
  if (n_scans > static_cast<size_t>(INT32_MAX)) {set_error(std::string(who) + ": too many scans"); return done(KH_ERR_INVALID_ARG);}
  std::vector<FitCandidate> candidates(static_cast<size_t>(n));
  std::vector<FitSensor> sensors(static_cast<size_t>(n) * n_scans);
  for (int32_t k = 0; k < n; ++k) {
    const Rigid t(corrections[3 * k], corrections[3 * k + 1], corrections[3 * k + 2]);
    candidates[static_cast<size_t>(k)] = FitCandidate{t.c, t.s, t.x, t.y};
    for (size_t i = 0; i < n_scans; ++i) {
      // GetSensorAt(transformed corrected pose), as build_grid does once per scan
      double corrected[3], sensor[3];
      t.pose(views[i].corrected, corrected);
      laser_sensor_at(moving.laser, corrected, sensor);
      sensors[static_cast<size_t>(k) * n_scans + i] = FitSensor{sensor[0], sensor[1]};
    }
  }
  // The walk-length guard (merge_fit_check, map_localize_plan.hpp): a candidate may put the submap anywhere, a walk is as long as its
  // end cells are apart, and the kernel's own bound only keeps a lane from spinning.  The scale is the grid's own (kh_occupancy_create).
  static_assert(sizeof(FitSensor) == 2 * sizeof(double), "the sensors are checked as they lie: pairs (x, y)");
  double offset[2] = {0.0, 0.0};
  rc = kh_occupancy_geometry(grid, offset, nullptr);
  if (rc) {return done(rc);}
  const FitInputs inputs = merge_fit_check(moving.laser.range_threshold, moving.laser.minimum_range, moving.laser.maximum_range,
      static_cast<size_t>(n), n_scans, sensors.empty() ? nullptr : &sensors[0].sx, offset[0], offset[1], 1.0 / g->resolution);
  if (inputs.failed != kFitInputsOk) {
    set_error(fit_inputs_text(inputs, who, kMergeLaserWords, kMergePoseWords));
    return done(KH_ERR_INVALID_ARG);
  }
  std::vector<uint64_t> sums(static_cast<size_t>(n) * kFitCounters);
  rc = occupancy_fit_merged(grid, n, candidates.data(), sensors.data(), static_cast<int32_t>(n_scans), resident.data(), moving.laser.n_beams,
      moving.laser.range_threshold, moving.laser.minimum_range, moving.laser.maximum_range, sums.data(), &times_ms[1]);
  if (rc) {return done(rc);}
  for (int32_t k = 0; k < n; ++k) {
    const uint64_t * c = &sums[static_cast<size_t>(k) * kFitCounters];
    kh_merge_fit_t & f = out[k];
    f.pass_unknown = c[kFitPassUnknown]; f.pass_occupied = c[kFitPassOccupied]; f.pass_free = c[kFitPassFree];
    f.hits_unknown = c[kFitHitsUnknown]; f.hits_occupied = c[kFitHitsOccupied]; f.hits_free = c[kFitHitsFree];
    // pass - 2 hits = the visits that are not the end cell of a hit beam (that cell is visited twice: by the line, and as the hit)
    f.agree = f.hits_occupied + (f.pass_free - 2 * f.hits_free);
    f.conflict = (f.pass_occupied - 2 * f.hits_occupied) + f.hits_free;
    f.known = f.agree + f.conflict;
    f.score = f.known == 0 ? 0.0 : static_cast<double>(f.agree) / static_cast<double>(f.known);
  }
  g->fit_stats[0] += 1; g->fit_stats[1] += n;
  g->fit_stats[2] = static_cast<int64_t>(n_scans) * moving.laser.n_beams * n;
  g->fit_stats[3] = static_cast<int64_t>(times_ms[1] * 1000.0);
  return done(KH_OK);
}

// the fit's ranking: enough known visits first, then score descending, agree descending, index ascending
bool fit_before(const kh_merge_align_cand & a, const kh_merge_align_cand & b)
{
  if (a.enough != b.enough) {return a.enough > b.enough;}
  if (a.fit.score != b.fit.score) {return a.fit.score > b.fit.score;}
  if (a.fit.agree != b.fit.agree) {return a.fit.agree > b.fit.agree;}
  return a.index < b.index;
}

bool same_laser(const kh_laser & a, const kh_laser & b)
{
  return a.n_beams == b.n_beams && a.minimum_angle == b.minimum_angle && a.angular_resolution == b.angular_resolution &&
         a.minimum_range == b.minimum_range && a.maximum_range == b.maximum_range && a.range_threshold == b.range_threshold &&
         a.offset_x == b.offset_x && a.offset_y == b.offset_y && a.offset_heading == b.offset_heading;
}
}  // namespace
}  // namespace kh

extern "C" {

int kh_merge_build(kh_merge * g, uint32_t min_pass_through, double occupancy_threshold, kh_occupancy ** out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  int64_t n_scans = 0, n_beams = 0, uploads[3];
  const int rc = kh::build_grid(g, -1, "kh_merge_build", min_pass_through, occupancy_threshold, out, &n_scans, &n_beams, uploads);
  if (rc) {return rc;}
  g->stats[0] += 1; g->stats[1] = n_scans; g->stats[2] = n_beams; g->stats[3] = uploads[0]; g->stats[4] = uploads[1];
  g->stats[5] += uploads[0]; g->stats[6] += uploads[1];
  g->stats[7] = uploads[2];
  return KH_OK;
}

int kh_merge_stats(const kh_merge * g, int64_t out[8])
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  std::copy(g->stats, g->stats + 8, out);
  return KH_OK;
}

int kh_merge_fit(kh_merge * g, int32_t submap_id, int32_t n_candidates, const double * corrections, uint32_t min_pass_through,
  double occupancy_threshold, kh_merge_fit_t * out)
{
  if (!corrections || !out || n_candidates < 1) {return KH_ERR_INVALID_ARG;}
  if (!std::isfinite(occupancy_threshold)) {kh::set_error("kh_merge_fit: the occupancy threshold is not finite"); return KH_ERR_INVALID_ARG;}
  for (int32_t k = 0; k < n_candidates; ++k) {
    if (!kh::finite3(corrections + 3 * k)) {kh::set_error("kh_merge_fit: correction " + std::to_string(k) + " is not finite"); return KH_ERR_INVALID_ARG;}
  }
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!g) {return KH_ERR_INVALID_ARG;}
  const Submap * s = kh::find_submap(g, submap_id, "kh_merge_fit");
  if (!s) {return KH_ERR_NOT_FOUND;}
  double times_ms[2] = {0.0, 0.0};
  return kh::fit_candidates(g, *s, "kh_merge_fit", n_candidates, corrections, min_pass_through, occupancy_threshold, out, times_ms);
}

int kh_merge_fit_stats(const kh_merge * g, int64_t out[4])
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  std::copy(g->fit_stats, g->fit_stats + 4, out);
  return KH_OK;
}

void kh_merge_align_params_default(const kh_merge * g, int32_t target_submap, kh_merge_align_params * p)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  p->n_probes = 4; p->top_k = 4; p->min_known = 0;
  p->min_pass_through = 2; p->occupancy_threshold = 0.1;          // OccupancyGrid's defaults, as slam_toolbox merges with
  // the relocalization defaults of the target's mapper (of kh_mapper_params_default where there is none to ask)
  kh_mapper_params mp;
  const Submap * s = g ? kh::find_submap(g, target_submap, "kh_merge_align_params_default") : nullptr;
  const bool have = s && kh_mapper_get_params(s->mapper, &mp) == KH_OK;
  kh_relocalize_params_default(have ? &mp : nullptr, &p->relocalize);
}

int kh_merge_align(kh_merge * g, int32_t moving_submap, int32_t target_submap, const kh_merge_align_params * params, kh_merge_align_cand * out,
  int32_t cap, int32_t * n_candidates, double times_ms[4])
{
  if (!params || !n_candidates || cap < 0 || (cap > 0 && !out)) {return KH_ERR_INVALID_ARG;}
  *n_candidates = 0;
  if (times_ms) {std::fill(times_ms, times_ms + 4, 0.0);}
  const kh_relocalize_params & rp = params->relocalize;
  if (params->n_probes < 1 || params->top_k < 1 || !std::isfinite(params->occupancy_threshold) || !(rp.seed_spacing > 0) ||
    !std::isfinite(rp.seed_spacing) || rp.n_headings < 0 || rp.max_base < 1 || !std::isfinite(rp.radius) || !std::isfinite(rp.center_xy[0]) ||
    !std::isfinite(rp.center_xy[1]))
  {
    kh::set_error("kh_merge_align: n_probes >= 1, top_k >= 1, a finite occupancy_threshold and valid relocalization parameters are required");
    return KH_ERR_INVALID_ARG;
  }
  if (moving_submap == target_submap) {kh::set_error("kh_merge_align: a submap cannot be aligned to itself"); return KH_ERR_INVALID_ARG;}
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!g) {return KH_ERR_INVALID_ARG;}
  const auto t_begin = std::chrono::steady_clock::now();
  const Submap * moving = kh::find_submap(g, moving_submap, "kh_merge_align");
  const Submap * target = moving ? kh::find_submap(g, target_submap, "kh_merge_align") : nullptr;
  if (!moving || !target) {return KH_ERR_NOT_FOUND;}
  if (!kh::same_laser(moving->laser, target->laser)) {
    kh::set_error("kh_merge_align: the two submaps have different lasers (the probe's ranges are read by the target's laser)");
    return KH_ERR_INVALID_ARG;
  }
  // candidate 0: what the moving submap has now
  std::vector<kh_merge_align_cand> cands(1);
  std::memset(&cands[0], 0, sizeof(cands[0]));
  cands[0].correction[0] = moving->correction.x; cands[0].correction[1] = moving->correction.y; cands[0].correction[2] = moving->correction.yaw;
  cands[0].probe_scan = -1; cands[0].hypothesis = -1;
  // the probes: entry floor(j * n_alive / n_probes) of the alive scans, each relocalized in the target's map
  std::vector<ScanView> views;
  kh::mapper_alive_scans(moving->mapper, views);
  const int64_t n_alive = static_cast<int64_t>(views.size());
  const int64_t n_probes = std::min<int64_t>(params->n_probes, n_alive);
  kh_relocalize_params relocalize = rp;
  relocalize.top_k = params->top_k;
  std::vector<kh_relocalize_hyp> hyps(static_cast<size_t>(params->top_k));
  const auto t_relocalize = std::chrono::steady_clock::now();
  for (int64_t j = 0; j < n_probes; ++j) {
    const ScanView & probe = views[static_cast<size_t>(j * n_alive / n_probes)];
    kh_relocalize_summary summary;
    const int rc = kh_mapper_relocalize(target->mapper, probe.ranges, &relocalize, hyps.data(), params->top_k, &summary);
    if (rc) {return rc;}
    const Rigid q(probe.corrected[0], probe.corrected[1], probe.corrected[2]);
    for (int32_t h = 0; h < summary.n_returned; ++h) {
      // C = T_target . P . inverse(Q), left to right: the probe, at Q in its own session, stands at P in the target's
      const double * pose = hyps[static_cast<size_t>(h)].robot_pose;
      const Rigid c = compose(compose(target->correction, Rigid(pose[0], pose[1], pose[2])), inverse(q));
      kh_merge_align_cand cand;
      std::memset(&cand, 0, sizeof(cand));
      cand.correction[0] = c.x; cand.correction[1] = c.y; cand.correction[2] = c.yaw;
      cand.probe_scan = probe.id; cand.hypothesis = h; cand.fine_response = hyps[static_cast<size_t>(h)].fine_response;
      cands.push_back(cand);
    }
  }
  const double relocalize_ms = kh::ms_since(t_relocalize);
  if (cands.size() > static_cast<size_t>(INT32_MAX)) {kh::set_error("kh_merge_align: too many candidates"); return KH_ERR_INVALID_ARG;}
  const int32_t n = static_cast<int32_t>(cands.size());
  std::vector<double> corrections(3 * cands.size());
  for (size_t k = 0; k < cands.size(); ++k) {
    if (!kh::finite3(cands[k].correction)) {kh::set_error("kh_merge_align: a candidate correction is not finite"); return KH_ERR_INVALID_ARG;}
    std::copy(cands[k].correction, cands[k].correction + 3, &corrections[3 * k]);
  }
  std::vector<kh_merge_fit_t> fits(cands.size());
  double fit_ms[2] = {0.0, 0.0};
  const int rc = kh::fit_candidates(g, *moving, "kh_merge_align", n, corrections.data(), params->min_pass_through, params->occupancy_threshold,
      fits.data(), fit_ms);
  if (rc) {return rc;}
  for (int32_t k = 0; k < n; ++k) {
    cands[static_cast<size_t>(k)].fit = fits[static_cast<size_t>(k)];
    cands[static_cast<size_t>(k)].index = k; cands[static_cast<size_t>(k)].enough = fits[static_cast<size_t>(k)].known >= params->min_known ? 1 : 0;
  }
  std::sort(cands.begin(), cands.end(), kh::fit_before);
  std::copy(cands.begin(), cands.begin() + std::min(cap, n), out);
  *n_candidates = n;
  if (times_ms) {times_ms[0] = relocalize_ms; times_ms[1] = fit_ms[0]; times_ms[2] = fit_ms[1]; times_ms[3] = kh::ms_since(t_begin);}
  return KH_OK;
}

}  // extern "C"
