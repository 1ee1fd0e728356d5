// Merging mapping sessions into one occupancy map (slam_toolbox's merge_maps_kinematic, src/merge_maps_kinematic.cpp):
//
//   addSubmapCallback           :66-160    kh_merge_add_session / kh_merge_add_mapper (+ kh_merge_build_submap for the submap's own grid)
//   processInteractiveFeedback  :313-352   kh_merge_move_submap (the MOUSE_UP branch: the release of the marker)
//   transformScan               :195-248   kh_merge_get_scan (what it leaves on one scan), and the trace kernel for the readings
//   mergeMapCallback            :251-291   kh_merge_build
//
// The reference rewrites every scan with the correction and hands the rewritten scans to OccupancyGrid::CreateFromScans.  Here the
// scans stay as their mapper holds them -- resident in HBM, untransformed -- and the correction goes to the trace kernel as one
// record per submap (occupancy.hip, k_occ_trace_merged); the host transforms what is per scan, not per beam: the four corners of the
// box (ComputeDimensions) and the corrected pose (sensor position).  The arithmetic is stated in DESIGN.md section 7a and restated
// in numpy by tests/merge_rule.py; every operation below is in that order, and the library is built without FMA contraction.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "mapper_internal.hpp"

namespace kh
{
void set_error(const std::string & s);
void stream_synchronize(void * hip_stream);      // comm.cpp

namespace
{
// cos and sin of the correction's yaw are libm's cos() and sin(), each called on its own: a compiler that merges the pair into one
// sincos() call would change the last bit for some angles (mapper_host.cpp, ref_sincos), hence the calls through volatile pointers
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
};

namespace kh
{
namespace
{
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

int kh_merge_build(kh_merge * g, uint32_t min_pass_through, double occupancy_threshold, kh_occupancy ** out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (g->submaps.empty()) {kh::set_error("kh_merge_build: no submap"); return KH_ERR_INVALID_ARG;}
  // ComputeDimensions (Karto.h:6086-6112) over the boxes transformScan leaves
  std::vector<std::vector<ScanView>> views(g->submaps.size());
  Box box;
  int64_t n_scans = 0, n_beams = 0;
  int32_t max_beams = 0;
  for (size_t k = 0; k < g->submaps.size(); ++k) {
    const Submap & s = g->submaps[k];
    kh::mapper_alive_scans(s.mapper, views[k]);
    for (const ScanView & v : views[k]) {loose_box(s.correction, v.bbox, &box);}
    n_scans += static_cast<int64_t>(views[k].size());
    n_beams += static_cast<int64_t>(views[k].size()) * s.laser.n_beams;
    if (!views[k].empty()) {max_beams = std::max(max_beams, s.laser.n_beams);}
  }
  if (n_scans == 0) {kh::set_error("kh_merge_build: no scan in any submap"); return KH_ERR_INVALID_ARG;}
  if (n_scans > INT32_MAX) {kh::set_error("kh_merge_build: too many scans"); return KH_ERR_INVALID_ARG;}
  int32_t width, height;
  double offset[2];
  kh::grid_dimensions(box, g->resolution, &width, &height, offset);
  kh_occupancy * grid = nullptr;
  int rc = kh_occupancy_create(width, height, offset[0], offset[1], g->resolution, g->device, &grid);
  if (rc) {return rc;}
  void * stream = kh::occupancy_stream(grid);
  auto fail = [&](int code) {kh::stream_synchronize(stream); kh_occupancy_destroy(grid); return code;};
  std::vector<MergeScan> scan_table;
  std::vector<MergeSubmap> submap_table;
  std::vector<ResidentScan> resident;
  scan_table.reserve(static_cast<size_t>(n_scans));
  int64_t up_points = 0, up_ranges = 0;
  for (size_t k = 0; k < g->submaps.size(); ++k) {
    const Submap & s = g->submaps[k];
    const Rigid & t = s.correction;
    MergeSubmap rec = {};                          // (value-initialised: the pad words are uploaded too)
    rec.c = t.c; rec.s = t.s; rec.tx = t.x; rec.ty = t.y;
    rec.range_threshold = s.laser.range_threshold; rec.min_range = s.laser.minimum_range; rec.max_range = s.laser.maximum_range;
    rec.n_beams = s.laser.n_beams;
    submap_table.push_back(rec);
    // the residency loop kh_mapper_build_map runs: the correction is no reason to upload
    int64_t up_p = 0, up_r = 0;
    rc = kh::mapper_resident_table(s.mapper, stream, "kh_merge_build", resident, &up_p, &up_r);
    if (rc) {return fail(rc);}
    up_points += up_p; up_ranges += up_r;
    if (resident.size() != views[k].size()) {kh::set_error("kh_merge_build: a submap changed during the merge"); return fail(KH_ERR_INVALID_ARG);}
    for (size_t i = 0; i < views[k].size(); ++i) {
      // GetSensorPose() of the transformed scan = GetSensorAt(transformed corrected pose), Karto.h:5566-5569
      double corrected[3], sensor[3];
      t.pose(views[k][i].corrected, corrected);
      kh::laser_sensor_at(s.laser, corrected, sensor);
      MergeScan scan = {};
      scan.points = resident[i].points; scan.ranges = resident[i].ranges;
      scan.sx = sensor[0]; scan.sy = sensor[1]; scan.submap = static_cast<int32_t>(k);
      scan_table.push_back(scan);
    }
  }
  rc = kh::occupancy_add_merged(grid, static_cast<int32_t>(n_scans), scan_table.data(), static_cast<int32_t>(g->submaps.size()), submap_table.data(),
      max_beams, n_beams);
  if (rc == KH_OK) {rc = kh_occupancy_update(grid, min_pass_through, occupancy_threshold);}
  if (rc) {return fail(rc);}
  g->stats[0] += 1; g->stats[1] = n_scans; g->stats[2] = n_beams; g->stats[3] = up_points; g->stats[4] = up_ranges;
  g->stats[5] += up_points; g->stats[6] += up_ranges;
  g->stats[7] = static_cast<int64_t>(scan_table.size() * sizeof(MergeScan) + submap_table.size() * sizeof(MergeSubmap));
  *out = grid;
  return KH_OK;
}

int kh_merge_stats(const kh_merge * g, int64_t out[8])
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  std::copy(g->stats, g->stats + 8, out);
  return KH_OK;
}

}  // extern "C"
