// What the session merger (merge.cpp) and the live map (live_map.cpp) read of a mapper (mapper_internal.hpp), and the occupancy
// map made from the scans where they lie in HBM (kh_mapper_build_map).
#include <algorithm>
#include <string>

#include "mapper_internal.hpp"
#include "mapper_private.hpp"

namespace kh
{
using namespace mapper;

// The residency loop kh_mapper_build_map and the session merger (merge.cpp) share: every scan still in the map gets its ranges
// (once in its life) and its point readings (again only after its pose moved) into HBM on the mapper's own device, the uploads
// queued on `stream`; table gains one record per scan in id order (ResidentScan, the record of kh::occupancy_add_resident).
// *up_points / *up_ranges = uploads this call made.
// ids = NULL: every scan still in the map; otherwise the n_ids scans named (each still in the map), in the order given.
int mapper_resident_table_of(kh_mapper * m, void * stream, const char * who, const int32_t * ids, size_t n_ids, std::vector<ResidentScan> & table,
  int64_t * up_points, int64_t * up_ranges)
{
  const int64_t range_bytes = static_cast<int64_t>(sizeof(double)) * m->laser.n;
  table.clear();
  table.reserve(ids ? n_ids : m->scans.size());
  *up_points = 0; *up_ranges = 0;
  const size_t n_visit = ids ? n_ids : m->scans.size();
  for (size_t k = 0; k < n_visit; ++k) {
    const size_t id = ids ? static_cast<size_t>(ids[k]) : k;
    if (!scan_alive(m, static_cast<int32_t>(id))) {
      if (!ids) {continue;}
      set_error(std::string(who) + ": scan " + std::to_string(id) + " is not in the map");
      return KH_ERR_NOT_FOUND;
    }
    MScan & s = *m->scans[id];
    if (!s.d_ranges) {
      s.d_ranges = take_slot(m->r_slabs, m->r_free_slots, m->device, static_cast<size_t>(m->laser.n));
      if (s.d_ranges) {s.d_ranges_fresh = false;}
    }
    if (s.d_ranges && !s.d_ranges_fresh && s.ranges.size() == static_cast<size_t>(m->laser.n) &&
      kh_device_upload_on(s.d_ranges, s.ranges.data(), range_bytes, stream) == KH_OK) {s.d_ranges_fresh = true; ++*up_ranges;}
    const bool points_stale = !(s.d_points[0] && (s.d_fresh & 1u));
    const double * d_points = resident_points(m, s, 0, stream);
    if (!d_points || !s.d_ranges || !s.d_ranges_fresh) {
      set_error(std::string(who) + ": a scan could not be made resident on the device");
      return KH_ERR_HIP;
    }
    *up_points += points_stale ? 1 : 0;
    table.push_back(ResidentScan{d_points, s.d_ranges, s.sensor.x, s.sensor.y});
  }
  return KH_OK;
}

int mapper_resident_table(kh_mapper * m, void * stream, const char * who, std::vector<ResidentScan> & table, int64_t * up_points, int64_t * up_ranges)
{
  return mapper_resident_table_of(m, stream, who, nullptr, 0, table, up_points, up_ranges);
}

void mapper_sensor_poses(const kh_mapper * m, std::vector<SensorView> & out)
{
  out.clear();
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    SensorView v;
    v.id = sp->id; put_pose(sp->sensor, v.sensor);
    std::copy(sp->bbox, sp->bbox + 4, v.bbox);
    out.push_back(v);
  }
}

// what merge.cpp reads of a mapper (mapper_internal.hpp)
int32_t mapper_device(const kh_mapper * m) {return m->device;}

kh_laser mapper_laser(const kh_mapper * m) {return to_kh_laser(m->laser);}

void mapper_alive_scans(const kh_mapper * m, std::vector<ScanView> & out)
{
  out.clear();
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    ScanView v;
    v.id = sp->id; v.points = sp->points.data(); v.ranges = sp->ranges.data();
    put_pose(sp->corrected, v.corrected); put_pose(sp->odometric, v.odometric);
    v.barycenter[0] = sp->barycenter[0]; v.barycenter[1] = sp->barycenter[1];
    v.barycenter[2] = sp->n_filtered != 0 ? 0.0 : sp->sensor.h;       // Pose2(averagePosition, 0.0), or the sensor pose (Karto.h:5687-5692)
    std::copy(sp->bbox, sp->bbox + 4, v.bbox);
    out.push_back(v);
  }
}

void laser_sensor_at(const kh_laser & laser, const double robot[3], double sensor[3])
{
  put_pose(sensor_at(to_laser(laser), to_pose(robot)), sensor);
}

double karto_normalize_angle(double angle) {return normalize_angle(angle);}
}  // namespace kh

using namespace kh;

extern "C" {

// OccupancyGrid::CreateFromScans (Karto.h:5947-5962) from the scans where they lie in HBM
int kh_mapper_build_map(kh_mapper * m, double resolution, uint32_t min_pass_through, double occupancy_threshold, kh_occupancy ** out)
{
  if (!m || !out || !(resolution > 0)) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  // ComputeDimensions (Karto.h:6086-6112): every scan's box is the min / max of its sensor position and its in-range readings
  // (update_scan), so the min / max over the boxes are the min / max kh_occupancy_compute_dimensions finds beam by beam
  kh::Box box;
  int32_t n_alive = 0;
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    ++n_alive;
    box.add(sp->bbox[0], sp->bbox[1]); box.add(sp->bbox[2], sp->bbox[3]);
  }
  if (n_alive == 0) {kh::set_error("kh_mapper_build_map: no scan in the map"); return KH_ERR_INVALID_ARG;}
  int32_t width, height;
  double offset[2];
  kh::grid_dimensions(box, resolution, &width, &height, offset);
  kh_occupancy * g = nullptr;
  int rc = kh_occupancy_create(width, height, offset[0], offset[1], resolution, m->device, &g);
  if (rc) {return rc;}
  void * stream = kh::occupancy_stream(g);
  std::vector<kh::ResidentScan> table;
  int64_t up_points = 0, up_ranges = 0;
  rc = kh::mapper_resident_table(m, stream, "kh_mapper_build_map", table, &up_points, &up_ranges);
  if (rc) {kh::stream_synchronize(stream); kh_occupancy_destroy(g); return rc;}
  rc = kh::occupancy_add_resident(g, n_alive, table.data(), m->laser.n, m->laser.range_threshold, m->laser.min_range, m->laser.max_range);
  if (rc == KH_OK) {rc = kh_occupancy_update(g, min_pass_through, occupancy_threshold);}
  if (rc) {kh::stream_synchronize(stream); kh_occupancy_destroy(g); return rc;}
  m->map_stats[0] += 1; m->map_stats[1] = n_alive; m->map_stats[2] = up_points; m->map_stats[3] = up_ranges;
  m->map_stats[4] += up_points; m->map_stats[5] += up_ranges;
  *out = g;
  return KH_OK;
}

int kh_mapper_map_stats(const kh_mapper * m, int64_t out[6])
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  std::copy(m->map_stats, m->map_stats + 6, out);
  return KH_OK;
}

}  // extern "C"
