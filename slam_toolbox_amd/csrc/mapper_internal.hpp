// What mapper_views.cpp shows of a mapper to the session merger (merge.cpp) and the live map (live_map.cpp).  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/karto_hip.h"
#include "occupancy_device.hpp"

namespace kh
{
// one scan still in a mapper's map; `points` is the mapper's own host memory (`ranges` too; valid until its next process / remove / destroy)
struct ScanView
{
  int32_t id;
  const double * points;        // 2 * n_beams unfiltered point readings
  const double * ranges;        // n_beams range readings
  double corrected[3], odometric[3];
  double barycenter[3];         // GetBarycenterPose: heading 0, or the sensor pose when no reading is in range
  double bbox[4];               // min x, min y, max x, max y (LocalizedRangeScan::Update, Karto.h:5694-5700)
};

int32_t mapper_device(const kh_mapper * m);
kh_laser mapper_laser(const kh_mapper * m);
void mapper_alive_scans(const kh_mapper * m, std::vector<ScanView> & out);        // id order
// makes every scan still in the map resident on the mapper's device (uploads queued on `stream`) and emits one record per scan in
// id order: where its readings lie on the device, and its sensor position
int mapper_resident_table(kh_mapper * m, void * stream, const char * who, std::vector<ResidentScan> & table, int64_t * up_points, int64_t * up_ranges);
// the same for a subset: ids = NULL is every scan still in the map, otherwise the n_ids scans named, in the order given (a scan
// that is not in the map is KH_ERR_NOT_FOUND)
int mapper_resident_table_of(kh_mapper * m, void * stream, const char * who, const int32_t * ids, size_t n_ids, std::vector<ResidentScan> & table,
  int64_t * up_points, int64_t * up_ranges);
// what the live map (live_map.cpp) classifies a scan by (SensorView, occupancy_device.hpp)
void mapper_sensor_poses(const kh_mapper * m, std::vector<SensorView> & out);     // id order
void laser_sensor_at(const kh_laser & laser, const double robot[3], double sensor[3]);   // LocalizedRangeScan::GetSensorAt, Karto.h:5566-5569
double karto_normalize_angle(double angle);                                              // math::NormalizeAngle, Math.h:181-202
}  // namespace kh
