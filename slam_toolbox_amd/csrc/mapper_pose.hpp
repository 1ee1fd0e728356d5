// The reference's pose arithmetic as the mapper needs it, in the reference's operation order (the library is built with
// -ffp-contract=off; the solver log is compared with the reference's at 17 digits): Karto.h LocalizedRangeScan::Update :5644-5704,
// GetSensorAt / GetCorrectedAt :5566-5586, Transform :2946-3041, Matrix3::FromAxisAngle :2482-2511; Math.h NormalizeAngle :181-202.
// Scope: one laser (mounted anywhere on the robot: kh_laser::offset_*, Karto.h:5566-5586).
// Included through mapper_private.hpp only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace kh
{
namespace mapper
{
// cos and sin of ONE angle, the way the reference's Release build computes them: GCC (-O1 and up) merges a cos(a) / sin(a)
// pair into one sincos(a) call, and glibc's sincos is NOT bit-identical to its cos and sin everywhere (a = 0.11462314399891493:
// cos(a) = 0.9934379567501339, sincos(a) gives 0.993437956750134).  Every place where the reference takes both of the same
// angle goes through here, so that the library does not depend on whether ITS compiler merges the pair (clang does not).
inline void ref_sincos(double a, double * s, double * c) {::sincos(a, s, c);}
constexpr double kTolerance = 1e-06;                  // KT_TOLERANCE, Math.h:41
constexpr double kPi = 3.14159265358979323846;        // Math.h:31
constexpr double k2Pi = 6.28318530717958647692;       // Math.h:32

inline double normalize_angle(double angle)           // math::NormalizeAngle, Math.h:181-202
{
  while (angle < -kPi) {
    if (angle < -k2Pi) {angle += static_cast<uint32_t>(angle / -k2Pi) * k2Pi;} else {angle += k2Pi;}
  }
  while (angle > kPi) {
    if (angle > k2Pi) {angle -= static_cast<uint32_t>(angle / k2Pi) * k2Pi;} else {angle -= k2Pi;}
  }
  return angle;
}

struct Pose {double x = 0.0, y = 0.0, h = 0.0;};
inline bool same_pose(const Pose & a, const Pose & b) {return a.x == b.x && a.y == b.y && a.h == b.h;}   // Karto.h:2180-2183
inline Pose to_pose(const double * a) {Pose p; p.x = a[0]; p.y = a[1]; p.h = a[2]; return p;}
inline void put_pose(const Pose & p, double * a) {a[0] = p.x; a[1] = p.y; a[2] = p.h;}

struct Mat3
{
  double m[3][3];
  void identity() {std::memset(m, 0, sizeof(m)); m[0][0] = m[1][1] = m[2][2] = 1.0;}
  // Rodrigues' rotation about a unit axis, in the operation order of Matrix3::FromAxisAngle (Karto.h:2482-2511) -- the solver log
  // is compared with the reference's at 17 digits: diagonal a_i a_i (1 - c) + c; off-diagonal (a_i a_j)(1 - c) -+ a_k s, "+" where
  // (i, j, k) is an odd permutation
  void from_axis_angle(double ax, double ay, double az, double angle)
  {
    const double axis[3] = {ax, ay, az};
    double s, c;
    ref_sincos(angle, &s, &c);
    const double versine = 1.0 - c;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) {
        if (i == j) {m[i][i] = axis[i] * axis[i] * versine + c; continue;}
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const double symmetric = axis[lo] * axis[hi] * versine, skew = axis[3 - i - j] * s;
        m[i][j] = ((j - i + 3) % 3 == 2) ? symmetric + skew : symmetric - skew;
      }
    }
  }
  Pose mul(const Pose & p) const                                          // Matrix3 * Pose2, Karto.h:2654-2666
  {
    Pose r;
    r.x = m[0][0] * p.x + m[0][1] * p.y + m[0][2] * p.h;
    r.y = m[1][0] * p.x + m[1][1] * p.y + m[1][2] * p.h;
    r.h = m[2][0] * p.x + m[2][1] * p.y + m[2][2] * p.h;
    return r;
  }
};

// karto::Transform(rPose1, rPose2).TransformPose(src), Karto.h:2946-3024
inline Pose transform_pose(const Pose & p1, const Pose & p2, const Pose & src)
{
  Mat3 rot;
  Pose t;
  if (same_pose(p1, p2)) {
    rot.identity();
  } else {
    rot.from_axis_angle(0, 0, 1, p2.h - p1.h);
    if (p1.x != 0.0 || p1.y != 0.0) {
      const Pose r = rot.mul(p1);
      t.x = p2.x - r.x; t.y = p2.y - r.y;
    } else {
      t.x = p2.x; t.y = p2.y;
    }
    t.h = p2.h - p1.h;
  }
  const Pose r = rot.mul(src);
  Pose out;
  out.x = t.x + r.x; out.y = t.y + r.y;
  out.h = normalize_angle(src.h + t.h);
  return out;
}

// One processed scan: what LocalizedRangeScan holds (zero mount offset: the sensor pose is the corrected pose with its
// heading normalised, GetSensorAt / GetCorrectedAt Karto.h:5566-5586)
struct MScan
{
  int32_t id = -1;
  double time = 0.0;
  Pose odometric, corrected;
  std::vector<double> ranges;
  std::vector<double> points;        // unfiltered point readings, x0 y0 x1 y1 ...
  std::vector<double> filtered;      // point readings with the range inside [minimum range, range threshold]
  std::vector<uint64_t> filter_mask; // bit i: reading i is one of `filtered` (the node-decay kernel reads `points` in HBM through it)
  double score = 1.0;                // Vertex::GetScore (Mapper.h: vertices start at 1.0)
  double barycenter[2] = {0.0, 0.0};
  double bbox[4] = {0.0, 0.0, 0.0, 0.0};   // min x, min y, max x, max y of the sensor position and the filtered readings
  int32_t n_filtered = 0;
  // the unfiltered readings once more, in HBM: as a base scan of a match the scan is read where it lies (kh_scan::
  // device_points_xy).  Uploaded on first use and again after the pose has moved (update_scan marks it stale).
  static constexpr int kMaxDeviceSlots = 16;
  double * d_points[kMaxDeviceSlots] = {};       // one copy per distinct device of the mapper (slot 0 = the mapper's own device)
  uint16_t d_fresh = 0;                          // bit k: the copy in slot k holds the current points
  // the range readings in HBM on the mapper's own device (kh_mapper_build_map reads them there): they never change after the scan
  // is made, so they are uploaded once
  double * d_ranges = nullptr;
  bool d_ranges_fresh = false;
  Pose sensor;                                   // GetSensorAt(corrected), refreshed by update_scan (every write of `corrected` is followed by one)
  Pose sensor_pose() const {return sensor;}
  MScan() = default;
  MScan(const MScan &) = delete;
  MScan & operator=(const MScan &) = delete;
  // d_points is a slot of the mapper's device slabs (take_slot / remove_node / kh_mapper_destroy), not owned here
};

struct Laser
{
  int32_t n = 0;
  double min_angle = 0, ang_res = 0, min_range = 0, max_range = 0, range_threshold = 0;
  Pose offset;                                   // LaserRangeFinder::GetOffsetPose: the sensor in the robot's frame
};

// LocalizedRangeScan::GetSensorAt (Karto.h:5566-5569): Transform(robot pose).TransformPose(offset pose)
inline Pose sensor_at(const Laser & L, const Pose & robot) {return transform_pose(Pose(), robot, L.offset);}

// LocalizedRangeScan::GetCorrectedAt (Karto.h:5576-5588): the robot pose that puts the sensor at `sensor`
inline Pose corrected_at(const Laser & L, const Pose & sensor)
{
  const double offset_length = std::sqrt(L.offset.x * L.offset.x + L.offset.y * L.offset.y);       // Vector2::Length
  const double offset_heading = L.offset.h;
  const double angle_offset = std::atan2(L.offset.y, L.offset.x);
  const double heading = normalize_angle(sensor.h);
  double sin_w, cos_w;
  ref_sincos(heading + angle_offset - offset_heading, &sin_w, &cos_w);
  Pose robot;                                      // Pose2::operator-: positions subtract, the heading difference is normalised
  robot.x = sensor.x - offset_length * cos_w;
  robot.y = sensor.y - offset_length * sin_w;
  robot.h = normalize_angle(sensor.h - offset_heading);
  return robot;
}

// LocalizedRangeScan::Update, Karto.h:5644-5704
inline void update_scan(MScan & s, const Laser & L)
{
  s.sensor = sensor_at(L, s.corrected);
  const Pose sp = s.sensor;
  s.points.resize(2 * static_cast<size_t>(L.n));
  s.d_fresh = 0;
  s.filtered.clear();
  s.filter_mask.assign((static_cast<size_t>(L.n) + 63) / 64, 0);
  double sum_x = 0.0, sum_y = 0.0;
  int32_t n_filtered = 0;
  double bb[4] = {sp.x, sp.y, sp.x, sp.y};
  for (int32_t i = 0; i < L.n; ++i) {
    const double r = s.ranges[i];
    const double angle = sp.h + L.min_angle + static_cast<uint32_t>(i) * L.ang_res;
    double sin_a, cos_a;
    ref_sincos(angle, &sin_a, &cos_a);
    const double px = sp.x + (r * cos_a);
    const double py = sp.y + (r * sin_a);
    s.points[2 * i] = px; s.points[2 * i + 1] = py;
    if (r >= L.min_range && r <= L.range_threshold) {          // math::InRange
      sum_x += px; sum_y += py; ++n_filtered;
      s.filtered.push_back(px); s.filtered.push_back(py);
      s.filter_mask[static_cast<size_t>(i) >> 6] |= 1ull << (i & 63);
      bb[0] = std::min(bb[0], px); bb[1] = std::min(bb[1], py); bb[2] = std::max(bb[2], px); bb[3] = std::max(bb[3], py);
    }
  }
  const double n_points = static_cast<double>(n_filtered);
  if (n_points != 0.0) {
    s.barycenter[0] = sum_x / n_points; s.barycenter[1] = sum_y / n_points;
  } else {
    s.barycenter[0] = sp.x; s.barycenter[1] = sp.y;
  }
  s.n_filtered = n_filtered;
  std::copy(bb, bb + 4, s.bbox);
}

}  // namespace mapper
}  // namespace kh
