// The host rules of the map change layer (kh_map_changes_*) without a device: the bound that keeps a counter of
// the layer from wrapping, and the argument checks of an observe and a diff call.  Needs no HIP header: tests/map_changes_plan_check.cpp
// drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cmath>
#include <cstdint>

#include "map_localize_plan.hpp"  // fit_inputs_check

namespace kh
{
constexpr int32_t kMaxEndTolerance = 4;               // cells: k_map_observe reads at most 9 x 9 cells around a beam's end
constexpr uint64_t kMaxChangeCount = 0xFFFFFFFFull;   // what a uint32 counter of the layer holds

// The bound: no cell of the layer holds more than it.  One scan adds at most 2 to a cell per beam (the line's visit and the hit's), so
// n_scans scans of n_beams beams add at most 2 * n_beams * n_scans; a decay shifts the bound as it shifts the cells.
// false = the call is refused: the bound would pass kMaxChangeCount.  *after is written only for a call that is taken.
inline bool changes_bound_after(uint64_t bound, int32_t n_scans, int32_t n_beams, uint64_t * after)
{
  if (n_scans < 1 || n_beams < 1 || bound > kMaxChangeCount) {return false;}
  const uint64_t gain = 2ull * static_cast<uint64_t>(n_beams) * static_cast<uint64_t>(n_scans);      // below 2^63: both are int32
  if (gain > kMaxChangeCount - bound) {return false;}
  *after = bound + gain;
  return true;
}
inline bool changes_shift_ok(int32_t shift) {return shift >= 1 && shift <= 31;}
inline uint64_t changes_bound_decayed(uint64_t bound, int32_t shift) {return bound >> shift;}

// what of an observe call can be judged without the handle: NULL pointers, the counts, the tolerance, numbers that are none
inline bool changes_observe_args_ok(const kh_laser * laser, int32_t n_scans, const double * ranges, const double * sensor_poses, int32_t end_tolerance)
{
  if (!laser || !ranges || !sensor_poses || n_scans < 1 || laser->n_beams < 1 || end_tolerance < 0 || end_tolerance > kMaxEndTolerance) {return false;}
  if (!std::isfinite(laser->range_threshold) || !(laser->range_threshold > 0.0) || std::isnan(laser->minimum_range) ||
    std::isnan(laser->maximum_range) || !std::isfinite(laser->minimum_angle) || !std::isfinite(laser->angular_resolution))
  {
    return false;
  }
  for (int64_t k = 0; k < 3 * static_cast<int64_t>(n_scans); ++k) {
    if (!std::isfinite(sensor_poses[k])) {return false;}
  }
  return true;
}

// ... and what depends on the view: kh_map_fit's check of the walk length (fit_inputs_check)
inline FitInputs changes_observe_walk(const kh_laser & laser, int32_t n_scans, const double * sensor_poses, double ax, double ay, double scale)
{
  return fit_inputs_check(laser.range_threshold, laser.minimum_range, laser.maximum_range, laser.minimum_angle, laser.angular_resolution,
      static_cast<size_t>(n_scans), sensor_poses, ax, ay, scale);
}

inline bool changes_diff_args_ok(double occupancy_threshold, const int32_t * cells, int32_t cap, const void * out)
{
  return out && cap >= 0 && (cap == 0 || cells) && !std::isnan(occupancy_threshold);
}
}  // namespace kh
