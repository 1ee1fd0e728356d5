// The host rules of kh_map_visibility_*  without a device: the reach of a laser and the bytes of a pose's
// bitmap, every refusal and their order, whether a view is another view of the handle's window.  Needs no HIP header:
// tests/map_visibility_plan_check.cpp drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cmath>
#include <cstdint>

#include "map_localize_plan.hpp"     // fit_inputs_check: the laser and pose rules of every walk on a view
#include "occupancy_device.hpp"      // map_view_refusal

namespace kh
{
constexpr int32_t kVisMaxReach = 511;                // cells: a bitmap of side 1023 fits one workgroup's LDS
constexpr int32_t kVisMaxPoses = 65536, kVisMaxPicks = 4096;
constexpr int64_t kVisMaxBeams = 1ll << 24;          // n * n_beams of one call: its far points are one table of 16 bytes a beam
constexpr int32_t kVisCounters = 9;                  // a record's fields but gain, in the record's order
constexpr int32_t kVisReduceWords = 4 * kVisCounters;          // the four waves' partial sums, behind the bitmap
constexpr int32_t kVisMaxLdsBytes = 160 * 1024;      // what a gfx950 workgroup may declare

// reach = floor(range_threshold * scale) + 2: both cells of a beam are rounded, the far point lies range_threshold from the sensor.
// The caller has passed fit_laser_ok (range_threshold * scale + 2 <= 2^20).
inline int32_t vis_reach(double range_threshold, double scale) {return static_cast<int32_t>(std::floor(range_threshold * scale)) + 2;}
inline int32_t vis_side(int32_t reach) {return 2 * reach + 1;}
// one bit per cell of the (2 reach + 1)^2 square around the sensor cell, in whole 32-bit words
inline int32_t vis_bitmap_words(int32_t reach) {return static_cast<int32_t>((static_cast<int64_t>(vis_side(reach)) * vis_side(reach) + 31) / 32);}
inline int32_t vis_bitmap_bytes(int32_t reach) {return 4 * vis_bitmap_words(reach);}
inline int32_t vis_lds_bytes(int32_t reach) {return vis_bitmap_bytes(reach) + 4 * kVisReduceWords;}
static_assert(4 * ((1023ll * 1023 + 31) / 32) + 4 * kVisReduceWords <= kVisMaxLdsBytes, "the largest bitmap and the reduction's words fit");
static_assert(1023ull * 1023 * 765 < (1ull << 32), "gain cannot overflow");
// the words of the covered mask: one bit per window cell, bit index row * width + column
inline int64_t vis_mask_words(int32_t width, int32_t height) {return (static_cast<int64_t>(width) * height + 31) / 32;}

// what kh_map_visibility_create refuses before a device is looked for, in this order
enum : int32_t {kVisOk = 0, kVisNull = 1, kVisBadView = 2, kVisBadLaser = 3, kVisBadBudget = 4, kVisBadWeights = 5, kVisTooFar = 6};
inline int32_t vis_create_check(const kh_map_view * view, const kh_laser * laser, const kh_visibility_params * p, const void * out, int32_t * reach)
{
  if (!view || !laser || !p || !out) {return kVisNull;}
  if (map_view_refusal(view) != kViewOk) {return kVisBadView;}
  if (laser->n_beams < 1 || fit_inputs_check(laser->range_threshold, laser->minimum_range, laser->maximum_range, laser->minimum_angle,
      laser->angular_resolution, 0, nullptr, view->anchor[0], view->anchor[1], view->scale).failed) {return kVisBadLaser;}
  if (p->max_unknown < -1) {return kVisBadBudget;}
  const int32_t w[3] = {p->w_unknown, p->w_free, p->w_occupied};
  for (int32_t k = 0; k < 3; ++k) {
    if (w[k] < 0 || w[k] > 255) {return kVisBadWeights;}
  }
  if (w[0] == 0 && w[1] == 0 && w[2] == 0) {return kVisBadWeights;}
  const int32_t r = vis_reach(laser->range_threshold, view->scale);
  if (r > kVisMaxReach) {return kVisTooFar;}
  *reach = r;
  return kVisOk;
}

// what a call that takes poses refuses before a device is looked for, in this order (select = false: k and min_gain are not read);
// *bad_pose takes the refused pose's index
enum : int32_t {kVisCallOk = 0, kVisCallNull = 1, kVisCallCount = 2, kVisCallPose = 3, kVisCallPicks = 4, kVisCallMinGain = 5, kVisCallBeams = 6};
inline int32_t vis_call_check(bool nulls, int32_t n, const double * poses, double ax, double ay, double scale, int32_t n_beams, bool select, int32_t k,
  uint32_t min_gain, int32_t * bad_pose)
{
  if (nulls || !poses) {return kVisCallNull;}
  if (n < 1 || n > kVisMaxPoses) {return kVisCallCount;}
  for (int32_t i = 0; i < n; ++i) {
    if (!fit_pose_ok(poses + 3 * static_cast<size_t>(i), ax, ay, scale)) {*bad_pose = i; return kVisCallPose;}
  }
  if (select && (k < 1 || k > (n < kVisMaxPicks ? n : kVisMaxPicks))) {return kVisCallPicks;}
  if (select && min_gain < 1u) {return kVisCallMinGain;}
  if (static_cast<int64_t>(n) * n_beams > kVisMaxBeams) {return kVisCallBeams;}
  return kVisCallOk;
}

// is `b` another view of a's window and lattice on a's device (kh_map_visibility_set_map)?  The stride and the cells may differ.
inline bool vis_same_window(const kh_map_view & a, const kh_map_view & b)
{
  return a.ox == b.ox && a.oy == b.oy && a.width == b.width && a.height == b.height && a.anchor[0] == b.anchor[0] && a.anchor[1] == b.anchor[1] &&
         a.scale == b.scale && a.device == b.device;
}
}  // namespace kh
