// The host rules of kh_map_field_update and of the live binding without a device: the clip of the caller's
// rectangle, the regions an update recomputes from the box of changed obstacles, the bands of the column pass, the same-lattice test
// with the order of its refusals, the limits of a new window, and when an update is a rebuild.  Needs no HIP header:
// tests/map_field_update_plan_check.cpp drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "live_map_plan.hpp"         // Rect
#include "map_field_plan.hpp"

namespace kh
{
constexpr int32_t kMinBandRows = 8;

// ---- rectangles: window columns and rows, [0, width) x [0, height) ----
inline Rect field_window_rect(int32_t width, int32_t height) {return Rect{0, 0, width, height};}

// the caller's rectangle (x, y, w, h in lattice cells; nullptr: the whole window) as window columns and rows, clipped to the window
inline Rect update_clip(const int32_t * rect, int32_t ox, int32_t oy, int32_t width, int32_t height)
{
  const Rect window = field_window_rect(width, height);
  if (!rect) {return window;}
  if (rect[2] <= 0 || rect[3] <= 0) {return Rect{};}
  const int64_t x0 = static_cast<int64_t>(rect[0]) - ox, y0 = static_cast<int64_t>(rect[1]) - oy;
  return Rect{x0, y0, x0 + rect[2], y0 + rect[3]}.clip(window);
}

// r grown by `by` cells on the sides named, clipped to the window
inline Rect grown(const Rect & r, int64_t by_x, int64_t by_y, const Rect & window)
{
  if (r.empty()) {return Rect{};}
  return Rect{r.x0 - by_x, r.y0 - by_y, r.x1 + by_x, r.y1 + by_y}.clip(window);
}

// k_field_changed's inclusive box (x0, y0, x1, y1), or its initial value (none), as a rectangle
inline Rect changed_box(const int32_t * w) {return w[0] > w[2] || w[1] > w[3] ? Rect{} : Rect{w[0], w[1], static_cast<int64_t>(w[2]) + 1, static_cast<int64_t>(w[3]) + 1};}

// What an update of a capped field recomputes from C, the box of the cells whose obstacle-ness changed (inside the window):
//   values    V = C grown by R: the values that can change (k_field_rows_region's cells)
//   columns   the columns of C on rows C.y grown by R: the column distances that can change (k_field_columns_band's rectangle)
//   reads     the cell states the column pass reads: the columns of C on rows C.y grown by 2R
//   staged    the column distances the row pass reads: V.x grown by R on the rows of V
struct UpdateRegions {Rect values, columns, reads, staged;};
inline UpdateRegions update_regions(const Rect & c, int32_t radius, int32_t width, int32_t height)
{
  const Rect window = field_window_rect(width, height);
  UpdateRegions u;
  u.values = grown(c, radius, radius, window);
  u.columns = grown(c, 0, radius, window);
  u.reads = grown(c, 0, 2 * static_cast<int64_t>(radius), window);
  u.staged = grown(u.values, radius, 0, window);
  return u;
}

// ---- the bands of the column pass ----
// The height of a band: a thread's sweeps cost (band + 2R) rows for `band` useful ones, and a band is a wave's worth of latency-bound
// work, so bands are as short as keeps that ratio bounded: max(R, 8) rows -- at most three rows walked per row written -- or the
// forced height, and never more than the rows there are.
inline int32_t band_rows(int32_t radius, int64_t rows, int32_t forced)
{
  const int64_t want = forced > 0 ? forced : std::max(radius, kMinBandRows);
  return static_cast<int32_t>(std::max<int64_t>(1, std::min(want, rows)));
}
inline int64_t band_count(int64_t rows, int32_t band) {return rows <= 0 ? 0 : (rows + band - 1) / band;}

// ---- the lattice ----
// a view is on the field's lattice when anchor and scale are equal BIT FOR BIT and the device is the same; the first difference, in
// this order, is the refusal
enum : int32_t {kLatticeSame = 0, kLatticeAnchorX = 1, kLatticeAnchorY = 2, kLatticeScale = 3, kLatticeDevice = 4};
inline int32_t lattice_check(const double field_anchor[2], double field_scale, int32_t field_device, const double anchor[2], double scale, int32_t device)
{
  if (std::memcmp(&field_anchor[0], &anchor[0], sizeof(double)) != 0) {return kLatticeAnchorX;}
  if (std::memcmp(&field_anchor[1], &anchor[1], sizeof(double)) != 0) {return kLatticeAnchorY;}
  if (std::memcmp(&field_scale, &scale, sizeof(double)) != 0) {return kLatticeScale;}
  return field_device == device ? kLatticeSame : kLatticeDevice;
}

// the limits of kh_map_field_create on a new window of a field whose R is known: field_check's codes
inline int32_t update_window_check(int32_t width, int32_t height, int32_t radius)
{
  if (width > kMaxFieldSide || height > kMaxFieldSide) {return kFieldSideTooLong;}
  if (static_cast<int64_t>(width) * height > kMaxFieldCells) {return kFieldTooManyCells;}
  if (radius == 0 && (width > kMaxUncappedSide || height > kMaxUncappedSide)) {return kFieldUncappedTooLong;}
  return kFieldOk;
}

// ---- when an update recomputes the whole window ----
enum : int32_t {kUpdateRegion = 0, kUpdateRelayout = 1, kUpdateNoColumns = 2, kUpdateUncapped = 3, kUpdateAfterFailure = 4};
inline int32_t update_kind(bool same_window, bool has_columns, int32_t radius, bool failed_before)
{
  if (!same_window) {return kUpdateRelayout;}
  if (!has_columns) {return kUpdateNoColumns;}
  if (radius == 0) {return kUpdateUncapped;}
  return failed_before ? kUpdateAfterFailure : kUpdateRegion;
}
}  // namespace kh
