// The host rules of kh_map_merge_*  without a device: the argument check, the footprint and its sample offsets,
// the output window with its refusals, the derived agreement.  Needs no HIP header: tests/map_merge_plan_check.cpp drives it on the
// CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "map_align_plan.hpp"     // AlignRigid, align_inverse: tests/merge_rule.py's arithmetic

namespace kh
{
constexpr int32_t kMaxMergeFootprint = 4;             // samples per axis of one output cell
constexpr double kMaxMergeCorner = 1073741824.0;      // |target-lattice index| of a carried corner of the moving map's known box (2^30)
constexpr int64_t kMaxMergeSide = 32768;              // cells of an output side
constexpr int64_t kMaxMergeCells = 1ll << 28;         // cells of an output
// the six counters of a merge, in this order (kh_map_merge_stats' first six uint64 fields)
enum : int32_t {kMergeTargetOnly = 0, kMergeMovingOnly = 1, kMergeAgreeFree = 2, kMergeAgreeOccupied = 3, kMergeMovingOccupied = 4, kMergeMovingFree = 5,
  kMergeCounters = 6};

// what kh_map_merge_create takes of its parameters before a device is looked for
inline bool merge_params_ok(const kh_map_merge_params & p)
{
  return std::isfinite(p.correction[0]) && std::isfinite(p.correction[1]) && std::isfinite(p.correction[2]) && p.footprint >= 0 &&
         p.footprint <= kMaxMergeFootprint && p.conflict >= KH_MERGE_CONFLICT_TARGET && p.conflict <= KH_MERGE_CONFLICT_UNKNOWN && p.grow >= 0 && p.grow <= 1;
}

// min(4, max(1, ceil(scale_m / scale_t))): 1 unless the moving map is finer than the target
inline int32_t merge_default_footprint(double scale_m, double scale_t)
{
  const double ratio = std::ceil(scale_m / scale_t);
  return ratio >= kMaxMergeFootprint ? kMaxMergeFootprint : ratio >= 1.0 ? static_cast<int32_t>(ratio) : 1;
}

// the offsets of the n sample points of one axis from the cell's centre: ((2 k + 1 - n) / (2.0 n)) / scale_t; exactly 0 for n = 1
inline void merge_sample_offsets(int32_t n, double scale_t, double d[kMaxMergeFootprint])
{
  for (int32_t k = 0; k < kMaxMergeFootprint; ++k) {
    d[k] = k < n ? (static_cast<double>(2 * k + 1 - n) / (2.0 * static_cast<double>(n))) / scale_t : 0.0;
  }
}

// the output window: lattice cells [ox, ox + width) x [oy, oy + height) of the target's lattice, row stride ws as kh_occupancy's
struct MergeWindow
{
  int32_t ox = 0, oy = 0, width = 0, height = 0, ws = 0;
};
enum : int32_t {kMergeWindowOk = 0, kMergeCornerTooFar = 1, kMergeSideTooLong = 2, kMergeTooManyCells = 3};

// grow 0: the target's window.  grow 1: its union with the carried box of the moving map's known cells box = (i0, j0, i1, j1), none
// where i1 < i0 -- the box's corner points anchor_m + idx / scale_m pushed outward by 0.5 / scale_m, carried by `correction`, rounded
// to target-lattice cells (occ_cell's operations), min / max over the four, one cell of padding on every side.
inline int32_t merge_window(const kh_map_view & target, const kh_map_view & moving, const int32_t box[4], const double correction[3], int32_t grow,
  MergeWindow * out)
{
  int64_t x0 = target.ox, y0 = target.oy, x1 = static_cast<int64_t>(target.ox) + target.width, y1 = static_cast<int64_t>(target.oy) + target.height;
  if (grow && box[2] >= box[0]) {
    const AlignRigid carry(correction[0], correction[1], correction[2]);
    const double half = 0.5 / moving.scale;
    const double xs[2] = {(moving.anchor[0] + static_cast<double>(box[0]) / moving.scale) - half, (moving.anchor[0] + static_cast<double>(box[2]) / moving.scale) + half};
    const double ys[2] = {(moving.anchor[1] + static_cast<double>(box[1]) / moving.scale) - half, (moving.anchor[1] + static_cast<double>(box[3]) / moving.scale) + half};
    for (int32_t k = 0; k < 4; ++k) {
      const double x = xs[k & 1], y = ys[k >> 1];
      const double px = (carry.c * x - carry.s * y) + carry.x, py = (carry.s * x + carry.c * y) + carry.y;
      const double ci = round_half_away((px - target.anchor[0]) * target.scale), cj = round_half_away((py - target.anchor[1]) * target.scale);
      if (!(std::fabs(ci) <= kMaxMergeCorner && std::fabs(cj) <= kMaxMergeCorner)) {return kMergeCornerTooFar;}
      const int64_t i = static_cast<int64_t>(ci), j = static_cast<int64_t>(cj);
      x0 = std::min(x0, i - 1); y0 = std::min(y0, j - 1);
      x1 = std::max(x1, i + 2); y1 = std::max(y1, j + 2);
    }
  }
  const int64_t width = x1 - x0, height = y1 - y0;
  if (width > kMaxMergeSide || height > kMaxMergeSide) {return kMergeSideTooLong;}
  if (width * height > kMaxMergeCells) {return kMergeTooManyCells;}
  out->ox = static_cast<int32_t>(x0); out->oy = static_cast<int32_t>(y0);
  out->width = static_cast<int32_t>(width); out->height = static_cast<int32_t>(height); out->ws = (out->width + 7) & ~7;
  return kMergeWindowOk;
}

// overlap = the last four counters; agreement = (agree_free + agree_occupied) / overlap as doubles, 0.0 without overlap
inline uint64_t merge_overlap(const uint64_t c[kMergeCounters])
{
  return c[kMergeAgreeFree] + c[kMergeAgreeOccupied] + c[kMergeMovingOccupied] + c[kMergeMovingFree];
}
inline double merge_agreement(const uint64_t c[kMergeCounters])
{
  const uint64_t overlap = merge_overlap(c);
  return overlap ? static_cast<double>(c[kMergeAgreeFree] + c[kMergeAgreeOccupied]) / static_cast<double>(overlap) : 0.0;
}
}  // namespace kh
