// The host rules of kh_map_regions_*  without a device: Rc, every refusal and their order, the tile grid and
// the seam count, the compaction's units, the centroid cell, the record's doubles.  Needs no HIP header:
// tests/map_regions_plan_check.cpp drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cmath>
#include <cstdint>

#include "map_field_plan.hpp"        // field_radius: R's rule is Rc's

namespace kh
{
constexpr int32_t kRegionTileW = 64, kRegionTileH = 16;      // the project's tiles: a tile row is one wave's ballot
constexpr int32_t kMaxRegionCount = 1 << 20;                 // max_regions, max_frontiers
// the device's counters, in the order the kernels keep them (uint64 each)
enum : int32_t {kRegionTraversable = 0, kRegionFrontierCells = 1, kRegionTotal = 2 /* + which */, kRegionPassing = 4 /* + which */, kRegionError = 6,
                kRegionCounters = 8};

// what kh_map_regions_create takes of its parameters at the field's scale before a device is looked for, in this order
enum : int32_t {kRegionsOk = 0, kRegionsBadClearance = 1, kRegionsClearanceTooFar = 2, kRegionsBadConnectivity = 3, kRegionsBadMinimum = 4,
                kRegionsBadMaximum = 5};
inline int32_t regions_check(const kh_map_regions_params & p, double scale, int32_t * rc)
{
  if (!std::isfinite(p.min_clearance) || p.min_clearance < 0.0) {return kRegionsBadClearance;}
  const int32_t r = field_radius(p.min_clearance, scale);
  if (r < 0) {return kRegionsClearanceTooFar;}
  if (p.connectivity != 4 && p.connectivity != 8) {return kRegionsBadConnectivity;}
  if (p.min_region_cells < 1 || p.min_frontier_cells < 1) {return kRegionsBadMinimum;}
  if (p.max_regions < 1 || p.max_regions > kMaxRegionCount || p.max_frontiers < 1 || p.max_frontiers > kMaxRegionCount) {return kRegionsBadMaximum;}
  *rc = r;
  return kRegionsOk;
}
// a field that does not reach as far as the threshold asks (the costs call's refusal)
inline bool regions_reach_ok(int32_t field_radius_cells, int32_t rc) {return !(field_radius_cells > 0 && field_radius_cells < rc);}

// the tiles of a window and the cells that look across their borders: every row that begins a tile but the first looks up, every
// column that begins a tile but the first looks left
struct RegionGrid
{
  int32_t tiles_x, tiles_y;
  int64_t seam_threads;        // (tiles_y - 1) * width + (tiles_x - 1) * height
  int64_t units;               // runs of 64 consecutive window indices: the compaction's units
};
inline RegionGrid region_grid(int32_t width, int32_t height)
{
  RegionGrid g;
  g.tiles_x = (width + kRegionTileW - 1) / kRegionTileW; g.tiles_y = (height + kRegionTileH - 1) / kRegionTileH;
  g.seam_threads = static_cast<int64_t>(g.tiles_y - 1) * width + static_cast<int64_t>(g.tiles_x - 1) * height;
  g.units = (static_cast<int64_t>(width) * height + 63) / 64;
  return g;
}

// one coordinate of the centroid cell: round-half-up of sum / n in integers (n >= 1; 2 sum + n < 2^64 for every window)
#if defined(__HIP__)
__host__ __device__
#endif
inline uint64_t centroid_cell(uint64_t sum, uint64_t n) {return (2u * sum + n) / (2u * n);}

// the record's doubles, operation by operation
inline double region_centroid(double anchor, int32_t o, uint64_t sum, uint32_t n, double scale)
{
  return anchor + (static_cast<double>(o) + static_cast<double>(sum) / static_cast<double>(n)) / scale;
}
inline double region_cell_world(double anchor, int32_t o, int32_t a, double scale) {return anchor + static_cast<double>(o + a) / scale;}
}  // namespace kh
