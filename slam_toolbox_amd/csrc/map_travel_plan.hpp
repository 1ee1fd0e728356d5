// The host rules of kh_map_travel_*  without a device: Rc, Rt and q_max, the overflow bound, every refusal and
// their order, the tile grid and which neighbours a tile flags, the path buffer's size check.  Needs no HIP header:
// tests/map_travel_plan_check.cpp drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cmath>
#include <cstdint>

#include "map_field_plan.hpp"        // field_radius, inflation_radius_cells: R's rule is Rc's and Rt's

namespace kh
{
constexpr int32_t kTravelTileW = 64, kTravelTileH = 16;      // the project's tiles: a tile row is one wave's lanes
constexpr int32_t kTravelTileCells = kTravelTileW * kTravelTileH;
constexpr int32_t kMaxTravelGoals = 4096, kMaxTravelSnap = 16;
constexpr int32_t kMaxPathCells = 65536;
constexpr int64_t kMaxPathBuffer = 1ll << 24;                // n * max_cells
constexpr int32_t kMaxRoundsPerCheck = 64, kDefaultRoundsPerCheck = 16;   // the default: DESIGN.md 7r's sweep
constexpr uint32_t kTravelFar = 0xFFFFFFFFu;
// the device's counters, in the order the kernels keep them (uint64 each)
enum : int32_t {kTravelTraversable = 0, kTravelReached = 1, kTravelMaxValue = 2, kTravelRuns = 3, kTravelError = 4, kTravelCounters = 8};

// the directions of a step, in the rule's order, and their lengths
#if defined(__HIP__)
#define KH_TRAVEL_BOTH __host__ __device__
#else
#define KH_TRAVEL_BOTH
#endif
KH_TRAVEL_BOTH inline int32_t travel_di(int32_t n) {return n == 0 || n == 4 || n == 7 ? 1 : n == 1 || n == 3 ? 0 : -1;}
KH_TRAVEL_BOTH inline int32_t travel_dj(int32_t n) {return n == 1 || n == 4 || n == 5 ? 1 : n == 0 || n == 2 ? 0 : -1;}
KH_TRAVEL_BOTH inline uint32_t travel_length(int32_t n) {return n < 4 ? 5u : 7u;}

// what kh_map_travel_create takes of its parameters at the field's scale before a device is looked for, in this order
enum : int32_t {kTravelOk = 0, kTravelBadConnectivity = 1, kTravelBadCutCorners = 2, kTravelBadNeutral = 3, kTravelBadWeight = 4, kTravelBadSnap = 5,
                kTravelBadClearance = 6, kTravelClearanceTooFar = 7, kTravelBadInflation = 8};
inline int32_t travel_check(const kh_map_travel_params & p, double scale, int32_t * rc, int32_t * rt)
{
  if (p.connectivity != 4 && p.connectivity != 8) {return kTravelBadConnectivity;}
  if (p.cut_corners < 0 || p.cut_corners > 1) {return kTravelBadCutCorners;}
  if (p.neutral_cost < 1 || p.neutral_cost > 255) {return kTravelBadNeutral;}
  if (p.cost_weight < 0 || p.cost_weight > 255) {return kTravelBadWeight;}
  if (p.goal_snap_cells < 0 || p.goal_snap_cells > kMaxTravelSnap) {return kTravelBadSnap;}
  if (!std::isfinite(p.min_clearance) || p.min_clearance < 0.0) {return kTravelBadClearance;}
  const int32_t c = field_radius(p.min_clearance, scale);
  if (c < 0) {return kTravelClearanceTooFar;}
  const int32_t t = inflation_radius_cells(p.inflation, scale);
  if (t < 0) {return kTravelBadInflation;}
  *rc = c; *rt = t;
  return kTravelOk;
}

// the largest weight the parameters can give a cell: the table's largest entry a free cell can hold is 253
inline uint32_t travel_q_max(int32_t neutral_cost, int32_t cost_weight)
{
  return static_cast<uint32_t>(neutral_cost) + ((static_cast<uint32_t>(cost_weight) * 253u) >> 4);
}
KH_TRAVEL_BOTH inline uint32_t travel_weight(uint32_t neutral_cost, uint32_t cost_weight, uint32_t c) {return neutral_cost + ((cost_weight * c) >> 4);}

// what is looked at once the field is known, in this order
enum : int32_t {kTravelFieldOk = 0, kTravelShortOfClearance = 1, kTravelShortOfInflation = 2, kTravelOverflow = 3};
// a simple path has fewer steps than the window has cells, a step costs at most Lmax * q_max: every value stays below KH_TRAVEL_FAR
inline bool travel_overflows(int64_t width, int64_t height, int32_t connectivity, uint32_t q_max)
{
  const uint64_t per_cell = (connectivity == 8 ? 7ull : 5ull) * q_max;           // <= 7 * 4287
  return static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > 0xFFFFFFFEull / per_cell;      // width * height * per_cell > 0xFFFFFFFE
}
inline int32_t travel_field_check(const kh_map_travel_params & p, int32_t rc, int32_t rt, int32_t field_radius_cells, int64_t width, int64_t height)
{
  if (field_radius_cells > 0 && field_radius_cells < rc) {return kTravelShortOfClearance;}
  if (p.cost_weight > 0 && field_radius_cells > 0 && field_radius_cells < rt) {return kTravelShortOfInflation;}
  if (travel_overflows(width, height, p.connectivity, travel_q_max(p.neutral_cost, p.cost_weight))) {return kTravelOverflow;}
  return kTravelFieldOk;
}

// the tiles of a window
struct TravelGrid {int32_t tiles_x, tiles_y; int64_t tiles;};
KH_TRAVEL_BOTH inline TravelGrid travel_grid(int32_t width, int32_t height)
{
  TravelGrid g;
  g.tiles_x = (width + kTravelTileW - 1) / kTravelTileW; g.tiles_y = (height + kTravelTileH - 1) / kTravelTileH;
  g.tiles = static_cast<int64_t>(g.tiles_x) * g.tiles_y;
  return g;
}

// The neighbours tile (tx, ty) flags, as a mask over the directions: bit n is the tile at (tx + di(n), ty + dj(n)), where the grid has
// one.  `lowered` holds, per direction, whether the tile lowered a cell that a cell of that neighbour can step to: bits 0 .. 3 a cell of
// the tile's right column, bottom row, left column, top row; bits 4 .. 7 its bottom-right, bottom-left, top-left, top-right corner
// cell.  Only a corner cell has a neighbour in a diagonal tile, and only under connectivity 8.
KH_TRAVEL_BOTH inline uint32_t travel_flagged(int32_t tx, int32_t ty, int32_t tiles_x, int32_t tiles_y, bool conn8, uint32_t lowered)
{
  uint32_t out = 0u;
  for (int32_t n = 0; n < (conn8 ? 8 : 4); ++n) {
    const int32_t x = tx + travel_di(n), y = ty + travel_dj(n);
    if (x >= 0 && x < tiles_x && y >= 0 && y < tiles_y && ((lowered >> n) & 1u)) {out |= 1u << n;}
  }
  return out;
}

// the arguments of kh_map_travel_paths that bound its buffer
inline bool travel_path_buffer_ok(int32_t n, int32_t max_cells)
{
  return n >= 1 && max_cells >= 1 && max_cells <= kMaxPathCells && static_cast<int64_t>(n) * max_cells <= kMaxPathBuffer;
}
inline bool travel_snap_ok(int32_t snap_cells) {return snap_cells >= 0 && snap_cells <= kMaxTravelSnap;}
}  // namespace kh
