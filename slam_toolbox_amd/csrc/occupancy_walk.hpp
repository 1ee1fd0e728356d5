// The device half of the occupancy module that its kernel files share (occupancy.hip, occupancy_live.hip, occupancy_map.hip,
// occupancy_changes.hip): the one statement of AddScan / RayTrace / TraceLine, the two kinds of cell index and the visitors built on
// them, the pieces of the (pose, run of 64 beams) work layout, UpdateCell and the nav values.  Device code only: included by .hip
// files, never by a HIP-free program (those include occupancy_device.hpp).  The reference's lines: occupancy.hip's header.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "occupancy_device.hpp"
#include "map_localize_plan.hpp"     // kMaxFitWalk

namespace kh
{
__device__ __forceinline__ double o_round(double v) {return v >= 0.0 ? floor(v + 0.5) : ceil(v - 0.5);}   // Math.h:87-90
__device__ __forceinline__ int32_t o_to_int(double v)
{
  if (!(v > -2147483649.0 && v < 2147483648.0)) {return INT32_MIN;}
  return (int32_t)v;
}

struct OccDev
{
  int32_t width, height, ws;
  double off_x, off_y, scale;
  uint32_t * pass;
  uint32_t * hits;
  uint8_t * cells;
};

// ---- the one statement of AddScan / RayTrace / TraceLine every trace kernel uses ----
// what AddScan (Karto.h:6148-6189) decides about one beam: whether it is traced at all, whether its end point counts as a hit, and
// the end point, clipped to the range threshold where the reading lies beyond it
struct Beam
{
  double px, py;
  bool kept, hit;
};
__device__ __forceinline__ Beam occ_gate(double r, double px, double py, double sx, double sy, double range_threshold, double min_range,
  double max_range)
{
  const bool valid_end = r < (range_threshold - 1e-06);                  // Karto.h:6167
  if (r <= min_range || r >= max_range || r != r) {return Beam{0.0, 0.0, false, false};}      // Karto.h:6169-6172
  if (r >= range_threshold) {                                           // Karto.h:6173-6180
    const double ratio = range_threshold / r;
    const double dx = px - sx, dy = py - sy;
    px = sx + ratio * dx; py = sy + ratio * dy;
  }
  return Beam{px, py, true, valid_end};
}

// CoordinateConverter::WorldToGrid (Karto.h:4421-4436, called at Karto.h:6208-6209) of one coordinate: origin = the grid's offset, or a
// live map's anchor
__device__ __forceinline__ int32_t occ_cell(double v, double origin, double scale) {return o_to_int(o_round((v - origin) * scale));}

// ---- where cell (cx, cy) of a walk lives: the two kinds of index, each stated once ----
struct CellAt
{
  int64_t wx, wy;                // column and row from the first cell, inside or not
  bool inside;
  int64_t k;                     // the cell's index in the arrays, if it is inside
};
// A whole grid: cell (0, 0) is the first; the guard is 32-bit.  (Kept apart from the window on purpose: the walk loops of the
// whole-grid trace kernels are a known instruction sequence, profiles/NOTES_r6.md section 8.)
__device__ __forceinline__ CellAt cell_at(const OccDev & g, int32_t cx, int32_t cy)
{
  return CellAt{cx, cy, cx >= 0 && cx < g.width && cy >= 0 && cy < g.height, cx + (int64_t)cy * g.ws};
}
// A window of the lattice (LiveWindow, MapWindow): cell (ox, oy) is the first.  64-bit: a logged cell is any int32, the window's
// origin too.  A live window holds every cell of every beam (coverage rule), there the bounds test is a guard.
template <typename Window>
__device__ __forceinline__ CellAt cell_at(const Window & g, int32_t cx, int32_t cy)
{
  const int64_t wx = (int64_t)cx - g.ox, wy = (int64_t)cy - g.oy;
  return CellAt{wx, wy, wx >= 0 && wx < g.width && wy >= 0 && wy < g.height, wx + wy * g.ws};
}

// ---- the visitors of a walk: add() is one visit of cell (cx, cy) -- and one hit, at a hit end -- if the cell exists ----
template <typename Where>
struct CountCells                // WRITE: a visit adds delta to the counters (1, or 0xFFFFFFFF = -1 where a live map takes a line back)
{
  const Where & g;
  uint32_t delta;
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    const CellAt at = cell_at(g, cx, cy);
    if (at.inside) {
      atomicAdd(&g.pass[at.k], delta);
      if (hit) {atomicAdd(&g.hits[at.k], delta);}
    }
  }
};

// the six counters of a fit: six named registers of the lane (kh_merge_fit_t's first six fields)
struct FitCounts
{
  uint32_t pass_unknown = 0u, pass_occupied = 0u, pass_free = 0u, hits_unknown = 0u, hits_occupied = 0u, hits_free = 0u;
};
template <typename Where>
struct FitCells                  // READ: a visit counts the cell's state (0 unknown, 100 occupied, 255 free) in the lane's registers
{
  const Where & g;
  FitCounts & n;
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    const CellAt at = cell_at(g, cx, cy);
    if (at.inside) {
      const uint32_t state = g.cells[at.k];
      // (three compares, no counter picked by an index computed from the state: that array would live in scratch memory)
      const uint32_t unknown = state == 0u, occupied = state == 100u, is_free = state == 255u;
      n.pass_unknown += unknown; n.pass_occupied += occupied; n.pass_free += is_free;
      if (hit) {n.hits_unknown += unknown; n.hits_occupied += occupied; n.hits_free += is_free;}
    }
  }
};

// The reduction of a workgroup's fit counters into row `row` of `out`: lanes -> wave by shuffles, the four waves through LDS, then one
// 64-bit atomicAdd per non-zero counter.  Every wave of the workgroup calls it (one with nothing to count, with zeros): there is a
// barrier inside.  The lane counters are uint32 (a walk visits fewer cells than the grid has); the sums are 64-bit from the first
// shuffle on.
__device__ __forceinline__ void fit_reduce(const FitCounts & c, unsigned long long * __restrict__ out, int32_t row)
{
  __shared__ unsigned long long part[4][kFitCounters];
  const uint32_t n[kFitCounters] = {c.pass_unknown, c.pass_occupied, c.pass_free, c.hits_unknown, c.hits_occupied, c.hits_free};     // kFitPassUnknown ..
  const int32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int32_t k = 0; k < kFitCounters; ++k) {
    unsigned long long v = n[k];
#pragma unroll
    for (int32_t d = 32; d >= 1; d >>= 1) {v += __shfl_xor(v, d);}
    if (lane == 0) {part[threadIdx.x >> 6][k] = v;}
  }
  __syncthreads();
  if (threadIdx.x < kFitCounters) {
    const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (v) {atomicAdd(&out[(int64_t)row * kFitCounters + threadIdx.x], v);}
  }
}

// Grid<kt_int32u>::TraceLine (Karto.h:4874-4927) from cell (x0, y0) to cell (x1, y1), then the end point (Karto.h:6213-6229)
template <typename Cells>
__device__ __forceinline__ void occ_walk(const Cells & cells, int32_t x0, int32_t y0, int32_t x1, int32_t y1, bool hit)
{
  const int32_t tx = x1, ty = y1;
  const bool steep = abs(y1 - y0) > abs(x1 - x0);
  int32_t t;
  if (steep) {t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t;}
  if (x0 > x1) {t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t;}
  const int32_t deltaX = x1 - x0, deltaY = abs(y1 - y0);
  int32_t error = 0, y = y0;
  const int32_t ystep = y0 < y1 ? 1 : -1;
  for (int32_t x = x0; x <= x1; x++) {
    const int32_t cx = steep ? y : x, cy = steep ? x : y;
    error += deltaY;
    if (2 * error >= deltaX) {y += ystep; error -= deltaX;}
    cells.add(cx, cy, false);
  }
  if (hit) {cells.add(tx, ty, true);}
}

// The bound in front of every walk on a map view.  The host has refused every input whose beams could walk more than kMaxFitWalk
// cells or leave the int32 lattice; this is the same bound once more, on the cells themselves, so that no lane can spin whatever
// reaches the kernel.
__device__ __forceinline__ bool walk_bounded(int32_t x0, int32_t y0, int32_t x1, int32_t y1)
{
  const int64_t limit = (1ll << 30) + 2 * kMaxFitWalk;
  const int64_t dx = (int64_t)x1 - x0, dy = (int64_t)y1 - y0;
  return x0 >= -limit && x0 <= limit && y0 >= -limit && y0 <= limit && dx >= -kMaxFitWalk && dx <= kMaxFitWalk &&
         dy >= -kMaxFitWalk && dy <= kMaxFitWalk;
}

// The work layout of the kernels that deal whole workgroups to a pose (a scan, a candidate): workgroup blockIdx.x belongs to pose
// blockIdx.x / blocks_per_pose, and its four waves are waves `wave` .. of that pose -- a wave is a run of 64 beams, lane l of it beam
// 64 wave + l.  (The host's side: blocks_per_pose() in occupancy_device.hpp.)
struct PoseWave
{
  int32_t pose;
  int64_t wave;
  __device__ __forceinline__ int64_t beam() const {return wave * 64 + (threadIdx.x & 63);}
};
__device__ __forceinline__ PoseWave pose_wave(int32_t blocks_per_pose)
{
  const int32_t pose = (int32_t)(blockIdx.x / (uint32_t)blocks_per_pose);
  return PoseWave{pose, (int64_t)(blockIdx.x - (uint32_t)pose * (uint32_t)blocks_per_pose) * 4 + (threadIdx.x >> 6)};
}

// ---- UpdateCell (Karto.h:6240-6256) ----
// the state a cell's two counters make: 0 = GridStates_Unknown (Clear()), 100 occupied, 255 free
// (h by reference: the hits of a cell that too few beams passed are not fetched)
__device__ __forceinline__ uint32_t occ_state(uint32_t p, const uint32_t & h, uint32_t min_pass, double threshold)
{
  uint32_t c = 0;
  if (p > min_pass) {                                                   // Karto.h:6244-6252
    const double ratio = (double)h / (double)p;
    c = ratio > threshold ? 100 : 255;
  }
  return c;
}
// ... for the cell at index k of the three arrays
__device__ __forceinline__ void occ_update_cell(const uint32_t * __restrict__ pass, const uint32_t * __restrict__ hits, uint8_t * __restrict__ cells,
  int64_t k, uint32_t min_pass, double threshold)
{
  cells[k] = (uint8_t)occ_state(pass[k], hits[k], min_pass, threshold);
}

// ---- nav_msgs/OccupancyGrid values (vis_utils::toNavMap, visualization_utils.hpp:108-146) ----
// Four cell states of one dword at once: 0 (unknown) -> -1 (0xFF), 100 (occupied) -> 100, 255 (free) -> 0.  Of the three states
// bit 2 is set in 100 and 255 and bit 7 in 255 only; a 0 / 1 byte times 0xFF is a 0x00 / 0xFF byte and carries nothing.
__device__ __forceinline__ uint32_t occ_nav4(uint32_t v)
{
  const uint32_t known = (v >> 2) & 0x01010101u, is_free = (v >> 7) & 0x01010101u;
  return (v & ~(is_free * 0xFFu)) | ((known ^ 0x01010101u) * 0xFFu);
}
}  // namespace kh
