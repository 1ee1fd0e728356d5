// karto::OccupancyGrid::CreateFromScans on the GPU: the map that slam_toolbox
// publishes every map_update_interval and that "end-to-end map build" (BASELINE config[4]) ends with.
//
//   ComputeDimensions  Karto.h:6086-6112 (+ LocalizedRangeScan::Update's bounding box, Karto.h:5694-5700)
//   AddScan            Karto.h:6148-6189   RayTrace   Karto.h:6199-6232
//   Grid::TraceLine    Karto.h:4874-4927   Update / UpdateCell  Karto.h:6240-6274
//
// One thread per beam: the clip to the range threshold and both WorldToGrid roundings are the reference's
// IEEE operations (compiled without FMA contraction), the Bresenham walk is integer, and the pass / hit
// counters are uint32 atomics in L2 -- increments commute, so the counters, hence the cells, are bit-exact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "occupancy_device.hpp"
#include "live_map_plan.hpp"
#include "map_localize_plan.hpp"

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

// ---- the one statement of AddScan / RayTrace / TraceLine every trace kernel below uses ----
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

// Where the cells of a walk live.  add() counts one visit of cell (cx, cy) -- and one hit, at a hit end -- if the cell exists.
struct GridCells                 // a whole grid: cell (0, 0) is the first, a visit adds 1
{
  const OccDev & g;
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    if (cx >= 0 && cx < g.width && cy >= 0 && cy < g.height) {
      atomicAdd(&g.pass[cx + (int64_t)cy * g.ws], 1u);
      if (hit) {atomicAdd(&g.hits[cx + (int64_t)cy * g.ws], 1u);}
    }
  }
};
struct WindowCells               // a live map's window of the lattice: cell (ox, oy) is the first, a visit adds delta (1, or 0xFFFFFFFF = -1)
{
  const LiveWindow & g;
  uint32_t delta;
  // 64-bit: a logged cell is any int32, the window's origin too.  The window holds every cell of every beam (coverage rule); the
  // bounds test is a guard.
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    const int64_t wx = (int64_t)cx - g.ox, wy = (int64_t)cy - g.oy;
    if (wx >= 0 && wx < g.width && wy >= 0 && wy < g.height) {
      atomicAdd(&g.pass[wx + wy * g.ws], delta);
      if (hit) {atomicAdd(&g.hits[wx + wy * g.ws], delta);}
    }
  }
};

struct FitCells                  // a whole grid, READ: a visit counts the cell's state (0 unknown, 100 occupied, 255 free) in the lane's registers
{
  const OccDev & g;
  uint32_t & pass_unknown, & pass_occupied, & pass_free, & hits_unknown, & hits_occupied, & hits_free;
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    if (cx >= 0 && cx < g.width && cy >= 0 && cy < g.height) {
      const uint32_t state = g.cells[cx + (int64_t)cy * g.ws];
      // (three compares, no counter picked by an index computed from the state: that array would live in scratch memory)
      const uint32_t unknown = state == 0u, occupied = state == 100u, is_free = state == 255u;
      pass_unknown += unknown; pass_occupied += occupied; pass_free += is_free;
      if (hit) {hits_unknown += unknown; hits_occupied += occupied; hits_free += is_free;}
    }
  }
};

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

// AddScan + RayTrace of one beam into a whole grid: what the three kernels below do once a thread has found its beam and its gates
// (the inputs by reference: a kernel that passes fields of a record it fetched leaves the fetch of the fields a dropped beam never
// needs behind the drop test, as when the statements stood in the kernel itself)
__device__ __forceinline__ void occ_trace_beam(const OccDev & g, const double & r, double px, double py, const double & sx, const double & sy,
  const double & range_threshold, const double & min_range, const double & max_range)
{
  const Beam b = occ_gate(r, px, py, sx, sy, range_threshold, min_range, max_range);
  if (!b.kept) {return;}
  const int32_t x0 = occ_cell(sx, g.off_x, g.scale), y0 = occ_cell(sy, g.off_y, g.scale);
  const int32_t x1 = occ_cell(b.px, g.off_x, g.scale), y1 = occ_cell(b.py, g.off_y, g.scale);
  occ_walk(GridCells{g}, x0, y0, x1, y1, b.hit);
}

// beams: [n_beams] of (range, point x, point y, sensor x, sensor y) packed as 5 doubles
__global__ __launch_bounds__(256) void k_occ_trace(
  OccDev g, const double * __restrict__ beams, int64_t n_beams, double range_threshold, double min_range, double max_range)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_beams) {return;}
  occ_trace_beam(g, beams[5 * i], beams[5 * i + 1], beams[5 * i + 2], beams[5 * i + 3], beams[5 * i + 4], range_threshold, min_range, max_range);
}

// The same trace fed from a mapper's RESIDENT scans (kh_mapper_build_map): one ResidentScan per scan instead of 40 bytes per beam.
// One wave per run of 64 neighbouring beams of ONE scan (a workgroup = 4 such runs): the beams of a wave leave the same cell and
// fan out over neighbouring ones, so its atomics land in neighbouring L2 lines, and neighbouring beams have similar lengths, which
// bounds the divergence of the walk.
__global__ __launch_bounds__(256) void k_occ_trace_resident(
  OccDev g, const ResidentScan * __restrict__ scans, int32_t n_scans, int32_t n_beams, int32_t runs_per_scan, double range_threshold,
  double min_range, double max_range)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int32_t lane = threadIdx.x & 63;
  const int64_t s = wave / runs_per_scan;
  if (s >= n_scans) {return;}
  const int32_t i = (int32_t)(wave - s * runs_per_scan) * 64 + lane;
  if (i >= n_beams) {return;}
  const ResidentScan sc = scans[s];
  occ_trace_beam(g, sc.ranges[i], sc.points[2 * i], sc.points[2 * i + 1], sc.sx, sc.sy, range_threshold, min_range, max_range);
}

// The trace of a MERGE of mapping sessions (kh_merge_build): the scans of several mappers, each mapper (submap) placed by a rigid
// correction.  The resident readings stay as their mapper made them; the submap's correction is applied to the point in registers
// -- x' = (c x - s y) + tx, y' = (s x + c y) + ty, no contraction -- and nothing transformed is written back.  The sensor position
// arrives transformed (the host does GetSensorAt of the transformed corrected pose, once per scan).
// The same work layout as k_occ_trace_resident.  Submaps may have different lasers: the grid is dealt max_runs waves per scan
// (the longest laser's), a wave beyond its scan's own beam count leaves at once.
__global__ __launch_bounds__(256) void k_occ_trace_merged(
  OccDev g, const MergeScan * __restrict__ scans, const MergeSubmap * __restrict__ submaps, int32_t n_scans, int32_t max_runs)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int32_t lane = threadIdx.x & 63;
  const int64_t s = wave / max_runs;
  if (s >= n_scans) {return;}
  const MergeScan sc = scans[s];
  const MergeSubmap sm = submaps[sc.submap];
  const int32_t i = (int32_t)(wave - s * max_runs) * 64 + lane;
  if (i >= sm.n_beams) {return;}
  const double ux = sc.points[2 * i], uy = sc.points[2 * i + 1];
  const double px = (sm.c * ux - sm.s * uy) + sm.tx, py = (sm.s * ux + sm.c * uy) + sm.ty;
  occ_trace_beam(g, sc.ranges[i], px, py, sc.sx, sc.sy, sm.range_threshold, sm.min_range, sm.max_range);
}

// The FIT of candidate corrections of one submap against a finished grid (kh_merge_fit): k_occ_trace_merged's work layout times the
// candidates -- one wave per (candidate, scan, run of 64 beams) -- and its arithmetic, but the walk looks up the state of every
// cell it would have incremented and counts, per state, visits and hits in six registers of the lane (FitCells).  The grid is only
// read.  A workgroup holds waves of ONE candidate (blocks_per_candidate = ceil(n_scans * runs_per_scan / 4)), so its sums go to one
// row of `out`: lanes -> wave by shuffles, the four waves through LDS, then one vector atomicAdd per non-zero counter.  A wave
// past the last scan and a lane past the beam count take part in the reduction with zeros: every wave reaches the barrier.
// The lane counters are uint32 (a walk visits fewer cells than the grid has); the sums are 64-bit from the first shuffle on.
__global__ __launch_bounds__(256) void k_occ_fit_merged(
  OccDev g, const ResidentScan * __restrict__ scans, const FitCandidate * __restrict__ candidates, const FitSensor * __restrict__ sensors,
  int32_t n_scans, int32_t n_beams, int32_t runs_per_scan, int32_t blocks_per_candidate, double range_threshold, double min_range,
  double max_range, unsigned long long * __restrict__ out)
{
  __shared__ unsigned long long part[4][kFitCounters];
  const int32_t candidate = (int32_t)(blockIdx.x / (uint32_t)blocks_per_candidate);
  const int64_t wave = (int64_t)(blockIdx.x - (uint32_t)candidate * (uint32_t)blocks_per_candidate) * 4 + (threadIdx.x >> 6);
  const int32_t lane = threadIdx.x & 63;
  const int64_t s = wave / runs_per_scan;
  const int32_t i = (int32_t)(wave - s * runs_per_scan) * 64 + lane;
  uint32_t n[kFitCounters] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (s < n_scans && i < n_beams) {
    const ResidentScan sc = scans[s];
    const FitCandidate t = candidates[candidate];
    const FitSensor sensor = sensors[(int64_t)candidate * n_scans + s];
    const double ux = sc.points[2 * i], uy = sc.points[2 * i + 1];
    const double px = (t.c * ux - t.s * uy) + t.tx, py = (t.s * ux + t.c * uy) + t.ty;
    const Beam b = occ_gate(sc.ranges[i], px, py, sensor.sx, sensor.sy, range_threshold, min_range, max_range);
    if (b.kept) {
      const int32_t x0 = occ_cell(sensor.sx, g.off_x, g.scale), y0 = occ_cell(sensor.sy, g.off_y, g.scale);
      const int32_t x1 = occ_cell(b.px, g.off_x, g.scale), y1 = occ_cell(b.py, g.off_y, g.scale);
      occ_walk(FitCells{g, n[kFitPassUnknown], n[kFitPassOccupied], n[kFitPassFree], n[kFitHitsUnknown], n[kFitHitsOccupied], n[kFitHitsFree]},
        x0, y0, x1, y1, b.hit);
    }
  }
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
    if (v) {atomicAdd(&out[(int64_t)candidate * kFitCounters + threadIdx.x], v);}
  }
}

// ---- a map view as a localizer reads it (kh_map_seeds, kh_map_fit) ----
struct FitWindowCells            // FitCells on a window of the lattice: cell (ox, oy) is the first; WindowCells' 64-bit index and bounds guard
{
  const MapWindow & g;
  uint32_t & pass_unknown, & pass_occupied, & pass_free, & hits_unknown, & hits_occupied, & hits_free;
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    const int64_t wx = (int64_t)cx - g.ox, wy = (int64_t)cy - g.oy;
    if (wx >= 0 && wx < g.width && wy >= 0 && wy < g.height) {
      const uint32_t state = g.cells[wx + wy * g.ws];
      const uint32_t unknown = state == 0u, occupied = state == 100u, is_free = state == 255u;
      pass_unknown += unknown; pass_occupied += occupied; pass_free += is_free;
      if (hit) {hits_unknown += unknown; hits_occupied += occupied; hits_free += is_free;}
    }
  }
};

// The FIT of one scan at many sensor poses against a map view (kh_map_fit): k_occ_fit_merged's layout without the scan dimension --
// one wave per (pose, run of 64 beams), a workgroup holds waves of ONE pose (blocks_per_pose = ceil(runs / 4)) -- and its reduction:
// six lane counters, shuffles, LDS, one 64-bit atomicAdd per non-zero counter and workgroup.  points: per pose the 2 * n_beams
// unfiltered point readings at that pose (kh_scan_points on the host: libm stays there); sensors: 2 per pose.  The view is only read.
// The host has refused every input whose beams could walk more than kMaxFitWalk cells or leave the int32 lattice; the test in front of
// the walk is the same bound once more, on the cells themselves, so that no lane can spin whatever reaches the kernel.
__global__ __launch_bounds__(256) void k_map_fit(
  MapWindow g, const double * __restrict__ ranges, const double * __restrict__ points, const double * __restrict__ sensors, int32_t n_beams,
  int32_t blocks_per_pose, double range_threshold, double min_range, double max_range, unsigned long long * __restrict__ out)
{
  __shared__ unsigned long long part[4][kFitCounters];
  const int32_t pose = (int32_t)(blockIdx.x / (uint32_t)blocks_per_pose);
  const int64_t wave = (int64_t)(blockIdx.x - (uint32_t)pose * (uint32_t)blocks_per_pose) * 4 + (threadIdx.x >> 6);
  const int32_t lane = threadIdx.x & 63;
  const int64_t i = wave * 64 + lane;
  uint32_t n[kFitCounters] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (i < n_beams) {
    const double sx = sensors[2 * (int64_t)pose], sy = sensors[2 * (int64_t)pose + 1];
    const double * const p = points + 2 * ((int64_t)pose * n_beams + i);
    const Beam b = occ_gate(ranges[i], p[0], p[1], sx, sy, range_threshold, min_range, max_range);
    if (b.kept) {
      const int32_t x0 = occ_cell(sx, g.ax, g.scale), y0 = occ_cell(sy, g.ay, g.scale);
      const int32_t x1 = occ_cell(b.px, g.ax, g.scale), y1 = occ_cell(b.py, g.ay, g.scale);
      const int64_t limit = (1ll << 30) + 2 * kMaxFitWalk;
      const int64_t dx = (int64_t)x1 - x0, dy = (int64_t)y1 - y0;
      const bool bounded = x0 >= -limit && x0 <= limit && y0 >= -limit && y0 <= limit && dx >= -kMaxFitWalk && dx <= kMaxFitWalk &&
        dy >= -kMaxFitWalk && dy <= kMaxFitWalk;
      if (bounded) {
        occ_walk(FitWindowCells{g, n[kFitPassUnknown], n[kFitPassOccupied], n[kFitPassFree], n[kFitHitsUnknown], n[kFitHitsOccupied], n[kFitHitsFree]},
          x0, y0, x1, y1, b.hit);
      }
    }
  }
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
    if (v) {atomicAdd(&out[(int64_t)pose * kFitCounters + threadIdx.x], v);}
  }
}

// The EXPECTED scan of a map view (kh_map_raycast): one lane per (pose, beam), k_map_fit's layout -- a wave holds
// 64 consecutive beams of one pose, so neighbouring lanes read neighbouring cells near the sensor.  points: per pose the far point of
// every beam (kh_scan_points of readings that are all range_threshold, on the host: libm stays there).  The lane visits the cells of
// TraceLine(sensor cell, far cell) outward from the sensor (RayWalk) and leaves at the first decision: an occupied cell (HIT), or
// the unknown cell that exceeds the budget (UNKNOWN; a cell outside the window and every state but 100 / 255 is unknown); the end of
// the line is FREE at the far cell.  FitWindowCells' 64-bit index and bounds guard; k_map_fit's bound in front of the walk.  Once a
// lane stands outside the window on a side its line leads away from, no later cell exists: with no budget to run out (max_unknown
// < 0) the answer is FREE, and the lane says so at once.  No atomics, no LDS, one 16-byte store per lane.  A wave runs as long as its
// longest lane.
__global__ __launch_bounds__(256) void k_map_raycast(
  MapWindow g, const double * __restrict__ points, const double * __restrict__ sensors, int32_t n_beams, int32_t blocks_per_pose,
  int32_t max_unknown, RayCell * __restrict__ out)
{
  const int32_t pose = (int32_t)(blockIdx.x / (uint32_t)blocks_per_pose);
  const int64_t i = ((int64_t)(blockIdx.x - (uint32_t)pose * (uint32_t)blocks_per_pose) * 4 + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
  if (i >= n_beams) {return;}
  const double sx = sensors[2 * (int64_t)pose], sy = sensors[2 * (int64_t)pose + 1];
  const double * const p = points + 2 * ((int64_t)pose * n_beams + i);
  const int32_t x0 = occ_cell(sx, g.ax, g.scale), y0 = occ_cell(sy, g.ay, g.scale);
  const int32_t x1 = occ_cell(p[0], g.ax, g.scale), y1 = occ_cell(p[1], g.ay, g.scale);
  const int64_t limit = (1ll << 30) + 2 * kMaxFitWalk;
  const int64_t ex = (int64_t)x1 - x0, ey = (int64_t)y1 - y0;
  const bool bounded = x0 >= -limit && x0 <= limit && y0 >= -limit && y0 <= limit && ex >= -kMaxFitWalk && ex <= kMaxFitWalk &&
    ey >= -kMaxFitWalk && ey <= kMaxFitWalk;
  RayCell r{x1, y1, 0, KH_RAY_FREE};
  if (bounded) {
    RayWalk walk(x0, y0, x1, y1);
    const int32_t length = walk.length();
    r.steps = length;
    int32_t unknown = 0;
    for (int32_t s = 0; s <= length; ++s, walk.next()) {
      const int32_t cx = walk.x(), cy = walk.y();
      const int64_t wx = (int64_t)cx - g.ox, wy = (int64_t)cy - g.oy;
      uint32_t state = 0u;
      if (wx >= 0 && wx < g.width && wy >= 0 && wy < g.height) {
        state = g.cells[wx + wy * g.ws];
      } else if (max_unknown < 0 && ((wx < 0 && ex <= 0) || (wx >= g.width && ex >= 0) || (wy < 0 && ey <= 0) || (wy >= g.height && ey >= 0))) {
        break;
      }
      if (state == 100u) {r = RayCell{cx, cy, s, KH_RAY_HIT}; break;}
      if (state != 255u) {
        ++unknown;
        if (max_unknown >= 0 && unknown > max_unknown) {r = RayCell{cx, cy, s, KH_RAY_UNKNOWN}; break;}
      }
    }
  }
  out[(int64_t)pose * n_beams + i] = r;
}

// Where a robot can stand (kh_map_seeds): one wave per block of pitch x pitch lattice cells; block `b` of the launch is block column
// bx0 + b % nbx, block row by0 + b / nbx of the lattice.  The lanes stride over the block's cells inside the window, row-major, so a
// wave reads runs of consecutive bytes of a row wherever the row segment is long enough.  Each lane keeps the minimum of a 64-bit
// key over its free cells: the squared distance of the doubled cell index from the doubled block centre in the high half (at most
// 2 * 4095^2), the row-major index inside the block in the low half (below 4096^2) -- so the minimum is the nearest free cell, ties
// to the smaller row, then the smaller column.  The wave reduces by shuffles and lane 0 writes the low half, or -1 when the block
// holds no free cell, to the block's own word: no atomic decides anything.
__global__ __launch_bounds__(256) void k_map_seeds(MapWindow g, int32_t pitch, int64_t bx0, int64_t by0, int64_t nbx, int64_t n_blocks,
  int32_t * __restrict__ out)
{
  const int64_t block = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (block >= n_blocks) {return;}                     // (the whole wave leaves)
  const int32_t lane = threadIdx.x & 63;
  const int64_t by = block / nbx, bx = block - by * nbx;
  const int64_t lx0 = (bx0 + bx) * pitch, ly0 = (by0 + by) * pitch;            // the block's first lattice cell
  // its part inside the window, in window columns and rows
  const int64_t wx0 = lx0 - g.ox > 0 ? lx0 - g.ox : 0, wx1 = lx0 + pitch - g.ox < g.width ? lx0 + pitch - g.ox : g.width;
  const int64_t wy0 = ly0 - g.oy > 0 ? ly0 - g.oy : 0, wy1 = ly0 + pitch - g.oy < g.height ? ly0 + pitch - g.oy : g.height;
  const int32_t cw = (int32_t)(wx1 - wx0), ch = (int32_t)(wy1 - wy0);
  unsigned long long key = ~0ull;
  if (cw > 0 && ch > 0) {
    const uint32_t total = (uint32_t)cw * (uint32_t)ch;
    const int64_t cx2 = 2 * lx0 + pitch - 1, cy2 = 2 * ly0 + pitch - 1;        // the doubled block centre
    for (uint32_t idx = lane; idx < total; idx += 64u) {
      const uint32_t row = idx / (uint32_t)cw, col = idx - row * (uint32_t)cw;
      const int64_t wx = wx0 + col, wy = wy0 + row;
      if (g.cells[wx + wy * g.ws] == 255u) {
        const int64_t lx = wx + g.ox, ly = wy + g.oy;
        const int64_t dx = 2 * lx - cx2, dy = 2 * ly - cy2;
        const unsigned long long k = ((unsigned long long)(dx * dx + dy * dy) << 32) | (unsigned long long)((ly - ly0) * pitch + (lx - lx0));
        key = k < key ? k : key;
      }
    }
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    const unsigned long long other = __shfl_xor(key, d);
    key = other < key ? other : key;
  }
  if (lane == 0) {out[block] = key == ~0ull ? -1 : (int32_t)(key & 0xFFFFFFFFull);}
}

// UpdateCell (Karto.h:6240-6256) for the cell at index k of the three arrays
__device__ __forceinline__ void occ_update_cell(const uint32_t * __restrict__ pass, const uint32_t * __restrict__ hits, uint8_t * __restrict__ cells,
  int64_t k, uint32_t min_pass, double threshold)
{
  uint8_t c = 0;                                                       // GridStates_Unknown (Clear())
  const uint32_t p = pass[k];
  if (p > min_pass) {                                                   // Karto.h:6244-6252
    const double ratio = (double)hits[k] / (double)p;
    c = ratio > threshold ? 100 : 255;
  }
  cells[k] = c;
}

__global__ __launch_bounds__(256) void k_occ_update(OccDev g, uint32_t min_pass, double threshold)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)g.ws * g.height) {return;}
  occ_update_cell(g.pass, g.hits, g.cells, k, min_pass, threshold);
}

// The same rule over a rectangle of a live map's window (kh_live_map_update: the cells a delta can have touched)
__global__ __launch_bounds__(256) void k_occ_update_rect(LiveWindow g, int32_t x0, int32_t y0, int32_t rect_w, int32_t rect_h, uint32_t min_pass,
  double threshold)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)rect_w * rect_h) {return;}
  const int64_t y = k / rect_w, x = k - y * rect_w;
  occ_update_cell(g.pass, g.hits, g.cells, (x0 + x) + (y0 + y) * (int64_t)g.ws, min_pass, threshold);
}

// ---- the live map's trace (kh_live_map_update) ----
// The work layout of k_occ_trace_resident -- one wave per run of 64 neighbouring beams of one scan -- over a table of ADD / SUB /
// MOVE records (occupancy_device.hpp).  ADD traces from the resident readings and writes the scan's slot of the log; SUB walks the
// logged lines with -1 and reads nothing else; MOVE compares the beam's new trace record with the logged one and walks (old line
// -1, new line +1) only where something differs.  One scan is one record, so no two waves touch the same log words: a beam's two
// words belong to its lane, and the slot's sensor cell is written by beam 0's lane and read by SUB records only (MOVE gets the old
// cell in its record).
__global__ __launch_bounds__(256) void k_occ_trace_delta(
  LiveWindow g, double ax, double ay, double scale, const DeltaRecord * __restrict__ records, int32_t n_records, int32_t n_beams,
  int32_t runs_per_scan, double range_threshold, double min_range, double max_range, int32_t * __restrict__ log, int64_t slot_words,
  unsigned long long * __restrict__ counters)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int32_t lane = threadIdx.x & 63;
  const int64_t s = wave / runs_per_scan;
  if (s >= n_records) {return;}
  const int32_t i = (int32_t)(wave - s * runs_per_scan) * 64 + lane;
  if (i >= n_beams) {return;}
  const DeltaRecord rec = records[s];
  int32_t * const slot = log + rec.slot * slot_words;
  int2 * const entry = reinterpret_cast<int2 *>(slot + 2) + i;
  // the logged line (SUB, MOVE) and the new one (ADD, MOVE)
  int32_t ocx = rec.old_cx, ocy = rec.old_cy, ncx = 0, ncy = 0;
  int2 was = make_int2(0, 0), now = make_int2(0, 0);
  if (rec.kind != kDeltaAdd) {was = *entry;}
  if (rec.kind == kDeltaSub) {ocx = slot[0]; ocy = slot[1];}
  if (rec.kind != kDeltaSub) {
    const Beam b = occ_gate(rec.ranges[i], rec.points[2 * i], rec.points[2 * i + 1], rec.sx, rec.sy, range_threshold, min_range, max_range);
    ncx = occ_cell(rec.sx, ax, scale); ncy = occ_cell(rec.sy, ay, scale);
    if (b.kept) {now = make_int2(occ_cell(b.px, ax, scale), (int32_t)(((uint32_t)(occ_cell(b.py, ay, scale) - ncy) << 2) | (b.hit ? 3u : 1u)));}
  }
  const bool same = rec.kind == kDeltaMove && was.x == now.x && was.y == now.y && ocx == ncx && ocy == ncy;
  const bool walk_old = rec.kind != kDeltaAdd && !same && (was.y & 1);
  const bool walk_new = rec.kind != kDeltaSub && !same && (now.y & 1);
  if (walk_old) {occ_walk(WindowCells{g, 0xFFFFFFFFu}, ocx, ocy, was.x, ocy + (was.y >> 2), (was.y & 2) != 0);}
  if (walk_new) {occ_walk(WindowCells{g, 1u}, ncx, ncy, now.x, ncy + (now.y >> 2), (now.y & 2) != 0);}
  if (rec.kind != kDeltaSub) {
    if (!same) {*entry = now;}
    if (i == 0) {slot[0] = ncx; slot[1] = ncy;}
  }
  // lane 0 holds the run's first beam, so it is here whenever the wave is
  const int walked = __popcll(__ballot(walk_old)) + __popcll(__ballot(walk_new));
  const int skipped = __popcll(__ballot(same && (now.y & 1)));
  if (lane == 0) {
    if (walked) {atomicAdd(&counters[0], (unsigned long long)walked);}
    if (skipped) {atomicAdd(&counters[1], (unsigned long long)skipped);}
  }
}

// ---- a change layer on a map view (kh_map_changes_*) ----
struct ObserveCells              // WindowCells with delta 1 on the layer and, in the same visit, FitWindowCells' read of the map's state
{
  const MapWindow & g;
  const ChangeLayer & layer;
  int64_t ex, ey, tolerance;     // the beam's end cell: a visit further than `tolerance` from it (Chebyshev) on an occupied map cell blocks
  uint32_t & blocked;
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    const int64_t wx = (int64_t)cx - g.ox, wy = (int64_t)cy - g.oy;
    if (wx >= 0 && wx < g.width && wy >= 0 && wy < g.height) {
      const int64_t k = wx + wy * g.ws;
      const uint32_t state = g.cells[k];               // (the load is issued before the atomics, not behind them)
      atomicAdd(&layer.pass[k], 1u);
      if (hit) {
        atomicAdd(&layer.hits[k], 1u);                 // (the hit's second visit of the end cell is no visit of the line)
      } else {
        const int64_t dx = cx > ex ? cx - ex : ex - cx, dy = cy > ey ? cy - ey : ey - cy;
        blocked += (uint32_t)(state == 100u) & (uint32_t)((dx > dy ? dx : dy) > tolerance);
      }
    }
  }
};

// OBSERVE n_scans scans into a change layer and label every beam against the map (kh_map_changes_observe): k_map_fit's layout with
// "pose" read as "scan" -- one wave per (scan, run of 64 beams), a workgroup holds waves of ONE scan -- and every scan with ranges of
// its own.  ONE walk under ONE visitor: it adds to the layer what k_occ_trace_delta's ADD adds, and counts in a lane register the
// occupied map cells the line crosses before it comes within `tolerance` cells of its end (the end cell is known before the walk, and
// the Chebyshev distance from it does not depend on the direction occ_walk takes).  Then at most (2 tolerance + 1)^2 cells around the
// end cell say whether the map holds an obstacle there, and the lane writes its two label words.  The map is only read, by plain
// loads; the layer only by atomics.  The walk bound in front of the walk is k_map_fit's; a beam it stops is labelled as dropped.
__global__ __launch_bounds__(256) void k_map_observe(
  MapWindow g, ChangeLayer layer, const double * __restrict__ ranges, const double * __restrict__ points, const double * __restrict__ sensors,
  int32_t n_beams, int32_t blocks_per_scan, double range_threshold, double min_range, double max_range, int32_t tolerance,
  int2 * __restrict__ labels)
{
  const int32_t scan = (int32_t)(blockIdx.x / (uint32_t)blocks_per_scan);
  const int64_t wave = (int64_t)(blockIdx.x - (uint32_t)scan * (uint32_t)blocks_per_scan) * 4 + (threadIdx.x >> 6);
  const int64_t i = wave * 64 + (threadIdx.x & 63);
  if (i >= n_beams) {return;}
  const int64_t beam = (int64_t)scan * n_beams + i;
  const double sx = sensors[2 * (int64_t)scan], sy = sensors[2 * (int64_t)scan + 1];
  const Beam b = occ_gate(ranges[beam], points[2 * beam], points[2 * beam + 1], sx, sy, range_threshold, min_range, max_range);
  int32_t label = KH_BEAM_DROPPED;
  uint32_t blocked = 0;
  if (b.kept) {
    const int32_t x0 = occ_cell(sx, g.ax, g.scale), y0 = occ_cell(sy, g.ay, g.scale);
    const int32_t x1 = occ_cell(b.px, g.ax, g.scale), y1 = occ_cell(b.py, g.ay, g.scale);
    const int64_t limit = (1ll << 30) + 2 * kMaxFitWalk;
    const int64_t dx = (int64_t)x1 - x0, dy = (int64_t)y1 - y0;
    const bool bounded = x0 >= -limit && x0 <= limit && y0 >= -limit && y0 <= limit && dx >= -kMaxFitWalk && dx <= kMaxFitWalk &&
      dy >= -kMaxFitWalk && dy <= kMaxFitWalk;
    if (bounded) {
      occ_walk(ObserveCells{g, layer, x1, y1, tolerance, blocked}, x0, y0, x1, y1, b.hit);
      if (blocked > 0) {
        label = KH_BEAM_THROUGH;
      } else if (!b.hit) {
        label = KH_BEAM_CLEAR;
      } else {
        // the window cells within `tolerance` of the end cell, clipped to the window; the end cell's own state from the same loads
        const int64_t ex = (int64_t)x1 - g.ox, ey = (int64_t)y1 - g.oy;
        const int64_t lo_x = ex - tolerance > 0 ? ex - tolerance : 0, hi_x = ex + tolerance < g.width - 1 ? ex + tolerance : g.width - 1;
        const int64_t lo_y = ey - tolerance > 0 ? ey - tolerance : 0, hi_y = ey + tolerance < g.height - 1 ? ey + tolerance : g.height - 1;
        bool near = false, end_free = false;
        for (int64_t wy = lo_y; wy <= hi_y; ++wy) {
          for (int64_t wx = lo_x; wx <= hi_x; ++wx) {
            const uint32_t state = g.cells[wx + wy * g.ws];
            near = near || state == 100u;
            end_free = end_free || (state == 255u && wx == ex && wy == ey);
          }
        }
        label = near ? KH_BEAM_EXPLAINED : end_free ? KH_BEAM_NOVEL : KH_BEAM_UNKNOWN;
      }
    }
  }
  labels[beam] = make_int2(label, (int32_t)blocked);
}

// both grids of a change layer >>= shift (kh_map_changes_decay): one thread per cell of the strided window
__global__ __launch_bounds__(256) void k_map_decay(ChangeLayer layer, int64_t size, int32_t shift)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= size) {return;}
  layer.pass[k] >>= shift;
  layer.hits[k] >>= shift;
}

// The layer set against its map (kh_map_changes_diff): one thread per cell of the strided window.  The observed state is
// occ_update_cell's rule on the layer's counters; the code says what it makes of the map's state, the patched state is the observed
// one where it is known, else the map's.  The threads of the row padding write 0 to both and count nowhere.  The six counts: one
// ballot per code, its popcount kept by lane 0, the four waves through LDS, one 64-bit atomicAdd per non-zero count and workgroup --
// integer sums, so the order does not matter.
__global__ __launch_bounds__(256) void k_map_diff(MapWindow g, ChangeLayer layer, uint32_t min_pass, double threshold, uint8_t * __restrict__ codes,
  uint8_t * __restrict__ patched, unsigned long long * __restrict__ counts)
{
  __shared__ uint32_t part[4][kChangeCodes];
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t y = k / g.ws;
  const bool cell = y < g.height && k - y * g.ws < g.width;
  uint32_t code = KH_CELL_UNOBSERVED;
  if (cell) {
    const uint32_t raw = g.cells[k], p = layer.pass[k];
    const uint32_t map = (raw == 100u || raw == 255u) ? raw : 0u;
    uint32_t seen = 0u;
    if (p > min_pass) {                                                 // Karto.h:6244-6252
      const double ratio = (double)layer.hits[k] / (double)p;
      seen = ratio > threshold ? 100u : 255u;
    }
    if (seen != 0u) {
      code = seen == map ? KH_CELL_CONFIRMED : map == 255u ? KH_CELL_APPEARED : map == 100u ? KH_CELL_VANISHED :
        seen == 100u ? KH_CELL_DISCOVERED_OCCUPIED : KH_CELL_DISCOVERED_FREE;
    }
    codes[k] = (uint8_t)code;
    patched[k] = (uint8_t)(seen != 0u ? seen : raw);
  } else if (y < g.height) {
    codes[k] = 0; patched[k] = 0;
  }
  const int32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int32_t c = 0; c < kChangeCodes; ++c) {
    const uint32_t n = (uint32_t)__builtin_popcountll(__ballot(cell && code == (uint32_t)c));
    if (lane == 0) {part[threadIdx.x >> 6][c] = n;}
  }
  __syncthreads();
  if (threadIdx.x < kChangeCodes) {
    const uint32_t v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (v) {atomicAdd(&counts[threadIdx.x], (unsigned long long)v);}
  }
}

// The changed cells (code >= 2) as a list in row-major window order, with no atomic deciding a position: k_map_collect's idiom
// (matcher_kernels.hip).  A wave takes a unit of 64 consecutive cells of a row; its ballot's popcount is the unit's count (count
// phase), k_map_changed_scan turns the counts into their exclusive prefix, and the fill phase repeats the ballot and writes cell
// `lane` of unit u to prefix[u] + the set bits below the lane -- never past the unit's room, nor past `cap` entries.
template <bool kFill>
__global__ __launch_bounds__(256) void k_map_changed(MapWindow g, const uint8_t * __restrict__ codes, int32_t units_per_row, int64_t n_units,
  int32_t * __restrict__ unit, int32_t * __restrict__ list, int32_t cap)
{
  const int32_t lane = threadIdx.x & 63;
  const int64_t first = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), step = (int64_t)gridDim.x * 4;
  for (int64_t u = first; u < n_units; u += step) {
    const int64_t row = u / units_per_row;
    const int64_t x = 64 * (u - row * units_per_row) + lane;
    const uint32_t code = x < g.width ? codes[x + row * g.ws] : 0u;
    const bool changed = code >= 2u;
    const unsigned long long mask = __ballot(changed);
    if (!kFill) {
      if (lane == 0) {unit[u] = __builtin_popcountll(mask);}
    } else if (changed) {
      const int32_t at = unit[u] + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
      if (at < unit[u + 1] && at < cap) {
        list[3 * (int64_t)at] = (int32_t)(g.ox + x); list[3 * (int64_t)at + 1] = (int32_t)(g.oy + row); list[3 * (int64_t)at + 2] = (int32_t)code;
      }
    }
  }
}

// counts -> exclusive prefix, in place; unit[n_units] takes the sum.  One workgroup (k_map_collect_scan's scan).
__global__ __launch_bounds__(1024) void k_map_changed_scan(int32_t * __restrict__ unit, int64_t n_units)
{
  const int64_t per = (n_units + 1023) / 1024;
  const int64_t lo = (int64_t)threadIdx.x * per < n_units ? (int64_t)threadIdx.x * per : n_units, hi = lo + per < n_units ? lo + per : n_units;
  __shared__ int32_t s_sum[1024];
  int32_t sum = 0;
  for (int64_t u = lo; u < hi; ++u) {sum += unit[u];}
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (int32_t d = 1; d < 1024; d <<= 1) {             // Hillis-Steele inclusive scan of the per-thread totals
    int32_t a = 0;
    if ((int32_t)threadIdx.x >= d) {a = s_sum[threadIdx.x - d];}
    __syncthreads();
    s_sum[threadIdx.x] += a;
    __syncthreads();
  }
  int32_t run = s_sum[threadIdx.x] - sum;
  for (int64_t u = lo; u < hi; ++u) {
    const int32_t c = unit[u];
    unit[u] = run;
    run += c;
  }
  if (threadIdx.x == 1023) {unit[n_units] = s_sum[1023];}
}

// ---- nav_msgs/OccupancyGrid values (vis_utils::toNavMap, visualization_utils.hpp:108-146) ----
// Four cell states of one dword at once: 0 (unknown) -> -1 (0xFF), 100 (occupied) -> 100, 255 (free) -> 0.  Of the three states
// bit 2 is set in 100 and 255 and bit 7 in 255 only; a 0 / 1 byte times 0xFF is a 0x00 / 0xFF byte and carries nothing.
__device__ __forceinline__ uint32_t occ_nav4(uint32_t v)
{
  const uint32_t known = (v >> 2) & 0x01010101u, is_free = (v >> 7) & 0x01010101u;
  return (v & ~(is_free * 0xFFu)) | ((known ^ 0x01010101u) * 0xFFu);
}

// toNavMap of a whole grid (kh_occupancy_read_nav): from the ws-strided cells into a DENSE width x height array, so that an output
// dword may span rows (any width, width < 4 too).  One thread per output dword; the bytes past `total` of the last one are padding
// of the buffer.
__global__ __launch_bounds__(256) void k_occ_to_nav(const uint8_t * __restrict__ cells, int32_t width, int32_t ws, int64_t total,
  uint32_t * __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t k = 4 * i;
  if (k >= total) {return;}
  int64_t y = k / width;
  int32_t x = (int32_t)(k - y * width);
  uint32_t v = 0;
  for (int32_t b = 0; b < 4 && k + b < total; ++b) {
    v |= (uint32_t)cells[x + y * ws] << (8 * b);
    if (++x == width) {x = 0; ++y;}
  }
  out[i] = occ_nav4(v);
}

// The inverse of k_occ_to_nav (kh_occupancy_write_nav): from a DENSE width x height array of nav values into the ws-strided cells,
// -1 -> 0 (unknown), 100 -> 100 (occupied), 0 -> 255 (free); the host has refused every other value.  One thread per dword of the
// cells (ws is a multiple of 8); the bytes of the row padding are written as 0.
__global__ __launch_bounds__(256) void k_nav_to_occ(const int8_t * __restrict__ nav, int32_t width, int32_t ws, int64_t words,
  uint32_t * __restrict__ cells)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) {return;}
  const int32_t words_per_row = ws >> 2;
  const int64_t y = i / words_per_row;
  const int32_t x = 4 * (int32_t)(i - y * words_per_row);
  uint32_t v = 0;
  for (int32_t b = 0; b < 4 && x + b < width; ++b) {
    const int32_t n = nav[y * width + x + b];
    v |= (n == 100 ? 100u : n == 0 ? 255u : 0u) << (8 * b);
  }
  cells[i] = v;
}

// The map feed's compare-and-pack (kh_map_feed_poll).  One wave per STRIP of four horizontally adjacent
// tiles, 64 cells x 16 rows: a load instruction of the wave reads four whole 64-byte row segments.  A lane owns the dword column
// lane & 15 of the strip -- so tile (lane & 15) >> 2 -- and the rows lane >> 4, + 4, + 8, + 12.  It turns its four dwords of cell
// states into nav values, compares them with the same four dwords of the published grid, and a ballot masked per tile says which
// of the four tiles changed.  A changed tile takes a slot (one atomic per wave) and its lanes write the new values to the packed
// buffer and to the published grid, and the tile's coordinates; an unchanged tile writes nothing.  Slots are dealt in no order: the
// host sorts the coordinates.  Strips are aligned to 64 lattice cells, as both windows are, so every dword is aligned; the tiles
// of a strip outside [tx0, tx1) are not read.
__global__ __launch_bounds__(256) void k_nav_feed(NavFeedJob j, int32_t strip0, int32_t strips_x, int64_t n_strips)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= n_strips) {return;}
  const int32_t lane = threadIdx.x & 63, col = lane & 15, row0 = lane >> 4, t = col >> 2;
  const int32_t sy = (int32_t)(wave / strips_x), sx = (int32_t)(wave - (int64_t)sy * strips_x);
  const int32_t tx = (strip0 + sx) * kStripTiles + t, ty = j.ty0 + sy;
  const bool active = tx >= j.tx0 && tx < j.tx1;
  const int64_t x = (int64_t)(strip0 + sx) * (kStripTiles * kMapTile) + 4 * col, y = (int64_t)ty * kMapTile + row0;
  const uint8_t * const src = j.cells + (x - j.cells_ox) + (y - j.cells_oy) * j.cells_ws;
  int8_t * const pub = j.published + (x - j.pub_ox) + (y - j.pub_oy) * j.pub_ws;
  uint32_t nav[4] = {0, 0, 0, 0};
  uint32_t differs = 0;                                 // (bitwise, not ||: all eight loads are issued before the first is waited for)
  if (active) {
#pragma unroll
    for (int32_t k = 0; k < 4; ++k) {
      nav[k] = occ_nav4(*reinterpret_cast<const uint32_t *>(src + (int64_t)(4 * k) * j.cells_ws));
      differs |= nav[k] ^ *reinterpret_cast<const uint32_t *>(pub + (int64_t)(4 * k) * j.pub_ws);
    }
  }
  const unsigned long long changed = __ballot(differs != 0);
  uint32_t flags = 0;                                   // bit t: tile t of the strip changed (its lanes: lane & 12 == 4 t)
#pragma unroll
  for (int32_t k = 0; k < kStripTiles; ++k) {flags |= (changed & (0x000F000F000F000Full << (4 * k))) ? 1u << k : 0u;}
  if (flags == 0) {return;}                             // (the whole wave leaves: nothing of the strip is written)
  uint32_t base = 0;
  if (lane == 0) {base = atomicAdd(j.count, (uint32_t)__popc(flags));}
  base = __shfl(base, 0);
  if (!((flags >> t) & 1u)) {return;}
  const int64_t slot = (int64_t)base + __popc(flags & ((1u << t) - 1u));
  uint32_t * const out = j.packed + slot * kTileWords + (col & 3);
#pragma unroll
  for (int32_t k = 0; k < 4; ++k) {
    out[(row0 + 4 * k) * (kMapTile / 4)] = nav[k];
    *reinterpret_cast<uint32_t *>(pub + (int64_t)(4 * k) * j.pub_ws) = nav[k];
  }
  if ((lane & 0x33) == 0) {j.tile_xy[2 * slot] = tx; j.tile_xy[2 * slot + 1] = ty;}
}

}  // namespace kh

using namespace kh;

struct kh_occupancy
{
  int32_t device = 0;
  hipStream_t stream = nullptr;
  OccDev dev;
  double * d_beams = nullptr; size_t cap_beams = 0;           // kh_occupancy_add_scans' staging: device (capacity in bytes) ...
  double * h_beams = nullptr; size_t cap_hbeams = 0;          // ... and pinned host memory (capacity in doubles)
  hipEvent_t ev[2] = {nullptr, nullptr};
  double trace_ms = 0.0; int64_t beams_traced = 0;
  ResidentScan * d_scans = nullptr; size_t cap_scans = 0;     // kh::occupancy_add_resident's table (capacity in bytes)
  uint8_t * d_merge = nullptr; size_t cap_merge = 0;          // kh::occupancy_add_merged's two tables (submaps, then scans; bytes)
  uint32_t * d_nav = nullptr; size_t cap_nav = 0;             // kh_occupancy_read_nav's dense output (capacity in bytes)
  uint8_t * d_fit = nullptr; size_t cap_fit = 0;              // kh::occupancy_fit_merged's sums and three tables (bytes)
};

namespace kh
{
namespace
{
// one wave per run of 64 beams, four waves per workgroup
dim3 blocks_of_runs(int32_t n_scans, int32_t runs_per_scan) {return dim3(static_cast<unsigned>((static_cast<int64_t>(n_scans) * runs_per_scan + 3) / 4));}

// What every AddScan route ends with: the trace kernel between two events, the wait for it, a failure reported under the caller's
// (`who`) name, the grid's trace time and beam counter.
template <typename Launch>
int timed_trace(kh_occupancy * g, const char * who, int64_t n_beams, Launch launch)
{
  (void)hipEventRecord(g->ev[0], g->stream);
  launch();
  (void)hipEventRecord(g->ev[1], g->stream);
  if (hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
  g->trace_ms += ms; g->beams_traced += n_beams;
  return KH_OK;
}
}  // namespace

void * occupancy_stream(kh_occupancy * g) {return g ? g->stream : nullptr;}

int occupancy_add_resident(kh_occupancy * g, int32_t n_scans, const ResidentScan * scans, int32_t n_beams, double range_threshold,
  double min_range, double max_range)
{
  if (!g || n_scans < 0 || n_beams < 0 || (n_scans > 0 && !scans)) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  if (n_scans == 0 || n_beams == 0) {return hipStreamSynchronize(g->stream) == hipSuccess ? KH_OK : KH_ERR_HIP;}
  const size_t bytes = static_cast<size_t>(n_scans) * sizeof(ResidentScan);
  if (!grow_device(g->stream, reinterpret_cast<void **>(&g->d_scans), &g->cap_scans, bytes, bytes + bytes / 2)) {
    set_error("kh_mapper_build_map: scan table allocation failed");
    return KH_ERR_HIP;
  }
  if (hipMemcpyAsync(g->d_scans, scans, bytes, hipMemcpyHostToDevice, g->stream) != hipSuccess) {
    (void)hipStreamSynchronize(g->stream);
    return KH_ERR_HIP;
  }
  const int32_t runs = (n_beams + 63) / 64;
  return timed_trace(g, "kh_mapper_build_map", static_cast<int64_t>(n_scans) * n_beams, [&] {
    hipLaunchKernelGGL(k_occ_trace_resident, blocks_of_runs(n_scans, runs), dim3(256), 0, g->stream, g->dev, g->d_scans, n_scans, n_beams, runs,
      range_threshold, min_range, max_range);
  });
}

int occupancy_add_merged(kh_occupancy * g, int32_t n_scans, const MergeScan * scans, int32_t n_submaps, const MergeSubmap * submaps,
  int32_t max_beams, int64_t n_total_beams)
{
  if (!g || n_scans < 0 || n_submaps < 0 || max_beams < 0 || (n_scans > 0 && (!scans || !submaps || n_submaps == 0))) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  if (n_scans == 0 || max_beams == 0) {return hipStreamSynchronize(g->stream) == hipSuccess ? KH_OK : KH_ERR_HIP;}
  const size_t submap_bytes = static_cast<size_t>(n_submaps) * sizeof(MergeSubmap), scan_bytes = static_cast<size_t>(n_scans) * sizeof(MergeScan);
  if (!grow_device(g->stream, reinterpret_cast<void **>(&g->d_merge), &g->cap_merge, submap_bytes + scan_bytes, submap_bytes + scan_bytes)) {
    set_error("kh_merge_build: table allocation failed");
    return KH_ERR_HIP;
  }
  const MergeSubmap * d_submaps = reinterpret_cast<const MergeSubmap *>(g->d_merge);
  const MergeScan * d_scans = reinterpret_cast<const MergeScan *>(g->d_merge + submap_bytes);      // (64 * n_submaps: 8-byte aligned)
  if (hipMemcpyAsync(g->d_merge, submaps, submap_bytes, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
    hipMemcpyAsync(g->d_merge + submap_bytes, scans, scan_bytes, hipMemcpyHostToDevice, g->stream) != hipSuccess)
  {
    (void)hipStreamSynchronize(g->stream);
    return KH_ERR_HIP;
  }
  const int32_t runs = (max_beams + 63) / 64;
  return timed_trace(g, "kh_merge_build", n_total_beams, [&] {
    hipLaunchKernelGGL(k_occ_trace_merged, blocks_of_runs(n_scans, runs), dim3(256), 0, g->stream, g->dev, d_scans, d_submaps, n_scans, runs);
  });
}

int occupancy_fit_merged(kh_occupancy * g, int32_t n_candidates, const FitCandidate * candidates, const FitSensor * sensors, int32_t n_scans,
  const ResidentScan * scans, int32_t n_beams, double range_threshold, double min_range, double max_range, uint64_t * out, double * kernel_ms)
{
  if (!g || n_candidates < 1 || !candidates || !out || n_scans < 0 || n_beams < 0 || (n_scans > 0 && (!scans || !sensors))) {return KH_ERR_INVALID_ARG;}
  if (kernel_ms) {*kernel_ms = 0.0;}
  std::fill(out, out + static_cast<size_t>(n_candidates) * kFitCounters, uint64_t{0});
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  if (n_scans == 0 || n_beams == 0) {return hipStreamSynchronize(g->stream) == hipSuccess ? KH_OK : KH_ERR_HIP;}
  const int32_t runs = (n_beams + 63) / 64;
  const int64_t blocks_per_candidate = (static_cast<int64_t>(n_scans) * runs + 3) / 4;
  if (blocks_per_candidate * n_candidates > INT32_MAX) {set_error("kh_merge_fit: too many candidates for one launch"); return KH_ERR_INVALID_ARG;}
  // the sums first, then the tables: every part a multiple of 8 bytes
  const size_t out_bytes = static_cast<size_t>(n_candidates) * kFitCounters * sizeof(unsigned long long);
  const size_t cand_bytes = static_cast<size_t>(n_candidates) * sizeof(FitCandidate);
  const size_t sensor_bytes = static_cast<size_t>(n_candidates) * static_cast<size_t>(n_scans) * sizeof(FitSensor);
  const size_t scan_bytes = static_cast<size_t>(n_scans) * sizeof(ResidentScan);
  const size_t bytes = out_bytes + cand_bytes + sensor_bytes + scan_bytes;
  if (!grow_device(g->stream, reinterpret_cast<void **>(&g->d_fit), &g->cap_fit, bytes, bytes)) {
    set_error("kh_merge_fit: table allocation failed");
    return KH_ERR_HIP;
  }
  unsigned long long * d_out = reinterpret_cast<unsigned long long *>(g->d_fit);
  uint8_t * const d_cand = g->d_fit + out_bytes, * const d_sensors = d_cand + cand_bytes, * const d_scans = d_sensors + sensor_bytes;
  if (hipMemsetAsync(d_out, 0, out_bytes, g->stream) != hipSuccess ||
    hipMemcpyAsync(d_cand, candidates, cand_bytes, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
    hipMemcpyAsync(d_sensors, sensors, sensor_bytes, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
    hipMemcpyAsync(d_scans, scans, scan_bytes, hipMemcpyHostToDevice, g->stream) != hipSuccess)
  {
    (void)hipStreamSynchronize(g->stream);
    return KH_ERR_HIP;
  }
  (void)hipEventRecord(g->ev[0], g->stream);
  hipLaunchKernelGGL(k_occ_fit_merged, dim3(static_cast<unsigned>(blocks_per_candidate * n_candidates)), dim3(256), 0, g->stream, g->dev,
    reinterpret_cast<const ResidentScan *>(d_scans), reinterpret_cast<const FitCandidate *>(d_cand), reinterpret_cast<const FitSensor *>(d_sensors),
    n_scans, n_beams, runs, static_cast<int32_t>(blocks_per_candidate), range_threshold, min_range, max_range, d_out);
  (void)hipEventRecord(g->ev[1], g->stream);
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the sums are downloaded as they lie");
  if (hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error(std::string("kh_merge_fit: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
  if (kernel_ms) {*kernel_ms = ms;}
  return KH_OK;
}

void live_trace_delta(void * stream, const LiveWindow & w, double anchor_x, double anchor_y, double scale, const DeltaRecord * d_records,
  int32_t n_records, int32_t n_beams, double range_threshold, double min_range, double max_range, int32_t * d_log,
  unsigned long long * d_counters)
{
  if (n_records <= 0 || n_beams <= 0) {return;}
  const int32_t runs = (n_beams + 63) / 64;
  hipLaunchKernelGGL(k_occ_trace_delta, blocks_of_runs(n_records, runs), dim3(256), 0, static_cast<hipStream_t>(stream), w, anchor_x, anchor_y,
    scale, d_records, n_records, n_beams, runs, range_threshold, min_range, max_range, d_log, live_log_slot_words(n_beams), d_counters);
}

void live_update_cells(void * stream, const LiveWindow & w, int32_t x0, int32_t y0, int32_t rect_w, int32_t rect_h, uint32_t min_pass,
  double threshold)
{
  if (rect_w <= 0 || rect_h <= 0) {return;}
  const int64_t size = static_cast<int64_t>(rect_w) * rect_h;
  hipLaunchKernelGGL(k_occ_update_rect, dim3(static_cast<unsigned>((size + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w, x0, y0,
    rect_w, rect_h, min_pass, threshold);
}

void nav_feed(void * stream, const NavFeedJob & job)
{
  if (job.tx1 <= job.tx0 || job.ty1 <= job.ty0) {return;}
  // the strips of 4 tiles that hold tile columns [tx0, tx1): floor quotients, tiles left of the anchor are negative
  const int32_t strip0 = static_cast<int32_t>(floor_div(job.tx0, kStripTiles));
  const int32_t strips_x = static_cast<int32_t>(floor_div(job.tx1 - 1, kStripTiles)) - strip0 + 1;
  const int64_t n_strips = static_cast<int64_t>(strips_x) * (job.ty1 - job.ty0);
  hipLaunchKernelGGL(k_nav_feed, dim3(static_cast<unsigned>((n_strips + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), job, strip0,
    strips_x, n_strips);
}

struct MapWork
{
  int32_t device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  uint8_t * d = nullptr; size_t cap = 0;               // the launch's tables and answers (bytes)
};

MapWork * map_work_create(int32_t device)
{
  MapWork * w = new MapWork();
  w->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess ||
    hipEventCreate(&w->ev[0]) != hipSuccess || hipEventCreate(&w->ev[1]) != hipSuccess)
  {
    (void)hipGetLastError();
    set_error("map view: HIP stream / event creation failed");
    map_work_destroy(w);
    return nullptr;
  }
  return w;
}

void map_work_destroy(MapWork * w)
{
  if (!w) {return;}
  (void)hipSetDevice(w->device);
  if (w->stream) {(void)hipStreamSynchronize(w->stream);}
  (void)hipFree(w->d);
  if (w->ev[0]) {(void)hipEventDestroy(w->ev[0]);}
  if (w->ev[1]) {(void)hipEventDestroy(w->ev[1]);}
  if (w->stream) {(void)hipStreamDestroy(w->stream);}
  delete w;
}

int map_view_check(const kh_map_view * v)
{
  if (!v || !v->device_cells || v->width <= 0 || v->height <= 0 || v->width_step < v->width || !std::isfinite(v->scale) || !(v->scale > 0.0) ||
    !std::isfinite(v->anchor[0]) || !std::isfinite(v->anchor[1]))
  {
    set_error("malformed map view");
    return KH_ERR_INVALID_ARG;
  }
  if (static_cast<int64_t>(v->width_step) * v->height > (1ll << 31) - 4096) {set_error("map view too large"); return KH_ERR_INVALID_ARG;}
  if (static_cast<int64_t>(v->ox) + v->width > INT32_MAX || static_cast<int64_t>(v->oy) + v->height > INT32_MAX) {
    set_error("map view: the window leaves the int32 lattice");
    return KH_ERR_INVALID_ARG;
  }
  return KH_OK;
}

namespace
{
MapWindow window_of(const kh_map_view & v)
{
  return MapWindow{v.device_cells, v.ox, v.oy, v.width, v.height, v.width_step, v.anchor[0], v.anchor[1], v.scale};
}

// the time between the work's two events, once its stream has drained; a failure is reported under `who`
int finish_timed(MapWork * w, const char * who, double * kernel_ms)
{
  if (hipStreamSynchronize(w->stream) != hipSuccess) {
    set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w->ev[0], w->ev[1]);
  if (kernel_ms) {*kernel_ms = ms;}
  return KH_OK;
}
}  // namespace

int map_seed_blocks(MapWork * w, const kh_map_view & v, int32_t pitch, int64_t bx0, int64_t by0, int64_t nbx, int64_t nby, int32_t * local,
  double * kernel_ms)
{
  if (kernel_ms) {*kernel_ms = 0.0;}
  const int64_t n_blocks = nbx * nby;
  if (!w || pitch < 1 || nbx < 1 || nby < 1 || !local || n_blocks > (1ll << 31) - 4096) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(w->device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t bytes = static_cast<size_t>(n_blocks) * sizeof(int32_t);
  if (!grow_device(w->stream, reinterpret_cast<void **>(&w->d), &w->cap, bytes, bytes)) {
    set_error("kh_map_seeds: block table allocation failed");
    return KH_ERR_HIP;
  }
  (void)hipEventRecord(w->ev[0], w->stream);
  hipLaunchKernelGGL(k_map_seeds, dim3(static_cast<unsigned>((n_blocks + 3) / 4)), dim3(256), 0, w->stream, window_of(v), pitch, bx0, by0, nbx,
    n_blocks, reinterpret_cast<int32_t *>(w->d));
  (void)hipEventRecord(w->ev[1], w->stream);
  if (hipMemcpyAsync(local, w->d, bytes, hipMemcpyDeviceToHost, w->stream) != hipSuccess) {
    (void)hipStreamSynchronize(w->stream);
    return KH_ERR_HIP;
  }
  return finish_timed(w, "kh_map_seeds", kernel_ms);
}

int map_fit_counts(MapWork * w, const kh_map_view & v, int32_t n_beams, const double * ranges, int32_t n_poses, const double * points,
  const double * sensor_xy, double range_threshold, double min_range, double max_range, uint64_t * counts, double * kernel_ms)
{
  if (kernel_ms) {*kernel_ms = 0.0;}
  if (!w || n_beams < 0 || n_poses < 1 || !counts || (n_beams > 0 && (!ranges || !points)) || !sensor_xy) {return KH_ERR_INVALID_ARG;}
  std::fill(counts, counts + static_cast<size_t>(n_poses) * kFitCounters, uint64_t{0});
  if (n_beams == 0) {return KH_OK;}
  const int64_t blocks_per_pose = ((static_cast<int64_t>(n_beams) + 63) / 64 + 3) / 4;
  if (blocks_per_pose * n_poses > INT32_MAX) {set_error("kh_map_fit: too many poses for one launch"); return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(w->device) != hipSuccess) {return KH_ERR_HIP;}
  // the sums first, then the tables: every part a multiple of 8 bytes
  const size_t out_bytes = static_cast<size_t>(n_poses) * kFitCounters * sizeof(unsigned long long);
  const size_t sensor_bytes = static_cast<size_t>(n_poses) * 2 * sizeof(double);
  const size_t range_bytes = static_cast<size_t>(n_beams) * sizeof(double);
  const size_t point_bytes = static_cast<size_t>(n_poses) * static_cast<size_t>(n_beams) * 2 * sizeof(double);
  const size_t bytes = out_bytes + sensor_bytes + range_bytes + point_bytes;
  if (!grow_device(w->stream, reinterpret_cast<void **>(&w->d), &w->cap, bytes, bytes + bytes / 2)) {
    set_error("kh_map_fit: table allocation failed");
    return KH_ERR_HIP;
  }
  unsigned long long * d_out = reinterpret_cast<unsigned long long *>(w->d);
  uint8_t * const d_sensors = w->d + out_bytes, * const d_ranges = d_sensors + sensor_bytes, * const d_points = d_ranges + range_bytes;
  if (hipMemsetAsync(d_out, 0, out_bytes, w->stream) != hipSuccess ||
    hipMemcpyAsync(d_sensors, sensor_xy, sensor_bytes, hipMemcpyHostToDevice, w->stream) != hipSuccess ||
    hipMemcpyAsync(d_ranges, ranges, range_bytes, hipMemcpyHostToDevice, w->stream) != hipSuccess ||
    hipMemcpyAsync(d_points, points, point_bytes, hipMemcpyHostToDevice, w->stream) != hipSuccess)
  {
    (void)hipStreamSynchronize(w->stream);
    return KH_ERR_HIP;
  }
  (void)hipEventRecord(w->ev[0], w->stream);
  hipLaunchKernelGGL(k_map_fit, dim3(static_cast<unsigned>(blocks_per_pose * n_poses)), dim3(256), 0, w->stream, window_of(v),
    reinterpret_cast<const double *>(d_ranges), reinterpret_cast<const double *>(d_points), reinterpret_cast<const double *>(d_sensors), n_beams,
    static_cast<int32_t>(blocks_per_pose), range_threshold, min_range, max_range, d_out);
  (void)hipEventRecord(w->ev[1], w->stream);
  if (hipMemcpyAsync(counts, d_out, out_bytes, hipMemcpyDeviceToHost, w->stream) != hipSuccess) {
    (void)hipStreamSynchronize(w->stream);
    return KH_ERR_HIP;
  }
  return finish_timed(w, "kh_map_fit", kernel_ms);
}

int map_raycast_cells(MapWork * w, const kh_map_view & v, int32_t n_beams, int32_t n_poses, const double * points, const double * sensor_xy,
  int32_t max_unknown, RayCell * out, double * kernel_ms)
{
  if (kernel_ms) {*kernel_ms = 0.0;}
  if (!w || n_beams < 1 || n_poses < 1 || !points || !sensor_xy || !out || max_unknown < -1) {return KH_ERR_INVALID_ARG;}
  const int64_t blocks_per_pose = ((static_cast<int64_t>(n_beams) + 63) / 64 + 3) / 4;
  if (blocks_per_pose * n_poses > INT32_MAX) {set_error("kh_map_raycast: too many poses for one launch"); return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(w->device) != hipSuccess) {return KH_ERR_HIP;}
  // the answers first, then the tables: every part a multiple of 16 bytes
  const size_t out_bytes = static_cast<size_t>(n_poses) * static_cast<size_t>(n_beams) * sizeof(RayCell);
  const size_t sensor_bytes = static_cast<size_t>(n_poses) * 2 * sizeof(double);
  const size_t point_bytes = static_cast<size_t>(n_poses) * static_cast<size_t>(n_beams) * 2 * sizeof(double);
  const size_t bytes = out_bytes + sensor_bytes + point_bytes;
  if (!grow_device(w->stream, reinterpret_cast<void **>(&w->d), &w->cap, bytes, bytes + bytes / 2)) {
    set_error("kh_map_raycast: table allocation failed");
    return KH_ERR_HIP;
  }
  uint8_t * const d_sensors = w->d + out_bytes, * const d_points = d_sensors + sensor_bytes;
  if (hipMemcpyAsync(d_sensors, sensor_xy, sensor_bytes, hipMemcpyHostToDevice, w->stream) != hipSuccess ||
    hipMemcpyAsync(d_points, points, point_bytes, hipMemcpyHostToDevice, w->stream) != hipSuccess)
  {
    (void)hipStreamSynchronize(w->stream);
    return KH_ERR_HIP;
  }
  (void)hipEventRecord(w->ev[0], w->stream);
  hipLaunchKernelGGL(k_map_raycast, dim3(static_cast<unsigned>(blocks_per_pose * n_poses)), dim3(256), 0, w->stream, window_of(v),
    reinterpret_cast<const double *>(d_points), reinterpret_cast<const double *>(d_sensors), n_beams, static_cast<int32_t>(blocks_per_pose),
    max_unknown, reinterpret_cast<RayCell *>(w->d));
  (void)hipEventRecord(w->ev[1], w->stream);
  if (hipMemcpyAsync(out, w->d, out_bytes, hipMemcpyDeviceToHost, w->stream) != hipSuccess) {
    (void)hipStreamSynchronize(w->stream);
    return KH_ERR_HIP;
  }
  return finish_timed(w, "kh_map_raycast", kernel_ms);
}

int map_raycast_check(const kh_map_view * view, const kh_laser * laser, int32_t n_poses, const double * sensor_poses, int32_t max_unknown)
{
  if (!laser || !sensor_poses || n_poses < 1 || max_unknown < -1 || laser->n_beams < 1 || map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (!fit_laser_ok(laser->range_threshold, laser->minimum_range, laser->maximum_range, view->scale) || !std::isfinite(laser->minimum_angle) ||
    !std::isfinite(laser->angular_resolution))
  {
    set_error("kh_map_raycast: the laser's range_threshold * scale must stay below 2^20 cells, its other fields must be numbers");
    return KH_ERR_INVALID_ARG;
  }
  for (int32_t k = 0; k < n_poses; ++k) {
    if (!fit_pose_ok(sensor_poses + 3 * static_cast<size_t>(k), view->anchor[0], view->anchor[1], view->scale)) {
      set_error("kh_map_raycast: pose " + std::to_string(k) + " is not finite or lies more than 2^30 cells from the anchor");
      return KH_ERR_INVALID_ARG;
    }
  }
  return KH_OK;
}

int map_raycast(MapWork * w, const kh_map_view & v, const kh_laser & laser, int32_t n_poses, const double * sensor_poses, int32_t max_unknown,
  double no_return, kh_ray_t * out, double * kernel_ms)
{
  const size_t nb = static_cast<size_t>(laser.n_beams), np = static_cast<size_t>(n_poses);
  const std::vector<double> far(nb, laser.range_threshold);
  std::vector<double> points(2 * nb * np), sensor_xy(2 * np);
  host_parallel_for_wide(np, [&](size_t k) {
    kh_scan_points(far.data(), laser.n_beams, sensor_poses + 3 * k, laser.minimum_angle, laser.angular_resolution, &points[2 * nb * k]);
    sensor_xy[2 * k] = sensor_poses[3 * k]; sensor_xy[2 * k + 1] = sensor_poses[3 * k + 1];
  });
  std::vector<RayCell> cells(nb * np);
  const int rc = map_raycast_cells(w, v, laser.n_beams, n_poses, points.data(), sensor_xy.data(), max_unknown, cells.data(), kernel_ms);
  if (rc) {return rc;}
  for (size_t k = 0; k < np; ++k) {
    const double sx = sensor_xy[2 * k], sy = sensor_xy[2 * k + 1];
    for (size_t b = 0; b < nb; ++b) {
      const RayCell & c = cells[k * nb + b];
      kh_ray_t & r = out[k * nb + b];
      r.cell[0] = c.i; r.cell[1] = c.j; r.steps = c.steps; r.code = c.code;
      r.range = no_return;
      if (c.code == KH_RAY_HIT) {         // to the hit cell's centre
        const double dx = (v.anchor[0] + static_cast<double>(c.i) / v.scale) - sx, dy = (v.anchor[1] + static_cast<double>(c.j) / v.scale) - sy;
        r.range = std::sqrt((dx * dx) + (dy * dy));
      }
    }
  }
  return KH_OK;
}

void map_observe(void * stream, const kh_map_view & v, const ChangeLayer & layer, const double * d_ranges, const double * d_points,
  const double * d_sensors, int32_t n_scans, int32_t n_beams, double range_threshold, double min_range, double max_range, int32_t tolerance,
  int32_t * d_labels)
{
  if (n_scans <= 0 || n_beams <= 0) {return;}
  const int64_t blocks_per_scan = ((static_cast<int64_t>(n_beams) + 63) / 64 + 3) / 4;
  hipLaunchKernelGGL(k_map_observe, dim3(static_cast<unsigned>(blocks_per_scan * n_scans)), dim3(256), 0, static_cast<hipStream_t>(stream),
    window_of(v), layer, d_ranges, d_points, d_sensors, n_beams, static_cast<int32_t>(blocks_per_scan), range_threshold, min_range, max_range,
    tolerance, reinterpret_cast<int2 *>(d_labels));
}

void map_decay(void * stream, const kh_map_view & v, const ChangeLayer & layer, int32_t shift)
{
  const int64_t size = static_cast<int64_t>(v.width_step) * v.height;
  hipLaunchKernelGGL(k_map_decay, dim3(static_cast<unsigned>((size + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), layer, size, shift);
}

void map_diff(void * stream, const kh_map_view & v, const ChangeLayer & layer, uint32_t min_pass, double threshold, uint8_t * d_codes,
  uint8_t * d_patched, unsigned long long * d_counts)
{
  const int64_t size = static_cast<int64_t>(v.width_step) * v.height;
  hipLaunchKernelGGL(k_map_diff, dim3(static_cast<unsigned>((size + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), window_of(v), layer,
    min_pass, threshold, d_codes, d_patched, d_counts);
}

void map_changed_cells(void * stream, const kh_map_view & v, const uint8_t * d_codes, int32_t * d_unit, int32_t * d_list, int32_t cap)
{
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int32_t units_per_row = (v.width + 63) / 64;
  const int64_t n_units = change_units(v.width, v.height);
  const dim3 blocks(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n_units + 3) / 4, 1024))));
  hipLaunchKernelGGL(k_map_changed<false>, blocks, dim3(256), 0, s, window_of(v), d_codes, units_per_row, n_units, d_unit, d_list, cap);
  hipLaunchKernelGGL(k_map_changed_scan, dim3(1), dim3(1024), 0, s, d_unit, n_units);
  if (cap > 0) {hipLaunchKernelGGL(k_map_changed<true>, blocks, dim3(256), 0, s, window_of(v), d_codes, units_per_row, n_units, d_unit, d_list, cap);}
}

void cells_to_nav(void * stream, const uint8_t * d_cells, int32_t width, int32_t height, int32_t ws, uint32_t * d_out)
{
  const int64_t total = static_cast<int64_t>(width) * height, words = (total + 3) / 4;
  hipLaunchKernelGGL(k_occ_to_nav, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_cells, width,
    ws, total, d_out);
}
}  // namespace kh

extern "C" {

int kh_occupancy_compute_dimensions(
  int32_t n_scans, const kh_scan * scans, double min_range, double range_threshold, double resolution,
  int32_t * width, int32_t * height, double offset[2])
{
  if (n_scans <= 0 || !scans || !width || !height || !offset || !(resolution > 0)) {return KH_ERR_INVALID_ARG;}
  // BoundingBox2 (Karto.h:2846-2903) over every scan's box = sensor position + in-range points (Karto.h:5694-5700)
  Box box;
  for (int32_t s = 0; s < n_scans; ++s) {
    if (scans[s].n < 0 || (scans[s].n > 0 && (!scans[s].ranges || !scans[s].points_xy))) {return KH_ERR_INVALID_ARG;}
    box.add(scans[s].sensor_pose[0], scans[s].sensor_pose[1]);
    for (int32_t i = 0; i < scans[s].n; ++i) {
      const double r = scans[s].ranges[i];
      if (r >= min_range && r <= range_threshold) {box.add(scans[s].points_xy[2 * i], scans[s].points_xy[2 * i + 1]);}   // math::InRange
    }
  }
  grid_dimensions(box, resolution, width, height, offset);
  return KH_OK;
}

int kh_occupancy_create(int32_t width, int32_t height, double offset_x, double offset_y, double resolution,
  int32_t device, kh_occupancy ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (width <= 0 || height <= 0 || !(resolution > 0) || grid_too_large(width, height)) {
    set_error("OccupancyGrid: invalid dimensions");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_occupancy * g = new kh_occupancy();
  g->device = device;
  g->dev.width = width; g->dev.height = height; g->dev.ws = (width + 7) & ~7;      // Karto.h:4640
  g->dev.off_x = offset_x; g->dev.off_y = offset_y; g->dev.scale = 1.0 / resolution;
  g->dev.pass = nullptr; g->dev.hits = nullptr; g->dev.cells = nullptr;
  const size_t size = static_cast<size_t>(g->dev.ws) * height;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
    hipEventCreate(&g->ev[0]) != hipSuccess || hipEventCreate(&g->ev[1]) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&g->dev.pass), size * 4) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&g->dev.hits), size * 4) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&g->dev.cells), size) != hipSuccess ||
    hipMemset(g->dev.pass, 0, size * 4) != hipSuccess || hipMemset(g->dev.hits, 0, size * 4) != hipSuccess ||
    hipMemset(g->dev.cells, 0, size) != hipSuccess ||
    // (the fills may still be in flight on the null stream, and the grid's own stream does not wait for that one: a write queued
    // there right after the create -- kh_occupancy_write_nav's small kernel -- must not be overtaken by them)
    hipStreamSynchronize(nullptr) != hipSuccess)
  {
    set_error("kh_occupancy_create: HIP allocation failed");
    kh_occupancy_destroy(g);
    return KH_ERR_HIP;
  }
  *out = g;
  return KH_OK;
}

void kh_occupancy_destroy(kh_occupancy * g)
{
  if (!g) {return;}
  (void)hipSetDevice(g->device);
  if (g->stream) {(void)hipStreamSynchronize(g->stream);}
  (void)hipFree(g->dev.pass); (void)hipFree(g->dev.hits); (void)hipFree(g->dev.cells); (void)hipFree(g->d_beams); (void)hipFree(g->d_scans); (void)hipFree(g->d_merge);
  (void)hipFree(g->d_nav); (void)hipFree(g->d_fit);
  if (g->h_beams) {(void)hipHostFree(g->h_beams);}
  if (g->ev[0]) {(void)hipEventDestroy(g->ev[0]);}
  if (g->ev[1]) {(void)hipEventDestroy(g->ev[1]);}
  if (g->stream) {(void)hipStreamDestroy(g->stream);}
  delete g;
}

int kh_occupancy_clear(kh_occupancy * g)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t size = static_cast<size_t>(g->dev.ws) * g->dev.height;
  if (hipMemsetAsync(g->dev.pass, 0, size * 4, g->stream) != hipSuccess || hipMemsetAsync(g->dev.hits, 0, size * 4, g->stream) != hipSuccess ||
    hipMemsetAsync(g->dev.cells, 0, size, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) {return KH_ERR_HIP;}
  return KH_OK;
}

int kh_occupancy_add_scans(kh_occupancy * g, int32_t n_scans, const kh_scan * scans, double range_threshold,
  double min_range, double max_range)
{
  if (!g || n_scans < 0 || (n_scans > 0 && !scans)) {return KH_ERR_INVALID_ARG;}
  if (n_scans == 0) {return KH_OK;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  size_t total = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    if (scans[s].n < 0 || (scans[s].n > 0 && (!scans[s].ranges || !scans[s].points_xy))) {return KH_ERR_INVALID_ARG;}
    total += static_cast<size_t>(scans[s].n);
  }
  if (total == 0) {return KH_OK;}
  if (total * 5 > g->cap_hbeams) {
    if (g->h_beams) {(void)hipStreamSynchronize(g->stream); (void)hipHostFree(g->h_beams); g->h_beams = nullptr;}
    const size_t cap = std::max(total * 5, g->cap_hbeams + g->cap_hbeams / 2);
    g->cap_hbeams = 0; g->cap_beams = 0;                      // (the device buffer follows the host buffer's size)
    if (hipHostMalloc(reinterpret_cast<void **>(&g->h_beams), cap * 8, hipHostMallocDefault) != hipSuccess ||
      !grow_device(g->stream, reinterpret_cast<void **>(&g->d_beams), &g->cap_beams, cap * 8, cap * 8))
    {
      set_error("kh_occupancy_add_scans: staging allocation failed");
      return KH_ERR_HIP;
    }
    g->cap_hbeams = cap;
  }
  size_t k = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    const double sx = scans[s].sensor_pose[0], sy = scans[s].sensor_pose[1];
    for (int32_t i = 0; i < scans[s].n; ++i, ++k) {
      double * b = g->h_beams + 5 * k;
      b[0] = scans[s].ranges[i]; b[1] = scans[s].points_xy[2 * i]; b[2] = scans[s].points_xy[2 * i + 1]; b[3] = sx; b[4] = sy;
    }
  }
  if (hipMemcpyAsync(g->d_beams, g->h_beams, total * 5 * 8, hipMemcpyHostToDevice, g->stream) != hipSuccess) {return KH_ERR_HIP;}
  return timed_trace(g, "kh_occupancy_add_scans", static_cast<int64_t>(total), [&] {
    hipLaunchKernelGGL(k_occ_trace, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, g->stream, g->dev, g->d_beams,
      static_cast<int64_t>(total), range_threshold, min_range, max_range);
  });
}

int kh_occupancy_update(kh_occupancy * g, uint32_t min_pass_through, double occupancy_threshold)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  const int64_t size = static_cast<int64_t>(g->dev.ws) * g->dev.height;
  hipLaunchKernelGGL(k_occ_update, dim3(static_cast<unsigned>((size + 255) / 256)), dim3(256), 0, g->stream, g->dev,
    min_pass_through, occupancy_threshold);
  if (hipStreamSynchronize(g->stream) != hipSuccess) {return KH_ERR_HIP;}
  return KH_OK;
}

int kh_occupancy_read(kh_occupancy * g, uint8_t * cells, uint32_t * pass, uint32_t * hits)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t size = static_cast<size_t>(g->dev.ws) * g->dev.height;
  if (cells && hipMemcpy(cells, g->dev.cells, size, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  if (pass && hipMemcpy(pass, g->dev.pass, size * 4, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  if (hits && hipMemcpy(hits, g->dev.hits, size * 4, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  return KH_OK;
}

int kh_occupancy_read_nav(kh_occupancy * g, int8_t * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  const int64_t total = static_cast<int64_t>(g->dev.width) * g->dev.height, words = (total + 3) / 4;
  if (!grow_device(g->stream, reinterpret_cast<void **>(&g->d_nav), &g->cap_nav, static_cast<size_t>(words) * 4, static_cast<size_t>(words) * 4)) {
    set_error("kh_occupancy_read_nav: output allocation failed");
    return KH_ERR_HIP;
  }
  hipLaunchKernelGGL(k_occ_to_nav, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, g->stream, g->dev.cells, g->dev.width,
    g->dev.ws, total, g->d_nav);
  if (hipMemcpyAsync(out, g->d_nav, static_cast<size_t>(total), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipStreamSynchronize(g->stream) != hipSuccess)
  {
    set_error(std::string("kh_occupancy_read_nav: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  return KH_OK;
}

int kh_occupancy_info(kh_occupancy * g, int32_t * width, int32_t * height, int32_t * width_step, double * trace_ms, int64_t * beams)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (width) {*width = g->dev.width;}
  if (height) {*height = g->dev.height;}
  if (width_step) {*width_step = g->dev.ws;}
  if (trace_ms) {*trace_ms = g->trace_ms;}
  if (beams) {*beams = g->beams_traced;}
  return KH_OK;
}

int kh_occupancy_geometry(kh_occupancy * g, double offset[2], double * resolution)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (offset) {offset[0] = g->dev.off_x; offset[1] = g->dev.off_y;}
  if (resolution) {*resolution = 1.0 / g->dev.scale;}
  return KH_OK;
}

int kh_occupancy_view(kh_occupancy * g, kh_map_view * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  out->device_cells = g->dev.cells; out->device = g->device;
  out->width = g->dev.width; out->height = g->dev.height; out->width_step = g->dev.ws;
  out->ox = 0; out->oy = 0;
  out->anchor[0] = g->dev.off_x; out->anchor[1] = g->dev.off_y; out->scale = g->dev.scale;
  return KH_OK;
}

int kh_map_seeds(const kh_map_view * view, double seed_spacing, const double * center_xy, double radius, int32_t * cells, double * xy,
  int32_t cap, int32_t * n_seeds)
{
  if (!n_seeds || cap < 0) {return KH_ERR_INVALID_ARG;}
  *n_seeds = 0;
  if (map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (!std::isfinite(radius) || (center_xy && (!std::isfinite(center_xy[0]) || !std::isfinite(center_xy[1])))) {
    set_error("kh_map_seeds: the region must be finite");
    return KH_ERR_INVALID_ARG;
  }
  const int32_t pitch = seed_pitch(seed_spacing, view->scale);
  if (pitch == 0) {
    set_error("kh_map_seeds: seed_spacing must be finite, > 0 and at most " + std::to_string(kMaxSeedPitch) + " cells");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(view->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  const SeedBlocks blocks = seed_blocks(view->ox, view->oy, view->width, view->height, pitch);
  MapWork * w = map_work_create(view->device);
  if (!w) {return KH_ERR_HIP;}
  std::vector<int32_t> local(static_cast<size_t>(blocks.count()));
  const int rc = map_seed_blocks(w, *view, pitch, blocks.bx0, blocks.by0, blocks.nx, blocks.ny, local.data(), nullptr);
  map_work_destroy(w);
  if (rc) {return rc;}
  const std::vector<Seed> seeds = compact_seeds(blocks, pitch, local.data(), view->anchor[0], view->anchor[1], view->scale, center_xy, radius);
  if (seeds.size() > static_cast<size_t>(INT32_MAX)) {set_error("kh_map_seeds: more than 2^31 seeds"); return KH_ERR_INVALID_ARG;}
  for (size_t k = 0; k < seeds.size() && k < static_cast<size_t>(cap); ++k) {
    if (cells) {cells[2 * k] = seeds[k].i; cells[2 * k + 1] = seeds[k].j;}
    if (xy) {xy[2 * k] = seeds[k].x; xy[2 * k + 1] = seeds[k].y;}
  }
  *n_seeds = static_cast<int32_t>(seeds.size());
  return KH_OK;
}

int kh_map_fit(const kh_map_view * view, const kh_laser * laser, const double * ranges, int32_t n_poses, const double * sensor_poses,
  kh_merge_fit_t * out)
{
  if (!laser || !ranges || !sensor_poses || !out || n_poses < 1 || laser->n_beams < 1 || map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (!fit_laser_ok(laser->range_threshold, laser->minimum_range, laser->maximum_range, view->scale) || !std::isfinite(laser->minimum_angle) ||
    !std::isfinite(laser->angular_resolution))
  {
    set_error("kh_map_fit: the laser's range_threshold * scale must stay below 2^20 cells, its other fields must be numbers");
    return KH_ERR_INVALID_ARG;
  }
  for (int32_t k = 0; k < n_poses; ++k) {
    if (!fit_pose_ok(sensor_poses + 3 * static_cast<size_t>(k), view->anchor[0], view->anchor[1], view->scale)) {
      set_error("kh_map_fit: pose " + std::to_string(k) + " is not finite or lies more than 2^30 cells from the anchor");
      return KH_ERR_INVALID_ARG;
    }
  }
  if (require_device(view->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  const size_t nb = static_cast<size_t>(laser->n_beams), np = static_cast<size_t>(n_poses);
  std::vector<double> points(2 * nb * np), sensor_xy(2 * np);
  std::vector<uint64_t> counts(np * kFitCounters);
  host_parallel_for_wide(np, [&](size_t k) {
    kh_scan_points(ranges, laser->n_beams, sensor_poses + 3 * k, laser->minimum_angle, laser->angular_resolution, &points[2 * nb * k]);
    sensor_xy[2 * k] = sensor_poses[3 * k]; sensor_xy[2 * k + 1] = sensor_poses[3 * k + 1];
  });
  MapWork * w = map_work_create(view->device);
  if (!w) {return KH_ERR_HIP;}
  const int rc = map_fit_counts(w, *view, laser->n_beams, ranges, n_poses, points.data(), sensor_xy.data(), laser->range_threshold,
      laser->minimum_range, laser->maximum_range, counts.data(), nullptr);
  map_work_destroy(w);
  if (rc) {return rc;}
  for (size_t k = 0; k < np; ++k) {out[k] = fit_derive(&counts[k * kFitCounters]);}
  return KH_OK;
}

int kh_map_raycast(const kh_map_view * view, const kh_laser * laser, int32_t n_poses, const double * sensor_poses, int32_t max_unknown,
  double no_return, kh_ray_t * out, double * kernel_ms)
{
  if (kernel_ms) {*kernel_ms = 0.0;}
  if (!out || map_raycast_check(view, laser, n_poses, sensor_poses, max_unknown) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (require_device(view->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  MapWork * w = map_work_create(view->device);
  if (!w) {return KH_ERR_HIP;}
  const int rc = map_raycast(w, *view, *laser, n_poses, sensor_poses, max_unknown, no_return, out, kernel_ms);
  map_work_destroy(w);
  return rc;
}

int kh_occupancy_write_nav(kh_occupancy * g, const int8_t * nav)
{
  if (!g || !nav) {return KH_ERR_INVALID_ARG;}
  const int64_t total = static_cast<int64_t>(g->dev.width) * g->dev.height;
  for (int64_t i = 0; i < total; ++i) {
    if (nav[i] != -1 && nav[i] != 0 && nav[i] != 100) {
      set_error("kh_occupancy_write_nav: value " + std::to_string(nav[i]) + " at " + std::to_string(i) + " is none of -1, 0, 100");
      return KH_ERR_INVALID_ARG;
    }
  }
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  // (the dense values go through kh_occupancy_read_nav's buffer)
  const size_t bytes = (static_cast<size_t>(total) + 3) & ~static_cast<size_t>(3);
  if (!grow_device(g->stream, reinterpret_cast<void **>(&g->d_nav), &g->cap_nav, bytes, bytes)) {
    set_error("kh_occupancy_write_nav: input allocation failed");
    return KH_ERR_HIP;
  }
  const size_t size = static_cast<size_t>(g->dev.ws) * g->dev.height;
  const int64_t words = static_cast<int64_t>(size / 4);
  if (hipMemcpyAsync(g->d_nav, nav, static_cast<size_t>(total), hipMemcpyHostToDevice, g->stream) != hipSuccess) {
    (void)hipStreamSynchronize(g->stream);
    return KH_ERR_HIP;
  }
  hipLaunchKernelGGL(k_nav_to_occ, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, g->stream,
    reinterpret_cast<const int8_t *>(g->d_nav), g->dev.width, g->dev.ws, words, reinterpret_cast<uint32_t *>(g->dev.cells));
  // (the stream is drained before returning: `nav` is the caller's pageable memory)
  if (hipMemsetAsync(g->dev.pass, 0, size * 4, g->stream) != hipSuccess || hipMemsetAsync(g->dev.hits, 0, size * 4, g->stream) != hipSuccess ||
    hipStreamSynchronize(g->stream) != hipSuccess)
  {
    set_error(std::string("kh_occupancy_write_nav: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  return KH_OK;
}

}  // extern "C"
