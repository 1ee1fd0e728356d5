// A map view as a localizer reads it (kh_map_seeds, kh_map_fit, kh_map_raycast; DESIGN.md sections 7k and 7m): the kernels that only
// READ a kh_map_view -- where a robot can stand, how a scan at many poses fits, what a scan from a pose would be -- their launchers on
// a caller's work buffers, and the three entry points that make such buffers for one call; and the two kernels of a merge of two
// views (kh_map_merge_*, section 7n; the handle: map_merge.cpp), which read both and write a third.  What the kernels share with the
// trace kernels: occupancy_walk.hpp; the rules that need no device: map_localize_plan.hpp, map_merge_plan.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "occupancy_walk.hpp"
#include "map_merge_plan.hpp"      // the order of a merge's six counters

namespace kh
{
// The FIT of one scan at many sensor poses against a map view (kh_map_fit): k_occ_fit_merged's layout without the scan dimension --
// one wave per (pose, run of 64 beams), a workgroup holds waves of ONE pose (pose_wave) -- and its reduction (fit_reduce).  points: per
// pose the 2 * n_beams unfiltered point readings at that pose (kh_scan_points on the host: libm stays there); sensors: 2 per pose.
// The view is only read.  A lane past the beam count takes part in the reduction with zeros: every wave reaches the barrier.
__global__ __launch_bounds__(256) void k_map_fit(
  MapWindow g, const double * __restrict__ ranges, const double * __restrict__ points, const double * __restrict__ sensors, int32_t n_beams,
  int32_t blocks_per_pose, double range_threshold, double min_range, double max_range, unsigned long long * __restrict__ out)
{
  const PoseWave w = pose_wave(blocks_per_pose);
  const int32_t pose = w.pose;
  const int64_t i = w.beam();
  FitCounts n;
  if (i < n_beams) {
    const double sx = sensors[2 * (int64_t)pose], sy = sensors[2 * (int64_t)pose + 1];
    const double * const p = points + 2 * ((int64_t)pose * n_beams + i);
    const Beam b = occ_gate(ranges[i], p[0], p[1], sx, sy, range_threshold, min_range, max_range);
    if (b.kept) {
      const int32_t x0 = occ_cell(sx, g.ax, g.scale), y0 = occ_cell(sy, g.ay, g.scale);
      const int32_t x1 = occ_cell(b.px, g.ax, g.scale), y1 = occ_cell(b.py, g.ay, g.scale);
      if (walk_bounded(x0, y0, x1, y1)) {occ_walk(FitCells<MapWindow>{g, n}, x0, y0, x1, y1, b.hit);}
    }
  }
  fit_reduce(n, out, pose);
}

// The EXPECTED scan of a map view (kh_map_raycast): one lane per (pose, beam), k_map_fit's layout -- a wave holds
// 64 consecutive beams of one pose, so neighbouring lanes read neighbouring cells near the sensor.  points: per pose the far point of
// every beam (kh_scan_points of readings that are all range_threshold, on the host: libm stays there).  The lane visits the cells of
// TraceLine(sensor cell, far cell) outward from the sensor (RayWalk) and leaves at the first decision: an occupied cell (HIT), or
// the unknown cell that exceeds the budget (UNKNOWN; a cell outside the window and every state but 100 / 255 is unknown); the end of
// the line is FREE at the far cell.  The window's index and bounds guard (cell_at); k_map_fit's bound in front of the walk.  Once a
// lane stands outside the window on a side its line leads away from, no later cell exists: with no budget to run out (max_unknown
// < 0) the answer is FREE, and the lane says so at once.  No atomics, no LDS, one 16-byte store per lane.  A wave runs as long as its
// longest lane.
__global__ __launch_bounds__(256) void k_map_raycast(
  MapWindow g, const double * __restrict__ points, const double * __restrict__ sensors, int32_t n_beams, int32_t blocks_per_pose,
  int32_t max_unknown, RayCell * __restrict__ out)
{
  const PoseWave w = pose_wave(blocks_per_pose);
  const int32_t pose = w.pose;
  const int64_t i = w.beam();
  if (i >= n_beams) {return;}
  const double sx = sensors[2 * (int64_t)pose], sy = sensors[2 * (int64_t)pose + 1];
  const double * const p = points + 2 * ((int64_t)pose * n_beams + i);
  const int32_t x0 = occ_cell(sx, g.ax, g.scale), y0 = occ_cell(sy, g.ay, g.scale);
  const int32_t x1 = occ_cell(p[0], g.ax, g.scale), y1 = occ_cell(p[1], g.ay, g.scale);
  const int64_t ex = (int64_t)x1 - x0, ey = (int64_t)y1 - y0;
  RayCell r{x1, y1, 0, KH_RAY_FREE};
  if (walk_bounded(x0, y0, x1, y1)) {
    RayWalk walk(x0, y0, x1, y1);
    const int32_t length = walk.length();
    r.steps = length;
    int32_t unknown = 0;
    for (int32_t s = 0; s <= length; ++s, walk.next()) {
      const int32_t cx = walk.x(), cy = walk.y();
      const CellAt at = cell_at(g, cx, cy);
      uint32_t state = 0u;
      if (at.inside) {
        state = g.cells[at.k];
      } else if (max_unknown < 0 && ((at.wx < 0 && ex <= 0) || (at.wx >= g.width && ex >= 0) || (at.wy < 0 && ey <= 0) || (at.wy >= g.height && ey >= 0))) {
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

// The box of a map's known cells (kh_map_merge_create): one pass over the window, a workgroup per row in a
// grid stride, its threads along the row, so a wave reads consecutive bytes and nothing of the padding.  Each lane keeps min / max of
// the lattice i and j of its cells of state != 0; the wave reduces by shuffles, the four waves through LDS, then one atomicMin /
// atomicMax on int32 per workgroup and bound that found a cell.  Integer extrema do not depend on the order.
__global__ __launch_bounds__(256) void k_map_known_box(MapWindow g, int32_t * __restrict__ box)
{
  __shared__ int32_t part[4][4];
  int32_t lo_i = INT32_MAX, lo_j = INT32_MAX, hi_i = INT32_MIN, hi_j = INT32_MIN;
  for (int32_t y = blockIdx.x; y < g.height; y += gridDim.x) {
    const uint8_t * const row = g.cells + (int64_t)y * g.ws;
    for (int32_t x = threadIdx.x; x < g.width; x += 256) {
      if (row[x] != 0u) {
        const int32_t i = g.ox + x, j = g.oy + y;      // (inside the int32 lattice: map_view_check)
        lo_i = i < lo_i ? i : lo_i; hi_i = i > hi_i ? i : hi_i;
        lo_j = j < lo_j ? j : lo_j; hi_j = j > hi_j ? j : hi_j;
      }
    }
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    const int32_t a = __shfl_xor(lo_i, d), b = __shfl_xor(lo_j, d), c = __shfl_xor(hi_i, d), e = __shfl_xor(hi_j, d);
    lo_i = a < lo_i ? a : lo_i; lo_j = b < lo_j ? b : lo_j; hi_i = c > hi_i ? c : hi_i; hi_j = e > hi_j ? e : hi_j;
  }
  if ((threadIdx.x & 63) == 0) {
    int32_t * const mine = part[threadIdx.x >> 6];
    mine[0] = lo_i; mine[1] = lo_j; mine[2] = hi_i; mine[3] = hi_j;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int32_t k = threadIdx.x;
    const int32_t a = part[0][k], b = part[1][k], c = part[2][k], e = part[3][k];
    if (k < 2) {
      const int32_t ab = a < b ? a : b, ce = c < e ? c : e, v = ab < ce ? ab : ce;
      if (v != INT32_MAX) {atomicMin(&box[k], v);}
    } else {
      const int32_t ab = a > b ? a : b, ce = c > e ? c : e, v = ab > ce ? ab : ce;
      if (v != INT32_MIN) {atomicMax(&box[k], v);}
    }
  }
}

// the state of lattice cell (cx, cy) of a view as a merge reads it: 0 where the window has no such cell or the index is o_to_int's
// "beyond the int32 lattice"
__device__ __forceinline__ uint32_t merge_state(const MapWindow & g, int32_t cx, int32_t cy)
{
  const CellAt at = cell_at(g, cx, cy);
  return (at.inside && cx != INT32_MIN && cy != INT32_MIN) ? g.cells[at.k] : 0u;
}

// Two maps merged (kh_map_merge_create): one thread per dword of the output, four horizontally adjacent cells;
// a workgroup a tile of 64 x 16 cells (thread t: dword t % 16 of row t / 16), so the gathers of a rotated tile stay within a few
// dozen rows of the moving map.  Every cell is evaluated by the rule as written, from its own lattice index -- nothing is stepped
// along a row: the world point anchor + (double)I / scale, the footprint's sample points, each through the inverse correction and
// occ_cell onto the moving lattice, one byte read there; the target's state at the same index; code and merged state by the table.
// The thread writes one dword of cells and one of codes (the cells of the row padding 0).  The six counters travel as six 10-bit
// fields of one 64-bit word (a wave holds 256 cells): lanes -> wave by shuffles, the four waves through LDS, one 64-bit atomicAdd per
// non-zero counter and workgroup -- integer sums, no atomic decides a position or a value.  Neither input is written.
__global__ __launch_bounds__(256) void k_map_merge(MergeJob q, uint8_t * __restrict__ cells, uint8_t * __restrict__ codes,
  unsigned long long * __restrict__ counts)
{
  __shared__ unsigned long long part[4];
  const int32_t col = 4 * (int32_t)(blockIdx.x * (kMergeTileWidth / 4) + (threadIdx.x & 15));
  const int32_t row = (int32_t)(blockIdx.y * kMergeTileHeight + (threadIdx.x >> 4));
  unsigned long long n = 0ull;
  if (row < q.height && col < q.ws) {
    const int32_t lj = q.oy + row;
    const double wy = q.target.ay + (double)lj / q.target.scale;
    uint32_t cell4 = 0u, code4 = 0u;
#pragma unroll
    for (int32_t e = 0; e < 4; ++e) {
      if (col + e < q.width) {
        const int32_t li = q.ox + col + e;
        const double wx = q.target.ax + (double)li / q.target.scale;
        bool occupied = false, is_free = false;
        for (int32_t b = 0; b < q.footprint; ++b) {
          const double sy = wy + q.d[b];
          for (int32_t a = 0; a < q.footprint; ++a) {
            const double sx = wx + q.d[a];
            const double px = (q.c * sx - q.s * sy) + q.tx, py = (q.s * sx + q.c * sy) + q.ty;
            const uint32_t state = merge_state(q.moving, occ_cell(px, q.moving.ax, q.moving.scale), occ_cell(py, q.moving.ay, q.moving.scale));
            occupied = occupied || state == 100u;
            is_free = is_free || state == 255u;
          }
        }
        const uint32_t m = occupied ? 100u : is_free ? 255u : 0u;
        const uint32_t raw = merge_state(q.target, li, lj);
        const uint32_t t = (raw == 100u || raw == 255u) ? raw : 0u;
        uint32_t code = KH_MERGED_NEITHER, cell = 0u;
        int32_t counter = -1;
        if (t == 0u) {
          if (m != 0u) {code = KH_MERGED_MOVING_ONLY; cell = m; counter = kMergeMovingOnly;}
        } else if (m == 0u) {
          code = KH_MERGED_TARGET_ONLY; cell = t; counter = kMergeTargetOnly;
        } else if (t == m) {
          code = KH_MERGED_AGREE; cell = t; counter = t == 255u ? kMergeAgreeFree : kMergeAgreeOccupied;
        } else {
          code = m == 100u ? KH_MERGED_MOVING_OCCUPIED : KH_MERGED_MOVING_FREE;
          counter = m == 100u ? kMergeMovingOccupied : kMergeMovingFree;
          cell = q.conflict == KH_MERGE_CONFLICT_TARGET ? t : q.conflict == KH_MERGE_CONFLICT_MOVING ? m : q.conflict == KH_MERGE_CONFLICT_OCCUPIED ? 100u : 0u;
        }
        cell4 |= cell << (8 * e); code4 |= code << (8 * e);
        if (counter >= 0) {n += 1ull << (10 * counter);}
      }
    }
    const int64_t at = ((int64_t)row * q.ws + col) >> 2;
    reinterpret_cast<uint32_t *>(cells)[at] = cell4;
    reinterpret_cast<uint32_t *>(codes)[at] = code4;
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {n += __shfl_xor(n, d);}
  if ((threadIdx.x & 63) == 0) {part[threadIdx.x >> 6] = n;}
  __syncthreads();
  if (threadIdx.x < kMergeCounters) {
    const int32_t shift = 10 * (int32_t)threadIdx.x;
    const unsigned long long v = ((part[0] >> shift) & 0x3FFull) + ((part[1] >> shift) & 0x3FFull) + ((part[2] >> shift) & 0x3FFull) +
      ((part[3] >> shift) & 0x3FFull);
    if (v) {atomicAdd(&counts[threadIdx.x], v);}
  }
}

void map_known_box(void * stream, const kh_map_view & v, int32_t * d_box)
{
  hipLaunchKernelGGL(k_map_known_box, dim3(static_cast<unsigned>(std::min(v.height, 1024))), dim3(256), 0, static_cast<hipStream_t>(stream), window_of(v),
    d_box);
}

void map_merge_cells(void * stream, const MergeJob & job, uint8_t * d_cells, uint8_t * d_codes, unsigned long long * d_counts)
{
  const dim3 blocks(static_cast<unsigned>((job.ws + kMergeTileWidth - 1) / kMergeTileWidth), static_cast<unsigned>((job.height + kMergeTileHeight - 1) / kMergeTileHeight));
  hipLaunchKernelGGL(k_map_merge, blocks, dim3(256), 0, static_cast<hipStream_t>(stream), job, d_cells, d_codes, d_counts);
}

struct MapWork : DeviceWork {};

MapWork * map_work_create(int32_t device)
{
  MapWork * w = new MapWork();
  if (!work_open(*w, device)) {
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
  work_close(*w);
  delete w;
}

int map_view_check(const kh_map_view * v)
{
  static const char * const kWhy[] = {"", "malformed map view", "map view too large", "map view: the window leaves the int32 lattice"};
  const int32_t bad = map_view_refusal(v);
  if (bad != kViewOk) {set_error(kWhy[bad]); return KH_ERR_INVALID_ARG;}
  return KH_OK;
}

int map_seed_blocks(MapWork * w, const kh_map_view & v, int32_t pitch, int64_t bx0, int64_t by0, int64_t nbx, int64_t nby, int32_t * local,
  double * kernel_ms)
{
  if (kernel_ms) {*kernel_ms = 0.0;}
  const int64_t n_blocks = nbx * nby;
  if (!w || pitch < 1 || nbx < 1 || nby < 1 || !local || n_blocks > (1ll << 31) - 4096) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(w->device) != hipSuccess) {return KH_ERR_HIP;}
  Part parts[] = {{nullptr, static_cast<size_t>(n_blocks) * sizeof(int32_t)}};
  const int rc = work_stage(*w, "kh_map_seeds", "block table", false, parts);
  if (rc) {return rc;}
  return work_run(*w, "kh_map_seeds", [&] {
    hipLaunchKernelGGL(k_map_seeds, dim3(static_cast<unsigned>((n_blocks + 3) / 4)), dim3(256), 0, w->stream, window_of(v), pitch, bx0, by0, nbx,
      n_blocks, parts[0].as<int32_t>());
  }, &parts[0], local, kernel_ms);
}

int map_fit_counts(MapWork * w, const kh_map_view & v, int32_t n_beams, const double * ranges, int32_t n_poses, const double * points,
  const double * sensor_xy, double range_threshold, double min_range, double max_range, uint64_t * counts, double * kernel_ms)
{
  if (kernel_ms) {*kernel_ms = 0.0;}
  if (!w || n_beams < 0 || n_poses < 1 || !counts || (n_beams > 0 && (!ranges || !points)) || !sensor_xy) {return KH_ERR_INVALID_ARG;}
  std::fill(counts, counts + static_cast<size_t>(n_poses) * kFitCounters, uint64_t{0});
  if (n_beams == 0) {return KH_OK;}
  const int32_t blocks = blocks_per_pose(n_beams, n_poses);
  if (blocks == 0) {set_error("kh_map_fit: too many poses for one launch"); return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(w->device) != hipSuccess) {return KH_ERR_HIP;}
  // the sums first, then the tables: every part a multiple of 8 bytes
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the sums are downloaded as they lie");
  const size_t np = static_cast<size_t>(n_poses), nb = static_cast<size_t>(n_beams);
  Part parts[] = {{kZeros, np * kFitCounters * sizeof(unsigned long long)}, {sensor_xy, np * 2 * sizeof(double)}, {ranges, nb * sizeof(double)},
    {points, np * nb * 2 * sizeof(double)}};
  const int rc = work_stage(*w, "kh_map_fit", "table", true, parts);
  if (rc) {return rc;}
  return work_run(*w, "kh_map_fit", [&] {
    hipLaunchKernelGGL(k_map_fit, dim3(static_cast<unsigned>(blocks) * static_cast<unsigned>(n_poses)), dim3(256), 0, w->stream, window_of(v),
      parts[2].as<const double>(), parts[3].as<const double>(), parts[1].as<const double>(), n_beams, blocks, range_threshold, min_range, max_range,
      parts[0].as<unsigned long long>());
  }, &parts[0], counts, kernel_ms);
}

int map_raycast_cells(MapWork * w, const kh_map_view & v, int32_t n_beams, int32_t n_poses, const double * points, const double * sensor_xy,
  int32_t max_unknown, RayCell * out, double * kernel_ms)
{
  if (kernel_ms) {*kernel_ms = 0.0;}
  if (!w || n_beams < 1 || n_poses < 1 || !points || !sensor_xy || !out || max_unknown < -1) {return KH_ERR_INVALID_ARG;}
  const int32_t blocks = blocks_per_pose(n_beams, n_poses);
  if (blocks == 0) {set_error("kh_map_raycast: too many poses for one launch"); return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(w->device) != hipSuccess) {return KH_ERR_HIP;}
  // the answers first, then the tables: every part a multiple of 16 bytes
  const size_t np = static_cast<size_t>(n_poses), nb = static_cast<size_t>(n_beams);
  Part parts[] = {{nullptr, np * nb * sizeof(RayCell)}, {sensor_xy, np * 2 * sizeof(double)}, {points, np * nb * 2 * sizeof(double)}};
  const int rc = work_stage(*w, "kh_map_raycast", "table", true, parts);
  if (rc) {return rc;}
  return work_run(*w, "kh_map_raycast", [&] {
    hipLaunchKernelGGL(k_map_raycast, dim3(static_cast<unsigned>(blocks) * static_cast<unsigned>(n_poses)), dim3(256), 0, w->stream, window_of(v),
      parts[2].as<const double>(), parts[1].as<const double>(), n_beams, blocks, max_unknown, parts[0].as<RayCell>());
  }, &parts[0], out, kernel_ms);
}

// the laser and pose check of a call that takes a view, refused under `who`
static int view_inputs_check(const char * who, const kh_map_view & view, const kh_laser & laser, int32_t n_poses, const double * sensor_poses)
{
  const FitInputs f = fit_inputs_check(laser.range_threshold, laser.minimum_range, laser.maximum_range, laser.minimum_angle, laser.angular_resolution,
      static_cast<size_t>(n_poses), sensor_poses, view.anchor[0], view.anchor[1], view.scale);
  if (f.failed) {set_error(fit_inputs_text(f, who, kViewLaserWords, kViewPoseWords)); return KH_ERR_INVALID_ARG;}
  return KH_OK;
}

int map_raycast_check(const kh_map_view * view, const kh_laser * laser, int32_t n_poses, const double * sensor_poses, int32_t max_unknown)
{
  if (!laser || !sensor_poses || n_poses < 1 || max_unknown < -1 || laser->n_beams < 1 || map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  return view_inputs_check("kh_map_raycast", *view, *laser, n_poses, sensor_poses);
}

int map_raycast(MapWork * w, const kh_map_view & v, const kh_laser & laser, int32_t n_poses, const double * sensor_poses, int32_t max_unknown,
  double no_return, kh_ray_t * out, double * kernel_ms)
{
  const size_t nb = static_cast<size_t>(laser.n_beams), np = static_cast<size_t>(n_poses);
  const std::vector<double> far(nb, laser.range_threshold);
  std::vector<double> points(2 * nb * np), sensor_xy(2 * np);
  scan_points_at(far.data(), 0, laser.n_beams, laser.minimum_angle, laser.angular_resolution, np, sensor_poses, points.data(), sensor_xy.data());
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
}  // namespace kh

using namespace kh;

extern "C" {

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
  if (view_inputs_check("kh_map_fit", *view, *laser, n_poses, sensor_poses) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (require_device(view->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  const size_t nb = static_cast<size_t>(laser->n_beams), np = static_cast<size_t>(n_poses);
  std::vector<double> points(2 * nb * np), sensor_xy(2 * np);
  std::vector<uint64_t> counts(np * kFitCounters);
  scan_points_at(ranges, 0, laser->n_beams, laser->minimum_angle, laser->angular_resolution, np, sensor_poses, points.data(), sensor_xy.data());
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

}  // extern "C"
