// A map view as a localizer reads it (kh_map_seeds, kh_map_fit, kh_map_raycast; DESIGN.md sections 7k and 7m): the kernels that only
// READ a kh_map_view -- where a robot can stand, how a scan at many poses fits, what a scan from a pose would be -- their launchers on
// a caller's work buffers, and the three entry points that make such buffers for one call.  What the kernels share with the trace
// kernels: occupancy_walk.hpp; the rules that need no device: map_localize_plan.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "occupancy_walk.hpp"

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
