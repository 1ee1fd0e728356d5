// The kernels of a change layer on a map view (kh_map_changes_*) and their launchers: scans observed into the
// layer's two counter grids and labelled against the map, the decay of the layer, the layer set against its map, and the changed
// cells as a list.  The handle and its buffers: map_changes.cpp; what the kernels share with the trace kernels: occupancy_walk.hpp.
#include <algorithm>

#include "occupancy_walk.hpp"

namespace kh
{
struct ObserveCells              // CountCells with delta 1 on the layer and, in the same visit, FitCells' read of the map's state
{
  const MapWindow & g;
  const ChangeLayer & layer;
  int64_t ex, ey, tolerance;     // the beam's end cell: a visit further than `tolerance` from it (Chebyshev) on an occupied map cell blocks
  uint32_t & blocked;
  __device__ __forceinline__ void add(int32_t cx, int32_t cy, bool hit) const
  {
    const CellAt at = cell_at(g, cx, cy);
    if (at.inside) {
      const int64_t k = at.k;
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
// "pose" read as "scan" -- one wave per (scan, run of 64 beams), a workgroup holds waves of ONE scan (pose_wave) -- and every scan with
// ranges of its own.  ONE walk under ONE visitor: it adds to the layer what k_occ_trace_delta's ADD adds, and counts in a lane register the
// occupied map cells the line crosses before it comes within `tolerance` cells of its end (the end cell is known before the walk, and
// the Chebyshev distance from it does not depend on the direction occ_walk takes).  Then at most (2 tolerance + 1)^2 cells around the
// end cell say whether the map holds an obstacle there, and the lane writes its two label words.  The map is only read, by plain
// loads; the layer only by atomics.  The walk bound in front of the walk is k_map_fit's; a beam it stops is labelled as dropped.
__global__ __launch_bounds__(256) void k_map_observe(
  MapWindow g, ChangeLayer layer, const double * __restrict__ ranges, const double * __restrict__ points, const double * __restrict__ sensors,
  int32_t n_beams, int32_t blocks_per_scan, double range_threshold, double min_range, double max_range, int32_t tolerance,
  int2 * __restrict__ labels)
{
  const PoseWave w = pose_wave(blocks_per_scan);
  const int32_t scan = w.pose;
  const int64_t i = w.beam();
  if (i >= n_beams) {return;}
  const int64_t beam = (int64_t)scan * n_beams + i;
  const double sx = sensors[2 * (int64_t)scan], sy = sensors[2 * (int64_t)scan + 1];
  const Beam b = occ_gate(ranges[beam], points[2 * beam], points[2 * beam + 1], sx, sy, range_threshold, min_range, max_range);
  int32_t label = KH_BEAM_DROPPED;
  uint32_t blocked = 0;
  if (b.kept) {
    const int32_t x0 = occ_cell(sx, g.ax, g.scale), y0 = occ_cell(sy, g.ay, g.scale);
    const int32_t x1 = occ_cell(b.px, g.ax, g.scale), y1 = occ_cell(b.py, g.ay, g.scale);
    if (walk_bounded(x0, y0, x1, y1)) {
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
// UpdateCell's rule (occ_state) on the layer's counters; the code says what it makes of the map's state, the patched state is the observed
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
    const uint32_t seen = occ_state(p, layer.hits[k], min_pass, threshold);
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

void map_observe(void * stream, const kh_map_view & v, const ChangeLayer & layer, const double * d_ranges, const double * d_points,
  const double * d_sensors, int32_t n_scans, int32_t n_beams, double range_threshold, double min_range, double max_range, int32_t tolerance,
  int32_t * d_labels)
{
  if (n_scans <= 0 || n_beams <= 0) {return;}
  const int32_t blocks = blocks_per_pose(n_beams, n_scans);
  hipLaunchKernelGGL(k_map_observe, dim3(static_cast<unsigned>(blocks) * static_cast<unsigned>(n_scans)), dim3(256), 0, static_cast<hipStream_t>(stream),
    window_of(v), layer, d_ranges, d_points, d_sensors, n_beams, blocks, range_threshold, min_range, max_range, tolerance,
    reinterpret_cast<int2 *>(d_labels));
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

void unit_scan(void * stream, int32_t * d_unit, int64_t n_units)
{
  hipLaunchKernelGGL(k_map_changed_scan, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), d_unit, n_units);
}

void map_changed_cells(void * stream, const kh_map_view & v, const uint8_t * d_codes, int32_t * d_unit, int32_t * d_list, int32_t cap)
{
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int32_t units_per_row = (v.width + 63) / 64;
  const int64_t n_units = change_units(v.width, v.height);
  const dim3 blocks(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n_units + 3) / 4, 1024))));
  hipLaunchKernelGGL(k_map_changed<false>, blocks, dim3(256), 0, s, window_of(v), d_codes, units_per_row, n_units, d_unit, d_list, cap);
  unit_scan(s, d_unit, n_units);
  if (cap > 0) {hipLaunchKernelGGL(k_map_changed<true>, blocks, dim3(256), 0, s, window_of(v), d_codes, units_per_row, n_units, d_unit, d_list, cap);}
}

}  // namespace kh
