// The distance field of a map (kh_map_field_*): the two passes of the exact Euclidean distance transform
// (k_field_columns, k_field_rows) and the field's three readers (k_field_costs and its rectangle form, k_field_lookup, k_field_score),
// with their launchers.  The kernels of an update (section 7p): occupancy_field_update.hip.
// Every kernel works on the field's OWN arrays (FieldWindow: the copied cells, the column distances, the values, all of one row stride
// that is a multiple of 4), so every dword and every 16-byte access is aligned whatever view the field was made from.  Everything a
// kernel produces is an integer: no result depends on the order of an atomic, none is decided by one.  The handle: map_field.cpp;
// the rules that need no device: map_field_plan.hpp; the gate, the rounding and the work layout of the score: occupancy_walk.hpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "../../include/karto_hip.h"
#include "lds_attr.hpp"
#include "map_field_plan.hpp"
#include "occupancy_walk.hpp"

namespace kh
{
// Pass 1: g = the distance along the column to the nearest obstacle of the column.  One thread per dword of a row -- four
// horizontally adjacent columns -- so the lanes of a wave sit on adjacent columns and every step of the sweep reads one coalesced
// piece of a row (a dword per lane) and writes one (four uint16 per lane).  The thread sweeps its four columns down, keeping four
// running distances in registers, then up, where it reads back what it wrote (g == 0 marks the obstacles: the cells are read once).
// A running distance above `limit` -- R, or for the uncapped field a number no column reaches -- is kFieldNoColumn and stays so
// until the next obstacle.  The columns beyond `width` of the last dword are never obstacles; what is written for them is never
// read.  The kernel has few threads and a long dependent walk, so a sweep takes kFieldBatch rows at a time: their loads are issued
// together, before the first store -- the addresses do not depend on the data -- and one memory latency is paid per batch, not per
// row.  (Whether a row exists is the same question in every lane.)
constexpr int32_t kFieldBatch = 8;
__global__ __launch_bounds__(64) void k_field_columns(FieldWindow f)
{
  const int32_t col = 4 * (int32_t)(blockIdx.x * 64 + threadIdx.x);
  if (col >= f.width) {return;}
  const uint32_t none = kFieldNoColumn, limit = f.radius > 0 ? (uint32_t)f.radius : 0xFFFEu;
  const bool not_free = f.obstacles == KH_FIELD_OBSTACLE_NOT_FREE;
  const uint32_t * const cells = reinterpret_cast<const uint32_t *>(f.cells);
  uint2 * const g = reinterpret_cast<uint2 *>(f.g);
  const int64_t step = f.ws >> 2, first = col >> 2;
  uint32_t d[4] = {none, none, none, none};
  for (int32_t row0 = 0; row0 < f.height; row0 += kFieldBatch) {
    uint32_t c4[kFieldBatch];
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {c4[k] = row0 + k < f.height ? cells[first + (int64_t)(row0 + k) * step] : 0u;}
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {
      if (row0 + k < f.height) {
#pragma unroll
        for (int32_t e = 0; e < 4; ++e) {
          const uint32_t state = (c4[k] >> (8 * e)) & 0xFFu;
          const bool obstacle = col + e < f.width && (not_free ? state != 255u : state == 100u);
          d[e] = obstacle ? 0u : d[e] >= limit ? none : d[e] + 1u;
        }
        g[first + (int64_t)(row0 + k) * step] = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));
      }
    }
  }
  uint32_t u[4] = {none, none, none, none};
  for (int32_t row0 = f.height - 1; row0 >= 0; row0 -= kFieldBatch) {
    uint2 down[kFieldBatch];
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {down[k] = row0 - k >= 0 ? g[first + (int64_t)(row0 - k) * step] : make_uint2(0u, 0u);}
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {
      if (row0 - k >= 0) {
        const uint32_t have[4] = {down[k].x & 0xFFFFu, down[k].x >> 16, down[k].y & 0xFFFFu, down[k].y >> 16};
        uint32_t both[4];
#pragma unroll
        for (int32_t e = 0; e < 4; ++e) {
          u[e] = have[e] == 0u ? 0u : u[e] >= limit ? none : u[e] + 1u;
          both[e] = u[e] < have[e] ? u[e] : have[e];
        }
        g[first + (int64_t)(row0 - k) * step] = make_uint2(both[0] | (both[1] << 16), both[2] | (both[3] << 16));
      }
    }
  }
}

// Pass 2: one workgroup per row.  The row of g is staged into LDS (at most 32768 x 2 B), then the thread of cell i scans outward,
// k = i, i -+ 1, i -+ 2, ..., keeping best = min(g[k]^2 + (i - k)^2), and leaves as soon as (i - k)^2 >= best (no farther column can
// win), when |i - k| > R for R > 0, or when both sides have run off the row: exact, and short wherever a wall is near.  Adjacent lanes
// read adjacent uint16s of LDS.  The thread writes d2, or KH_FIELD_FAR for "none" and for a value above R^2, and counts; the three
// statistics go lanes -> wave by shuffles, the four waves through LDS, one atomic per non-zero counter and workgroup.
__global__ __launch_bounds__(256) void k_field_rows(FieldWindow f, unsigned long long * __restrict__ counts)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char field_lds[];
  uint16_t * const g = reinterpret_cast<uint16_t *>(field_lds);
  uint32_t * const part = reinterpret_cast<uint32_t *>(field_lds + (((size_t)f.ws * 2 + 15) & ~(size_t)15));      // [4][kFieldCounters]
  const int32_t row = (int32_t)blockIdx.x;
  const uint2 * const src = reinterpret_cast<const uint2 *>(f.g + (int64_t)row * f.ws);
  for (int32_t q = (int32_t)threadIdx.x; q < (f.ws >> 2); q += 256) {reinterpret_cast<uint2 *>(g)[q] = src[q];}
  __syncthreads();
  const uint32_t inf = 0xFFFFFFFFu, radius = (uint32_t)f.radius, r2 = radius * radius;
  uint32_t n_obstacles = 0u, n_far = 0u, max_d2 = 0u;
  for (int32_t i = (int32_t)threadIdx.x; i < f.width; i += 256) {
    const uint32_t here = g[i];
    uint32_t best = here == kFieldNoColumn ? inf : here * here;
    for (uint32_t d = 1u; ; ++d) {
      const uint32_t dd = d * d;
      if (dd >= best || (radius > 0u && d > radius)) {break;}
      const int32_t left = i - (int32_t)d, right = i + (int32_t)d;
      if (left < 0 && right >= f.width) {break;}
      if (left >= 0) {
        const uint32_t gl = g[left], v = gl * gl + dd;
        best = (gl != kFieldNoColumn && v < best) ? v : best;
      }
      if (right < f.width) {
        const uint32_t gr = g[right], v = gr * gr + dd;
        best = (gr != kFieldNoColumn && v < best) ? v : best;
      }
    }
    if (best == inf || (radius > 0u && best > r2)) {
      best = KH_FIELD_FAR;
      ++n_far;
    } else {
      n_obstacles += best == 0u;
      max_d2 = best > max_d2 ? best : max_d2;
    }
    f.d2[(int64_t)row * f.ws + i] = best;
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    n_obstacles += __shfl_xor(n_obstacles, d);
    n_far += __shfl_xor(n_far, d);
    const uint32_t other = __shfl_xor(max_d2, d);
    max_d2 = other > max_d2 ? other : max_d2;
  }
  if ((threadIdx.x & 63) == 0) {
    uint32_t * const mine = part + (threadIdx.x >> 6) * kFieldCounters;
    mine[kFieldObstacles] = n_obstacles; mine[kFieldFar] = n_far; mine[kFieldMaxD2] = max_d2;
  }
  __syncthreads();
  if (threadIdx.x < kFieldCounters) {
    const uint32_t a = part[threadIdx.x], b = part[kFieldCounters + threadIdx.x], c = part[2 * kFieldCounters + threadIdx.x],
      e = part[3 * kFieldCounters + threadIdx.x];
    if (threadIdx.x == kFieldMaxD2) {
      const uint32_t ab = a > b ? a : b, ce = c > e ? c : e, v = ab > ce ? ab : ce;
      if (v) {atomicMax(&counts[kFieldMaxD2], (unsigned long long)v);}
    } else {
      const unsigned long long v = (unsigned long long)a + b + c + e;
      if (v) {atomicAdd(&counts[threadIdx.x], v);}
    }
  }
}

// Costmap values: one thread per four cells -- a dword of states, 16 bytes of values, a dword of costs.  c = table[d2] where d2 <=
// rt2, else 0 (KH_FIELD_FAR lies above every rt2); an unknown cell (neither 100 nor 255) under track_unknown is 255 unless c >= 253
// or, with inflate_unknown, c > 0.  The cells of the row padding get 0.
__device__ __forceinline__ uint32_t field_cost(uint32_t state, uint32_t v, const uint8_t * __restrict__ table, uint32_t rt2, int32_t track_unknown,
  int32_t inflate_unknown)
{
  const uint32_t c = v <= rt2 ? table[v] : 0u;
  const bool unknown = state != 100u && state != 255u;
  return unknown && track_unknown && !(c >= 253u || (inflate_unknown && c > 0u)) ? 255u : c;
}

__global__ __launch_bounds__(256) void k_field_costs(FieldWindow f, const uint8_t * __restrict__ table, uint32_t rt2, int32_t track_unknown,
  int32_t inflate_unknown, uint32_t * __restrict__ out)
{
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t quads = f.ws >> 2;
  if (q >= (int64_t)quads * f.height) {return;}
  const int32_t col = 4 * (int32_t)(q % quads);
  const uint32_t c4 = reinterpret_cast<const uint32_t *>(f.cells)[q];
  const uint4 v4 = reinterpret_cast<const uint4 *>(f.d2)[q];
  const uint32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
  uint32_t cost4 = 0u;
#pragma unroll
  for (int32_t e = 0; e < 4; ++e) {
    if (col + e < f.width) {
      cost4 |= field_cost((c4 >> (8 * e)) & 0xFFu, v[e], table, rt2, track_unknown, inflate_unknown) << (8 * e);
    }
  }
  out[q] = cost4;
}

// The same costs for window columns [r.x0, r.x1) and rows [r.y0, r.y1) as a dense block of row stride out_ws (a multiple of 4): one
// thread per dword of the block.  The rectangle begins at any column, so its states and values are read cell by cell; the four costs
// leave as one dword.  The cells of the block's row padding get 0.
__global__ __launch_bounds__(256) void k_field_costs_rect(FieldWindow f, FieldRect r, const uint8_t * __restrict__ table, uint32_t rt2,
  int32_t track_unknown, int32_t inflate_unknown, uint32_t * __restrict__ out, int32_t out_ws)
{
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t quads = out_ws >> 2;
  if (q >= (int64_t)quads * (r.y1 - r.y0)) {return;}
  const int32_t col = r.x0 + 4 * (int32_t)(q % quads);
  const int64_t at = (int64_t)(r.y0 + (int32_t)(q / quads)) * f.ws + col;
  uint32_t cost4 = 0u;
#pragma unroll
  for (int32_t e = 0; e < 4; ++e) {
    if (col + e < r.x1) {cost4 |= field_cost(f.cells[at + e], f.d2[at + e], table, rt2, track_unknown, inflate_unknown) << (8 * e);}
  }
  out[q] = cost4;
}

// Clearance: one thread per point; its cell by occ_cell, the window's index and bounds guard (cell_at).  A coordinate beyond +-2^30
// cells (occ_cell's "beyond the int32 lattice" among them) and a cell outside the window are OUTSIDE.
__global__ __launch_bounds__(256) void k_field_lookup(FieldWindow f, int32_t n, const double * __restrict__ xy, uint32_t * __restrict__ d2,
  int32_t * __restrict__ status)
{
  const int32_t k = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (k >= n) {return;}
  const int32_t cx = occ_cell(xy[2 * (int64_t)k], f.ax, f.scale), cy = occ_cell(xy[2 * (int64_t)k + 1], f.ay, f.scale);
  const int32_t limit = 1 << 30;
  uint32_t v = KH_FIELD_FAR;
  int32_t code = KH_CLEAR_OUTSIDE;
  if (cx >= -limit && cx <= limit && cy >= -limit && cy <= limit) {
    const CellAt at = cell_at(f, cx, cy);
    if (at.inside) {
      v = f.d2[at.k];
      code = v == KH_FIELD_FAR ? KH_CLEAR_FAR : KH_CLEAR_OK;
    }
  }
  d2[k] = v;
  status[k] = code;
}

// The endpoint score of one scan at many poses: k_map_fit's tables and layout -- one wave per (pose, run of 64 beams), a workgroup
// holds waves of ONE pose -- but no line is walked: a beam that passes the gate with a valid end reads the value of its end cell.  A
// lane's four flags (kept, hit, inside, near) travel as four bytes of one word (a wave holds 64 beams) next to its value; the wave
// reduces both by shuffles and lanes 0 .. 4 add the five sums to the pose's row, one atomic per non-zero counter and wave.
__global__ __launch_bounds__(256) void k_field_score(
  FieldWindow f, const double * __restrict__ ranges, const double * __restrict__ points, const double * __restrict__ sensors, int32_t n_beams,
  int32_t blocks_per_pose, double range_threshold, double min_range, double max_range, uint32_t t2, unsigned long long * __restrict__ out)
{
  const PoseWave w = pose_wave(blocks_per_pose);
  const int32_t pose = w.pose;
  const int64_t i = w.beam();
  uint32_t flags = 0u, sum = 0u;
  if (i < n_beams) {
    const double sx = sensors[2 * (int64_t)pose], sy = sensors[2 * (int64_t)pose + 1];
    const double * const p = points + 2 * ((int64_t)pose * n_beams + i);
    const Beam b = occ_gate(ranges[i], p[0], p[1], sx, sy, range_threshold, min_range, max_range);
    if (b.kept) {
      flags = 1u << (8 * kScoreKept);
      if (b.hit) {
        flags |= 1u << (8 * kScoreHit);
        const int32_t cx = occ_cell(b.px, f.ax, f.scale), cy = occ_cell(b.py, f.ay, f.scale);
        const CellAt at = cell_at(f, cx, cy);
        if (at.inside && cx != INT32_MIN && cy != INT32_MIN) {
          flags |= 1u << (8 * kScoreInside);
          const uint32_t v = f.d2[at.k];
          if (v <= t2) {flags |= 1u << (8 * kScoreNear); sum = v;}
        }
      }
    }
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    flags += __shfl_xor(flags, d);           // (at most 64 per byte)
    sum += __shfl_xor(sum, d);               // (at most 64 x 1024^2)
  }
  const int32_t lane = threadIdx.x & 63;
  if (lane < kScoreCounters) {
    const uint32_t v = lane == kScoreSum ? sum : (flags >> (8 * lane)) & 0xFFu;
    if (v) {atomicAdd(&out[(int64_t)pose * kScoreCounters + lane], (unsigned long long)v);}
  }
}

void field_columns(void * stream, const FieldWindow & f)
{
  hipLaunchKernelGGL(k_field_columns, dim3(static_cast<unsigned>(((f.ws >> 2) + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), f);
}

bool field_rows(void * stream, const FieldWindow & f, unsigned long long * d_counts)
{
  const size_t lds = ((static_cast<size_t>(f.ws) * 2 + 15) & ~static_cast<size_t>(15)) + 4 * kFieldCounters * sizeof(uint32_t);
  static std::atomic<unsigned long long> done{0};
  allow_dynamic_lds(reinterpret_cast<const void *>(k_field_rows), static_cast<int>(kMaxFieldSide * 2 + 4 * kFieldCounters * sizeof(uint32_t)), done);
  hipLaunchKernelGGL(k_field_rows, dim3(static_cast<unsigned>(f.height)), dim3(256), lds, static_cast<hipStream_t>(stream), f, d_counts);
  return hipPeekAtLastError() == hipSuccess;
}

void field_costs(void * stream, const FieldWindow & f, const uint8_t * d_table, uint32_t rt2, int32_t track_unknown, int32_t inflate_unknown,
  uint8_t * d_out)
{
  const int64_t quads = static_cast<int64_t>(f.ws >> 2) * f.height;
  hipLaunchKernelGGL(k_field_costs, dim3(static_cast<unsigned>((quads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), f, d_table, rt2,
    track_unknown, inflate_unknown, reinterpret_cast<uint32_t *>(d_out));
}

void field_costs_rect(void * stream, const FieldWindow & f, const FieldRect & r, const uint8_t * d_table, uint32_t rt2, int32_t track_unknown,
  int32_t inflate_unknown, uint8_t * d_out, int32_t out_ws)
{
  const int64_t quads = static_cast<int64_t>(out_ws >> 2) * (r.y1 - r.y0);
  hipLaunchKernelGGL(k_field_costs_rect, dim3(static_cast<unsigned>((quads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), f, r, d_table,
    rt2, track_unknown, inflate_unknown, reinterpret_cast<uint32_t *>(d_out), out_ws);
}

void field_lookup(void * stream, const FieldWindow & f, int32_t n, const double * d_xy, uint32_t * d_d2, int32_t * d_status)
{
  hipLaunchKernelGGL(k_field_lookup, dim3(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), f, n,
    d_xy, d_d2, d_status);
}

void field_score(void * stream, const FieldWindow & f, const double * d_ranges, const double * d_points, const double * d_sensors, int32_t n_beams,
  int32_t n_poses, double range_threshold, double min_range, double max_range, uint32_t t2, unsigned long long * d_sums)
{
  const int32_t blocks = blocks_per_pose(n_beams, n_poses);
  hipLaunchKernelGGL(k_field_score, dim3(static_cast<unsigned>(blocks) * static_cast<unsigned>(n_poses)), dim3(256), 0, static_cast<hipStream_t>(stream), f,
    d_ranges, d_points, d_sensors, n_beams, blocks, range_threshold, min_range, max_range, t2, d_sums);
}
}  // namespace kh
