// The kernels of a field that follows its map (kh_map_field_update), with their launchers: what changed
// (k_field_changed), the column pass over a rectangle cut into bands of rows (k_field_columns_band), the row pass over a rectangle
// (k_field_rows_region) and the recount of the statistics (k_field_count).  They work on the arrays of occupancy_field.hip's
// FieldWindow and write exactly what k_field_columns and k_field_rows write there.  Everything a kernel produces is an integer; the
// atomics are minima, maxima and sums of integers, so no result depends on their order.  The rules that need no device -- which
// rectangle, which bands -- are map_field_update_plan.hpp's; the handle is map_field.cpp's.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "../../include/karto_hip.h"
#include "lds_attr.hpp"
#include "map_field_plan.hpp"
#include "occupancy_device.hpp"

namespace kh
{
namespace
{
__device__ __forceinline__ bool is_obstacle(uint32_t state, bool not_free) {return not_free ? state != 255u : state == 100u;}
}  // namespace

// What changed: one thread per dword of the field's copy (its rows are dword-aligned whatever the view's are) that holds a cell of the
// rectangle.  The view's four cells come as one dword where the dword lies inside the rectangle and the view's address is aligned,
// else byte by byte -- a cell outside the rectangle, the view's row padding among them, is never read and keeps the copy's value.
// The copy takes the new cells in the same pass.  A thread keeps two boxes, of the cells whose state differs and of those whose
// obstacle-ness differs, as (min x, min y, -max x, -max y): eight minima that go lanes -> wave by shuffles, the four waves through
// LDS, then one atomicMin / atomicMax per bound a workgroup has; the cells compared are summed the same way.
__global__ __launch_bounds__(256) void k_field_changed(FieldWindow f, uint8_t * __restrict__ snapshot, const uint8_t * __restrict__ view, int32_t view_ws,
  FieldRect r, int32_t * __restrict__ result)
{
  __shared__ int32_t part[4][kChangedCount + 1];
  const int32_t q0 = r.x0 >> 2, quads = ((r.x1 + 3) >> 2) - q0;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool not_free = f.obstacles == KH_FIELD_OBSTACLE_NOT_FREE;
  int32_t low[kChangedCount];
#pragma unroll
  for (int32_t k = 0; k < kChangedCount; ++k) {low[k] = INT32_MAX;}
  int32_t compared = 0;
  if (t < (int64_t)quads * (r.y1 - r.y0)) {
    const int32_t row = r.y0 + (int32_t)(t / quads), col = 4 * (q0 + (int32_t)(t % quads));
    uint32_t * const mine = reinterpret_cast<uint32_t *>(snapshot + (int64_t)row * f.ws + col);
    const uint8_t * const src = view + (int64_t)row * view_ws + col;
    const uint32_t old4 = *mine;
    uint32_t new4 = old4;
    if (col >= r.x0 && col + 4 <= r.x1 && (reinterpret_cast<uintptr_t>(src) & 3u) == 0u) {
      new4 = *reinterpret_cast<const uint32_t *>(src);
      compared = 4;
    } else {
#pragma unroll
      for (int32_t e = 0; e < 4; ++e) {
        if (col + e >= r.x0 && col + e < r.x1) {
          new4 = (new4 & ~(0xFFu << (8 * e))) | ((uint32_t)src[e] << (8 * e));
          ++compared;
        }
      }
    }
    if (new4 != old4) {
      *mine = new4;
#pragma unroll
      for (int32_t e = 0; e < 4; ++e) {
        const uint32_t before = (old4 >> (8 * e)) & 0xFFu, now = (new4 >> (8 * e)) & 0xFFu;
        if (before != now) {
          const int32_t x = col + e;
          low[kChangedStates] = min(low[kChangedStates], x); low[kChangedStates + 1] = row;
          low[kChangedStates + 2] = min(low[kChangedStates + 2], -x); low[kChangedStates + 3] = -row;
          if (is_obstacle(before, not_free) != is_obstacle(now, not_free)) {
            low[kChangedObstacles] = min(low[kChangedObstacles], x); low[kChangedObstacles + 1] = row;
            low[kChangedObstacles + 2] = min(low[kChangedObstacles + 2], -x); low[kChangedObstacles + 3] = -row;
          }
        }
      }
    }
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int32_t k = 0; k < kChangedCount; ++k) {low[k] = min(low[k], __shfl_xor(low[k], d));}
    compared += __shfl_xor(compared, d);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int32_t k = 0; k < kChangedCount; ++k) {part[threadIdx.x >> 6][k] = low[k];}
    part[threadIdx.x >> 6][kChangedCount] = compared;
  }
  __syncthreads();
  if (threadIdx.x < kChangedCount) {
    const int32_t k = (int32_t)threadIdx.x;
    const int32_t v = min(min(part[0][k], part[1][k]), min(part[2][k], part[3][k]));
    if (v != INT32_MAX) {
      if (k & 2) {atomicMax(&result[k], -v);} else {atomicMin(&result[k], v);}
    }
  } else if (threadIdx.x == kChangedCount) {
    const int32_t n = part[0][kChangedCount] + part[1][kChangedCount] + part[2][kChangedCount] + part[3][kChangedCount];   // (at most 1024)
    if (n) {atomicAdd(reinterpret_cast<unsigned long long *>(result + kChangedCount), (unsigned long long)n);}
  }
}

// The column pass over a rectangle, capped fields only.  k_field_columns' thread -- four adjacent columns, lanes on adjacent dwords of
// a row -- but blockIdx.y names a band of `band` rows, [b0, b1).  A running distance above R is "none", so what lies more than R rows
// away cannot reach into the band: the down-sweep begins R rows above b0 (or at the window's first row) with "none" and has, by b0,
// the running distances of a sweep from row 0; the up-sweep begins R rows below b1 - 1, over the cell states -- those rows' g is
// another band's to write -- and goes on through the band over the g the down-sweep left (0 marks the obstacles).  Only rows of the
// band are written: every entry of g has one writer, in one launch, whatever the band height.  A dword whose columns are only
// partly inside [x0, x1) is computed whole; its other columns get the value they had.  Rows go kFieldBatch at a time, loads before
// the first dependent step, as in k_field_columns.
constexpr int32_t kFieldBatch = 8;

// rows first, first + step, ... (n of them) of the cell states through the running distances d; row k is written to g when k >= store_from
template <int32_t kStep>
__device__ __forceinline__ void sweep_states(const FieldWindow & f, int32_t col, int32_t first, int32_t n, int32_t store_from, uint32_t d[4])
{
  const uint32_t none = kFieldNoColumn, limit = (uint32_t)f.radius;
  const bool not_free = f.obstacles == KH_FIELD_OBSTACLE_NOT_FREE;
  const uint32_t * const cells = reinterpret_cast<const uint32_t *>(f.cells);
  uint2 * const g = reinterpret_cast<uint2 *>(f.g);
  const int64_t step = f.ws >> 2, quad = col >> 2;
  for (int32_t k0 = 0; k0 < n; k0 += kFieldBatch) {
    uint32_t c4[kFieldBatch];
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {c4[k] = k0 + k < n ? cells[quad + (int64_t)(first + kStep * (k0 + k)) * step] : 0u;}
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {
      if (k0 + k < n) {
#pragma unroll
        for (int32_t e = 0; e < 4; ++e) {
          const bool obstacle = col + e < f.width && is_obstacle((c4[k] >> (8 * e)) & 0xFFu, not_free);
          d[e] = obstacle ? 0u : d[e] >= limit ? none : d[e] + 1u;
        }
        if (k0 + k >= store_from) {g[quad + (int64_t)(first + kStep * (k0 + k)) * step] = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));}
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_field_columns_band(FieldWindow f, FieldRect r, int32_t band)
{
  const int32_t quad = (r.x0 >> 2) + (int32_t)(blockIdx.x * 64 + threadIdx.x);
  if (quad >= (r.x1 + 3) >> 2) {return;}
  const int32_t col = 4 * quad;
  const int32_t b0 = r.y0 + (int32_t)blockIdx.y * band, b1 = min(b0 + band, r.y1);
  const uint32_t none = kFieldNoColumn, limit = (uint32_t)f.radius;
  const int32_t above = max(0, b0 - f.radius), below = min(f.height, b1 + f.radius);
  uint32_t d[4] = {none, none, none, none};
  sweep_states<1>(f, col, above, b1 - above, b0 - above, d);
  uint32_t u[4] = {none, none, none, none};
  sweep_states<-1>(f, col, below - 1, below - b1, below - b1, u);
  uint2 * const g = reinterpret_cast<uint2 *>(f.g);
  const int64_t step = f.ws >> 2;
  for (int32_t row0 = b1 - 1; row0 >= b0; row0 -= kFieldBatch) {
    uint2 down[kFieldBatch];
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {down[k] = row0 - k >= b0 ? g[quad + (int64_t)(row0 - k) * step] : make_uint2(0u, 0u);}
#pragma unroll
    for (int32_t k = 0; k < kFieldBatch; ++k) {
      if (row0 - k >= b0) {
        const uint32_t have[4] = {down[k].x & 0xFFFFu, down[k].x >> 16, down[k].y & 0xFFFFu, down[k].y >> 16};
        uint32_t both[4];
#pragma unroll
        for (int32_t e = 0; e < 4; ++e) {
          u[e] = have[e] == 0u ? 0u : u[e] >= limit ? none : u[e] + 1u;
          both[e] = u[e] < have[e] ? u[e] : have[e];
        }
        g[quad + (int64_t)(row0 - k) * step] = make_uint2(both[0] | (both[1] << 16), both[2] | (both[3] << 16));
      }
    }
  }
}

// The row pass over a rectangle, capped fields only: one workgroup per row of the rectangle.  It stages the row's g over columns
// [s0, s1) -- the rectangle's columns grown by R, clipped to the window and rounded out to whole groups of four -- and the thread of
// cell i runs k_field_rows' outward scan with its early exit; no step of it reaches beyond R columns, so none leaves what is staged.
// No counters: the statistics of an updated field are k_field_count's.
__global__ __launch_bounds__(256) void k_field_rows_region(FieldWindow f, FieldRect r, int32_t s0, int32_t s1)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char region_lds[];
  uint16_t * const g = reinterpret_cast<uint16_t *>(region_lds);
  const int32_t row = r.y0 + (int32_t)blockIdx.x;
  const uint2 * const src = reinterpret_cast<const uint2 *>(f.g + (int64_t)row * f.ws + s0);
  for (int32_t q = (int32_t)threadIdx.x; q < ((s1 - s0) >> 2); q += 256) {reinterpret_cast<uint2 *>(g)[q] = src[q];}
  __syncthreads();
  const uint32_t inf = 0xFFFFFFFFu, radius = (uint32_t)f.radius, r2 = radius * radius;
  for (int32_t i = r.x0 + (int32_t)threadIdx.x; i < r.x1; i += 256) {
    const uint32_t here = g[i - s0];
    uint32_t best = here == kFieldNoColumn ? inf : here * here;
    for (uint32_t d = 1u; ; ++d) {
      const uint32_t dd = d * d;
      if (dd >= best || d > radius) {break;}
      const int32_t left = i - (int32_t)d, right = i + (int32_t)d;
      if (left < 0 && right >= f.width) {break;}
      if (left >= 0) {
        const uint32_t gl = g[left - s0], v = gl * gl + dd;
        best = (gl != kFieldNoColumn && v < best) ? v : best;
      }
      if (right < f.width) {
        const uint32_t gr = g[right - s0], v = gr * gr + dd;
        best = (gr != kFieldNoColumn && v < best) ? v : best;
      }
    }
    f.d2[(int64_t)row * f.ws + i] = best == inf || best > r2 ? KH_FIELD_FAR : best;
  }
}

// The statistics from the values as they stand: one thread per four cells (16 bytes), workgroups striding over the window; the cells
// of the row padding hold nothing and are skipped.  k_field_rows' reduction: lanes -> wave by shuffles, the four waves through LDS,
// one atomic per non-zero counter and workgroup.
__global__ __launch_bounds__(256) void k_field_count(FieldWindow f, unsigned long long * __restrict__ counts)
{
  __shared__ uint32_t part[4][kFieldCounters];
  const int32_t quads = f.ws >> 2;
  const int64_t total = (int64_t)quads * f.height;
  uint32_t n_obstacles = 0u, n_far = 0u, max_d2 = 0u;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int32_t col = 4 * (int32_t)(q % quads);
    const uint4 v4 = reinterpret_cast<const uint4 *>(f.d2)[q];
    const uint32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int32_t e = 0; e < 4; ++e) {
      if (col + e < f.width) {
        n_obstacles += v[e] == 0u;
        n_far += v[e] == KH_FIELD_FAR;
        max_d2 = v[e] != KH_FIELD_FAR && v[e] > max_d2 ? v[e] : max_d2;
      }
    }
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    n_obstacles += __shfl_xor(n_obstacles, d);
    n_far += __shfl_xor(n_far, d);
    const uint32_t other = __shfl_xor(max_d2, d);
    max_d2 = other > max_d2 ? other : max_d2;
  }
  if ((threadIdx.x & 63) == 0) {
    uint32_t * const mine = part[threadIdx.x >> 6];
    mine[kFieldObstacles] = n_obstacles; mine[kFieldFar] = n_far; mine[kFieldMaxD2] = max_d2;
  }
  __syncthreads();
  if (threadIdx.x < kFieldCounters) {
    const uint32_t a = part[0][threadIdx.x], b = part[1][threadIdx.x], c = part[2][threadIdx.x], e = part[3][threadIdx.x];
    if (threadIdx.x == kFieldMaxD2) {
      const uint32_t ab = a > b ? a : b, ce = c > e ? c : e, v = ab > ce ? ab : ce;
      if (v) {atomicMax(&counts[kFieldMaxD2], (unsigned long long)v);}
    } else {
      const unsigned long long v = (unsigned long long)a + b + c + e;
      if (v) {atomicAdd(&counts[threadIdx.x], v);}
    }
  }
}

void field_changed(void * stream, const FieldWindow & f, uint8_t * d_snapshot, const uint8_t * d_view_cells, int32_t view_ws, const FieldRect & r,
  int32_t * d_result)
{
  const int64_t quads = static_cast<int64_t>(((r.x1 + 3) >> 2) - (r.x0 >> 2)) * (r.y1 - r.y0);
  hipLaunchKernelGGL(k_field_changed, dim3(static_cast<unsigned>((quads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), f, d_snapshot,
    d_view_cells, view_ws, r, d_result);
}

void field_columns_band(void * stream, const FieldWindow & f, const FieldRect & r, int32_t band_rows)
{
  const int32_t quads = ((r.x1 + 3) >> 2) - (r.x0 >> 2), bands = (r.y1 - r.y0 + band_rows - 1) / band_rows;
  hipLaunchKernelGGL(k_field_columns_band, dim3(static_cast<unsigned>((quads + 63) / 64), static_cast<unsigned>(bands)), dim3(64), 0,
    static_cast<hipStream_t>(stream), f, r, band_rows);
}

bool field_rows_region(void * stream, const FieldWindow & f, const FieldRect & r)
{
  const int32_t s0 = (r.x0 - f.radius > 0 ? r.x0 - f.radius : 0) & ~3;
  const int32_t s1 = ((r.x1 + f.radius < f.width ? r.x1 + f.radius : f.width) + 3) & ~3;
  static std::atomic<unsigned long long> done{0};
  allow_dynamic_lds(reinterpret_cast<const void *>(k_field_rows_region), static_cast<int>(kMaxFieldSide * 2), done);
  hipLaunchKernelGGL(k_field_rows_region, dim3(static_cast<unsigned>(r.y1 - r.y0)), dim3(256), static_cast<size_t>(s1 - s0) * 2,
    static_cast<hipStream_t>(stream), f, r, s0, s1);
  return hipPeekAtLastError() == hipSuccess;
}

void field_count(void * stream, const FieldWindow & f, unsigned long long * d_counts)
{
  const int64_t quads = static_cast<int64_t>(f.ws >> 2) * f.height;
  const int64_t blocks = (quads + 255) / 256;
  hipLaunchKernelGGL(k_field_count, dim3(static_cast<unsigned>(blocks < 2048 ? blocks : 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), f, d_counts);
}
}  // namespace kh
