// Footprints on a map (kh_map_footprint_*): an oriented convex polygon checked against the snapshot of a
// distance field's window -- at poses, and at every window cell turned to each of a set of headings.  The rule
// (tests/map_footprint_rule.py states it in numpy):
//
//   vertex cells  V_k of a pose: the host's (libm stays there): round_half_away of the rotated, shifted vertices on the field's lattice;
//                 of the layer: window cell (i, j) + O_hk, the host's rounded rotated vertices of heading h.  All within Chebyshev
//                 distance reach = ceil(r_max * scale) + 1 of the pose's own cell
//   outline       edge k = the cells of RayWalk(V_k -> V_(k + 1) mod n), steps 0 .. length, in the order the vertices were given;
//                 the outline is the union of the edges, a closed 8-connected loop
//   covered       for every row j from the smallest to the largest V_k.y: lo_j and hi_j are the smallest and the largest column of an
//                 outline cell of that row; Covered = {(i, j): lo_j <= i <= hi_j}.  No row of that range is empty
//   record        the covered cells by state -- 100 occupied, 255 free, any other unknown, off the window outside --, their sum, the
//                 smallest d2 under the covered window cells (KH_FIELD_FAR without one); status = the largest of FREE 0, UNKNOWN 1
//                 (n_unknown > 0), OUTSIDE 2 (n_outside > 0), COLLISION 3 (n_occupied > 0), LATTICE 4 (the host's: a vertex beyond
//                 +-2^30 cells: every other field 0, min_d2 KH_FIELD_FAR)
//   layer         bit h of a window cell's mask: the status of the cell's polygon at heading h is <= max_status
//
// The spans come from foot_edge (map_footprint_plan.hpp), the one statement of the outline; the walk is the one walk of section 7m
// (RayWalk), the cell index cell_at's.  Sets, counts, minima and ORs of integers: no execution order shows in any result.  The
// handle: map_footprint.cpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/karto_hip.h"
#include "map_footprint_plan.hpp"
#include "occupancy_walk.hpp"

namespace kh
{
namespace
{
constexpr int32_t kSpanRows = 512;                   // kFootMaxRows = 511 rows of spans per wave
static_assert(kFootMaxRows <= kSpanRows, "a pose's rows fit its wave's spans");

// the spans of one wave in LDS: row r of the pose is lattice row y0 + r, its columns lattice columns
struct LdsSpans
{
  int32_t * lo;
  int32_t * hi;
  int32_t y0;
  __device__ __forceinline__ void fold(int32_t x, int32_t y)
  {
    atomicMin(&lo[y - y0], x); atomicMax(&hi[y - y0], x);
  }
};

// what a lane counts of the covered cells: four named registers and a minimum (three compares, no counter picked by an index, as
// FitCells)
struct FootCounts
{
  uint32_t n_free = 0u, n_occupied = 0u, n_unknown = 0u, n_outside = 0u, min_d2 = KH_FIELD_FAR;
  __device__ __forceinline__ void add(const FieldWindow & f, int32_t x, int32_t y)
  {
    const CellAt at = cell_at(f, x, y);
    if (at.inside) {
      const uint32_t state = f.cells[at.k], d = f.d2[at.k];
      const uint32_t occupied = state == 100u, is_free = state == 255u;
      n_occupied += occupied; n_free += is_free; n_unknown += (occupied | is_free) ^ 1u;
      min_d2 = d < min_d2 ? d : min_d2;
    } else {
      n_outside += 1u;
    }
  }
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {v += __shfl_xor(v, d);}
  return v;
}
}  // namespace

// One wave per pose, four poses per workgroup; every wave runs every barrier, one without a pose (or whose pose left the lattice)
// with nothing to do.  The wave's LDS: lo / hi of up to 511 rows, and the exclusive prefix of the row widths.
//   1  lanes k < n_v hold vertex k; the wave checks the reach bound on all of them (a broken bound sets *error and the pose's record
//      is zeros), takes the row range by shuffles and clears its rows
//   2  lane k walks edge k (foot_edge) and folds its cells into the rows with LDS atomicMin / atomicMax
//   3  the sweep of the covered cells by a flat index: a lane sums the widths of 8 rows, the wave scans the 64 sums by shuffles, the
//      prefix goes to LDS; covered cell t lies in the last row whose prefix is <= t (9 halving steps), lane l takes t = l, l + 64, ..:
//      the wave is full whatever the rows' widths (row by row, a robot's rows of 12 - 25 cells leave most of it idle: DESIGN.md 7t)
//   4  lanes -> wave by shuffles; lane 0 writes the 32-byte record with plain stores.  No global atomic.
__global__ __launch_bounds__(256) void k_footprint_poses(FootJob q, int32_t n, const FootPose * __restrict__ poses, kh_footprint_t * __restrict__ out)
{
  __shared__ int32_t s_lo[4][kSpanRows], s_hi[4][kSpanRows];
  __shared__ uint32_t s_prefix[4][kSpanRows];
  const int32_t wave = (int32_t)(threadIdx.x >> 6), lane = (int32_t)(threadIdx.x & 63);
  const int64_t pose = (int64_t)blockIdx.x * 4 + wave;
  const bool mine = pose < n;
  const FootPose * const p = poses + (mine ? pose : 0);
  const bool lattice = mine && p->lattice != 0;
  bool walk = mine && !lattice;
  int32_t y0 = 0, rows = 0;
  if (walk) {
    const int32_t k = lane < q.n_vertices ? lane : 0;
    const int32_t vx = p->v[2 * k], vy = p->v[2 * k + 1];
    const int64_t ex = (int64_t)vx - p->cx, ey = (int64_t)vy - p->cy;
    const bool within = ex >= -q.reach && ex <= q.reach && ey >= -q.reach && ey <= q.reach && q.reach <= kFootMaxReach;
    if (!__all(within)) {
      if (lane == 0) {*q.error = 1u;}
      walk = false;
    } else {
      int32_t lo_y = vy, hi_y = vy;
#pragma unroll
      for (int32_t d = 32; d >= 1; d >>= 1) {
        const int32_t a = __shfl_xor(lo_y, d), b = __shfl_xor(hi_y, d);
        lo_y = a < lo_y ? a : lo_y; hi_y = b > hi_y ? b : hi_y;
      }
      y0 = lo_y; rows = hi_y - lo_y + 1;             // (<= 2 reach + 1 <= 511)
    }
  }
  int32_t * const lo = s_lo[wave];
  int32_t * const hi = s_hi[wave];
  for (int32_t r = lane; r < rows; r += 64) {lo[r] = INT32_MAX; hi[r] = INT32_MIN;}
  __syncthreads();

  if (walk && lane < q.n_vertices) {
    LdsSpans spans{lo, hi, y0};
    foot_edge(p->v, q.n_vertices, lane, spans);
  }
  __syncthreads();

  FootCounts c;
  uint32_t * const prefix = s_prefix[wave];
  uint32_t width[8], mine_sum = 0u;
#pragma unroll
  for (int32_t e = 0; e < 8; ++e) {
    const int32_t r = 8 * lane + e;
    width[e] = r < rows && hi[r] >= lo[r] ? (uint32_t)(hi[r] - lo[r]) + 1u : 0u;
    mine_sum += width[e];
  }
  uint32_t upto = mine_sum;                           // inclusive scan over the lanes
#pragma unroll
  for (int32_t d = 1; d < 64; d <<= 1) {
    const uint32_t below = __shfl_up(upto, d);
    if (lane >= d) {upto += below;}
  }
  const uint32_t total = __shfl(upto, 63);
  uint32_t at = upto - mine_sum;
#pragma unroll
  for (int32_t e = 0; e < 8; ++e) {
    prefix[8 * lane + e] = at;
    at += width[e];
  }
  __syncthreads();
  for (uint32_t t = (uint32_t)lane; t < total; t += 64u) {
    int32_t r = 0;
#pragma unroll
    for (int32_t step = 256; step >= 1; step >>= 1) {
      const int32_t m = r + step;
      if (m < rows && prefix[m] <= t) {r = m;}
    }
    c.add(q.f, lo[r] + (int32_t)(t - prefix[r]), y0 + r);
  }

  const uint32_t n_free = wave_sum(c.n_free), n_occupied = wave_sum(c.n_occupied), n_unknown = wave_sum(c.n_unknown), n_outside = wave_sum(c.n_outside);
  uint32_t min_d2 = c.min_d2;
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    const uint32_t other = __shfl_xor(min_d2, d);
    min_d2 = other < min_d2 ? other : min_d2;
  }
  if (mine && lane == 0) {
    kh_footprint_t r;
    r.status = lattice ? KH_FOOTPRINT_LATTICE : n_occupied > 0u ? KH_FOOTPRINT_COLLISION : n_outside > 0u ? KH_FOOTPRINT_OUTSIDE :
      n_unknown > 0u ? KH_FOOTPRINT_UNKNOWN : KH_FOOTPRINT_FREE;
    r.n_cells = n_free + n_occupied + n_unknown + n_outside; r.n_free = n_free; r.n_occupied = n_occupied; r.n_unknown = n_unknown; r.n_outside = n_outside;
    r.min_d2 = min_d2; r.pad = 0u;
    out[pose] = r;
  }
}

namespace
{
constexpr int32_t kLayerTileW = 64, kLayerTileH = 16;                                  // the tile of merge, regions and travel
constexpr int32_t kLayerCols = kLayerTileW + 2 * kFootLayerMaxReach;                   // 192 staged columns at most
constexpr int32_t kLayerRows = kLayerTileH + 2 * kFootLayerMaxReach;                   // 144 staged rows at most
constexpr int32_t kLayerStride = kLayerCols + 4;                                       // a row's prefix counts: entries 0 .. cols
constexpr int32_t kLayerCounters = kFootMaxHeadings + 2;
static_assert(kLayerCols <= 255, "a row's prefix count fits a byte");
static_assert(kLayerCols <= 4 * 64, "one wave stages a row, four columns a lane");
static_assert(sizeof(kh_footprint_layer_t) == 8 * kLayerCounters, "the counters are the summary");
}  // namespace

// One workgroup of 256 threads per 64 x 16 tile of the window.  Only "status <= max_status" is asked, so a cell's part in it is one
// bit: it blocks when it is occupied; when it is unknown and max_status < 1; when it is off the window and max_status < 2.
//   1  the bit of the tile plus a halo of reach cells goes into LDS as per-row exclusive prefix counts, one byte each (a row holds at
//      most 192 cells): a wave stages a row, a lane four columns of it, the 64 sums scanned by shuffles
//   2  a thread takes the cells of its lane's column in rows wave, wave + 4, .. of the tile; per heading it runs down the stencil's
//      rows (the host's table, made by foot_spans): a span is free of blocking cells where the prefix counts at its two ends are
//      equal -- two reads and a compare -- and the heading is dropped at the first span that is not.  The mask word goes out dense
//   3  the counters: lanes -> wave by ballots, the waves through LDS, one atomic per non-zero counter and workgroup
__global__ __launch_bounds__(256) void k_footprint_layer(FootJob q, int32_t n_headings, int32_t max_status, const int32_t * __restrict__ table,
  uint32_t * __restrict__ masks, unsigned long long * __restrict__ counts)
{
  __shared__ uint8_t s_prefix[kLayerRows * kLayerStride];
  __shared__ uint32_t s_counts[kLayerCounters];
  const FieldWindow & f = q.f;
  const int32_t wave = (int32_t)(threadIdx.x >> 6), lane = (int32_t)(threadIdx.x & 63);
  const int32_t reach = q.reach < kFootLayerMaxReach ? q.reach : kFootLayerMaxReach;      // (the host refused a larger one)
  const int32_t tx0 = (int32_t)blockIdx.x * kLayerTileW, ty0 = (int32_t)blockIdx.y * kLayerTileH;
  const int32_t cols = kLayerTileW + 2 * reach, rows = kLayerTileH + 2 * reach;
  if (threadIdx.x < (uint32_t)kLayerCounters) {s_counts[threadIdx.x] = 0u;}
  const uint32_t unknown_blocks = max_status < KH_FOOTPRINT_UNKNOWN, outside_blocks = max_status < KH_FOOTPRINT_OUTSIDE;
  for (int32_t r = wave; r < rows; r += 4) {
    const int32_t wy = ty0 - reach + r;
    uint32_t bit[4], mine_sum = 0u;
#pragma unroll
    for (int32_t e = 0; e < 4; ++e) {
      const int32_t wx = tx0 - reach + 4 * lane + e;
      uint32_t b = 0u;
      if (4 * lane + e < cols) {
        if (wx >= 0 && wx < f.width && wy >= 0 && wy < f.height) {
          const uint32_t state = f.cells[wx + (int64_t)wy * f.ws];
          b = state == 100u ? 1u : state == 255u ? 0u : unknown_blocks;
        } else {
          b = outside_blocks;
        }
      }
      bit[e] = b; mine_sum += b;
    }
    uint32_t upto = mine_sum;
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
      const uint32_t below = __shfl_up(upto, d);
      if (lane >= d) {upto += below;}
    }
    uint32_t at = upto - mine_sum;                    // blocking cells of the row before column 4 lane
    uint8_t * const row = s_prefix + r * kLayerStride;
    if (lane == 0) {row[0] = 0;}
#pragma unroll
    for (int32_t e = 0; e < 4; ++e) {
      at += bit[e];
      if (4 * lane + e < cols) {row[4 * lane + e + 1] = (uint8_t)at;}
    }
  }
  __syncthreads();

  uint32_t mask[4];
  const uint32_t full = n_headings >= 32 ? 0xFFFFFFFFu : (1u << n_headings) - 1u;
#pragma unroll
  for (int32_t e = 0; e < 4; ++e) {
    const int32_t ly = wave + 4 * e, wx = tx0 + lane, wy = ty0 + ly;
    uint32_t m = 0u;
    if (wx < f.width && wy < f.height) {
      for (int32_t h = 0; h < n_headings; ++h) {
        const int32_t first = table[4 * h], dy = table[4 * h + 1], n_rows = table[4 * h + 2];
        const uint8_t * row = s_prefix + (ly + reach + dy) * kLayerStride + lane + reach;
        bool blocked = false;
        for (int32_t r = 0; r < n_rows && !blocked; ++r, row += kLayerStride) {
          blocked = row[table[first + 2 * r + 1] + 1] != row[table[first + 2 * r]];
        }
        m |= (blocked ? 0u : 1u) << h;
      }
      if (masks != nullptr) {masks[(int64_t)wy * f.width + wx] = m;}
    }
    mask[e] = m;
  }
  for (int32_t h = 0; h < n_headings; ++h) {
    uint32_t sum = 0u;
#pragma unroll
    for (int32_t e = 0; e < 4; ++e) {sum += (uint32_t)__popcll(__ballot((mask[e] >> h) & 1u));}
    if (lane == 0 && sum != 0u) {atomicAdd(&s_counts[h], sum);}
  }
  uint32_t any = 0u, all = 0u;
#pragma unroll
  for (int32_t e = 0; e < 4; ++e) {
    any += (uint32_t)__popcll(__ballot(mask[e] != 0u)); all += (uint32_t)__popcll(__ballot(mask[e] == full));
  }
  if (lane == 0) {
    if (any != 0u) {atomicAdd(&s_counts[kFootMaxHeadings], any);}
    if (all != 0u) {atomicAdd(&s_counts[kFootMaxHeadings + 1], all);}
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)kLayerCounters && s_counts[threadIdx.x] != 0u) {atomicAdd(&counts[threadIdx.x], (unsigned long long)s_counts[threadIdx.x]);}
}

void footprint_poses(void * stream, const FootJob & job, int32_t n, const FootPose * d_poses, kh_footprint_t * d_out)
{
  const dim3 blocks(static_cast<unsigned>((static_cast<int64_t>(n) + 3) / 4));
  hipLaunchKernelGGL(k_footprint_poses, blocks, dim3(256), 0, static_cast<hipStream_t>(stream), job, n, d_poses, d_out);
}

void footprint_layer(void * stream, const FootJob & job, int32_t n_headings, int32_t max_status, const int32_t * d_table, uint32_t * d_masks,
  unsigned long long * d_counts)
{
  const dim3 blocks(static_cast<unsigned>((job.f.width + kLayerTileW - 1) / kLayerTileW), static_cast<unsigned>((job.f.height + kLayerTileH - 1) / kLayerTileH));
  hipLaunchKernelGGL(k_footprint_layer, blocks, dim3(256), 0, static_cast<hipStream_t>(stream), job, n_headings, max_status, d_table, d_masks, d_counts);
}
}  // namespace kh
