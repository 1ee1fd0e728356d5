// Travel costs on a map (kh_map_travel_*): the least cost of travelling from every traversable cell of a
// distance field's window to the nearest of a set of goal cells, and its readers.  The rule, as tests/map_travel_rule.py states it:
//   traversable  state 255 and d2 >= Rc * Rc (KH_FIELD_FAR counts as beyond); cells outside the window do not exist, the row padding of
//                the field's arrays is never read
//   weight       q(v) = neutral_cost + ((cost_weight * c(v)) >> 4) for a traversable cell, c(v) = table[d2] for d2 <= Rt * Rt, else 0;
//                q = 0 for every other cell
//   steps        n = 0 .. 7: (+1,0), (0,+1), (-1,0), (0,-1), (+1,+1), (-1,+1), (-1,-1), (+1,-1); connectivity 4 has 0 .. 3 only;
//                L(n) = 5 for n < 4, else 7.  u -> v is allowed when v is a traversable window cell; a diagonal step (di, dj) from
//                (i, j) only with cut_corners, or when both (i + di, j) and (i, j + dj) are traversable.  The step costs L(n) * q(u).
//   values       V = 0 at a goal cell; elsewhere the minimum over allowed steps u -> v of V(v) + L * q(u); KH_TRAVEL_FAR where no goal
//                is reached and at every cell that is not traversable
//   goal cell    the traversable window cell within Chebyshev distance `snap` of the point's cell of the smallest key
//                dist2 << 32 | window index
//   lookup       the window cell within Chebyshev distance `snap` of the point's cell of the smallest key V << 32 | window index
//                among those with V != KH_TRAVEL_FAR
//   path         from the lookup's cell, while V(cur) != 0 to the allowed neighbour v of the smallest n with V(v) + L * q(cur) == V(cur)
// The pipeline: k_travel_weights makes q; k_travel_goals finds the goal cells, sets V = 0 there and flags their tiles;
// k_travel_relax, the hot path, is launched until a launch flags nothing; k_travel_count, k_travel_lookup, k_travel_paths read.
// Across tiles: a tile's interior is written by that tile's workgroup alone and a tile runs at most once per launch, so no store
// races and no atomic decides a value.  A halo read of a neighbour that is being written in the same launch may be stale: every value
// ever stored is the cost of a real path -- an upper bound of the answer -- and values only fall, so a stale value is only a worse
// bound, and the neighbour that lowered a cell of its perimeter flags this tile for the next launch whatever this tile saw.  The
// launch boundary makes the new values visible.  No workgroup waits for another: no flag is spun on, there is no grid barrier.
// Every sum fits: a stored value is the cost of a simple path (a walk that came back to a cell would have to lower it to more than
// it held), and kh_map_travel_create refused a window whose longest simple path could reach KH_TRAVEL_FAR.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/karto_hip.h"
#include "map_travel_plan.hpp"
#include "occupancy_walk.hpp"

namespace kh
{
namespace
{
constexpr uint32_t kFar = kTravelFar;
constexpr int32_t kHaloW = kTravelTileW + 2, kHaloH = kTravelTileH + 2;

__device__ __forceinline__ void travel_lost(unsigned long long * counters) {atomicMax(&counters[kTravelError], 1ull);}

// the directions u = (i, j) may step in, as a mask, from the weights around it: at(di, dj) is the weight of (i + di, j + dj), 0 where
// the window has no such cell
template <typename At>
__device__ __forceinline__ uint32_t allowed_steps(const At & at, bool conn8, bool cut)
{
  uint32_t mask = 0u;
#pragma unroll
  for (int32_t n = 0; n < 8; ++n) {
    const int32_t di = travel_di(n), dj = travel_dj(n);
    bool ok = at(di, dj) != 0u;
    if (n >= 4) {ok = ok && conn8 && (cut || (at(di, 0) != 0u && at(0, dj) != 0u));}
    mask |= ok ? 1u << n : 0u;
  }
  return mask;
}

// the lattice cell of a point and whether the window holds it (k_field_lookup's cell and guards)
struct PointCell {int64_t wx, wy; bool inside;};
__device__ __forceinline__ PointCell point_cell(const FieldWindow & f, double x, double y)
{
  const int32_t cx = occ_cell(x, f.ax, f.scale), cy = occ_cell(y, f.ay, f.scale);
  const int32_t limit = 1 << 30;
  if (!(cx >= -limit && cx <= limit && cy >= -limit && cy <= limit)) {return PointCell{0, 0, false};}
  const CellAt at = cell_at(f, cx, cy);
  return PointCell{at.wx, at.wy, at.inside};
}

// The snap square's key minimum around window cell (wx, wy), one lane: the cell of the smallest key V << 32 | window index among the
// window cells within Chebyshev distance `snap` that hold a value; ~0 without one.
__device__ __forceinline__ unsigned long long nearest_valued(const TravelJob & job, int64_t wx, int64_t wy, int32_t snap)
{
  unsigned long long best = ~0ull;
  const int32_t width = job.f.width, height = job.f.height;
  for (int64_t j = wy - snap; j <= wy + snap; ++j) {
    if (j < 0 || j >= height) {continue;}
    for (int64_t i = wx - snap; i <= wx + snap; ++i) {
      if (i < 0 || i >= width) {continue;}
      const int64_t index = j * width + i;
      const uint32_t value = job.v[index];
      const unsigned long long key = ((unsigned long long)value << 32) | (unsigned long long)index;
      if (value != kFar && key < best) {best = key;}
    }
  }
  return best;
}
}  // namespace

// The weights: one thread per window cell, one pass over the field's states and values.  The table has Rt * Rt + 1 entries -- up to a
// megabyte: it is read where it lies, through the caches (a default curve at 0.05 m is 122 bytes).  The traversable count takes one
// atomic per wave.
__global__ __launch_bounds__(256) void k_travel_weights(TravelJob job, uint32_t rc2, const uint8_t * __restrict__ table, uint32_t rt2, uint32_t neutral_cost,
  uint32_t cost_weight)
{
  const FieldWindow & f = job.f;
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x, cells = (int64_t)f.width * f.height;
  uint32_t q = 0u;
  if (x < cells) {
    const int32_t j = (int32_t)(x / f.width), i = (int32_t)(x - (int64_t)j * f.width);
    const int64_t at = (int64_t)j * f.ws + i;
    const uint32_t d2 = f.d2[at];
    if (f.cells[at] == 255u && d2 >= rc2) {
      const uint32_t c = cost_weight != 0u && d2 <= rt2 ? table[d2] : 0u;
      q = travel_weight(neutral_cost, cost_weight, c);
    }
    job.q[x] = (uint16_t)q;
  }
  const unsigned long long set = __ballot(q != 0u);
  if ((threadIdx.x & 63) == 0 && set) {atomicAdd(&job.counters[kTravelTraversable], (unsigned long long)__builtin_popcountll(set));}
}

// The goals: one wave per goal.  The lanes share out the snap square (at most 33 x 33 cells), each keeps the least key
// dist2 << 32 | window index of its traversable cells, the wave takes the minimum by shuffles (k_map_seeds' idiom, no atomics).  Lane 0
// writes the status and the cell, V = 0 there, and flags the cell's tile and every neighbour of that tile for the first launch: a
// goal on a tile's edge is a value its neighbours have not seen.  Two goals may share a cell or a tile: they store the same words.
__global__ __launch_bounds__(256) void k_travel_goals(TravelJob job, int32_t n, const double * __restrict__ xy, int32_t snap, int32_t * __restrict__ status,
  uint32_t * __restrict__ cell)
{
  const int32_t lane = threadIdx.x & 63, k = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (k >= n) {return;}
  const FieldWindow & f = job.f;
  const PointCell p = point_cell(f, xy[2 * (int64_t)k], xy[2 * (int64_t)k + 1]);
  if (!p.inside) {
    if (lane == 0) {status[k] = KH_TRAVEL_GOAL_OUTSIDE; cell[k] = kFar;}
    return;
  }
  const int32_t side = 2 * snap + 1;
  unsigned long long best = ~0ull;
  for (int32_t s = lane; s < side * side; s += 64) {
    const int64_t dj = s / side - snap, di = s % side - snap, i = p.wx + di, j = p.wy + dj;
    if (i < 0 || i >= f.width || j < 0 || j >= f.height) {continue;}
    const int64_t index = j * f.width + i;
    if (job.q[index] == 0u) {continue;}
    const unsigned long long key = ((unsigned long long)(di * di + dj * dj) << 32) | (unsigned long long)index;
    best = key < best ? key : best;
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    best = o < best ? o : best;
  }
  if (lane != 0) {return;}
  if (best == ~0ull) {status[k] = KH_TRAVEL_GOAL_BLOCKED; cell[k] = kFar; return;}
  const uint32_t index = (uint32_t)(best & 0xFFFFFFFFull);
  status[k] = KH_TRAVEL_GOAL_OK; cell[k] = index;
  job.v[index] = 0u;
  const TravelGrid g = travel_grid(f.width, f.height);
  const int32_t tx = (int32_t)(index % (uint32_t)f.width) / kTravelTileW, ty = (int32_t)(index / (uint32_t)f.width) / kTravelTileH;
  for (int32_t y = max(ty - 1, 0); y <= min(ty + 1, g.tiles_y - 1); ++y) {
    for (int32_t x = max(tx - 1, 0); x <= min(tx + 1, g.tiles_x - 1); ++x) {job.flags[(int64_t)y * g.tiles_x + x] = 1u;}
  }
}

// The relaxation, one workgroup per 64 x 16 tile; a tile without a flag leaves at once.  The workgroup loads its tile of V and q and
// a one-cell halo into LDS (cells off the window: q = 0, V = FAR), wave w takes rows 4 w .. 4 w + 3, a lane one column.  A cell's
// allowed directions and its two step costs are worked out once; then every cell pulls V(u) = min(V(u), V(v) + L q(u)) from LDS, in
// place -- and every row is swept along its lanes in registers (relax_row below) --, until a workgroup-wide OR says that a whole pass
// changed nothing -- a pass that changed nothing read only final values, so the tile is at the fixed point of its halo.  Other waves write the words a pass reads: a 32-bit LDS word is read whole, and it
// holds the cost of a real path whichever write the read meets.  A pass makes final every cell whose best path has one step more than
// the cells final before it, and a best path inside the tile has at most as many steps as the tile has cells: pass
// kTravelTileCells + 1 changes nothing in a correct run, and one that does sets the error word.  The lowered cells go back with plain
// stores; a lowered perimeter cell flags the tiles that can step to it for the next launch.
__global__ __launch_bounds__(256) void k_travel_relax(TravelJob job, uint32_t parity, uint32_t * __restrict__ any)
{
  __shared__ uint32_t val[kHaloH][kHaloW];
  __shared__ uint16_t wq[kHaloH][kHaloW];
  __shared__ uint32_t lowered_bits;
  const int32_t width = job.f.width, height = job.f.height;
  const int32_t tiles_x = (int32_t)gridDim.x, tiles_y = (int32_t)gridDim.y, tx = (int32_t)blockIdx.x, ty = (int32_t)blockIdx.y;
  const int64_t tiles = (int64_t)tiles_x * tiles_y, tile = (int64_t)ty * tiles_x + tx;
  uint32_t * const mine_flag = job.flags + (int64_t)parity * tiles + tile;
  if (*mine_flag == 0u) {return;}
  const int32_t x0 = tx * kTravelTileW, y0 = ty * kTravelTileH;
  for (int32_t k = (int32_t)threadIdx.x; k < kHaloH * kHaloW; k += 256) {
    const int32_t r = k / kHaloW, c = k - r * kHaloW, i = x0 - 1 + c, j = y0 - 1 + r;
    const bool inside = i >= 0 && i < width && j >= 0 && j < height;
    const int64_t index = (int64_t)j * width + i;
    val[r][c] = inside ? job.v[index] : kFar;
    wq[r][c] = inside ? job.q[index] : (uint16_t)0;
  }
  if (threadIdx.x == 0) {lowered_bits = 0u;}
  __syncthreads();
  if (threadIdx.x == 0) {
    *mine_flag = 0u;                                         // read by every thread above; only this workgroup touches the word in this launch
    atomicAdd(&job.counters[kTravelRuns], 1ull);
  }
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane + 1;
  const bool conn8 = job.conn8 != 0, cut = job.cut_corners != 0;
  // Per row, once: the allowed directions, the weight, and what the row sweep needs.  Along a row every step between two traversable
  // cells is allowed, and the way from lane i to lane k < i costs 5 q summed over lanes k + 1 .. i -- a difference of the prefix sums
  // P --, to lane k > i 5 q over lanes i .. k - 1.  run_left / run_right count the traversable cells from the lane on, itself included:
  // a lane d away lies in the same stretch when the count is above d.  span_left[s] / span_right[s] is the way to the lane 2^s away.
  uint32_t steps[4], weight[4], first[4], run_left[4], run_right[4], span_left[4][6], span_right[4][6];
#pragma unroll
  for (int32_t e = 0; e < 4; ++e) {
    const int32_t r = 4 * wave + e + 1;
    const uint32_t q = wq[r][c];
    steps[e] = q != 0u ? allowed_steps([&](int32_t di, int32_t dj) {return (uint32_t)wq[r + dj][c + di];}, conn8, cut) : 0u;
    weight[e] = q;
    first[e] = val[r][c];
    const unsigned long long set = __ballot(q != 0u), below = ~set & ((1ull << lane) - 1ull), above = ~set & ~((2ull << lane) - 1ull);
    run_left[e] = q != 0u ? (uint32_t)(lane + 1 - (below ? 64 - __builtin_clzll(below) : 0)) : 0u;
    run_right[e] = q != 0u ? (uint32_t)((above ? __builtin_ctzll(above) : 64) - lane) : 0u;
    uint32_t prefix = 5u * q;
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(prefix, d);
      if (lane >= d) {prefix += o;}
    }
    const uint32_t before = prefix - 5u * q;
#pragma unroll
    for (int32_t s = 0; s < 6; ++s) {
      span_left[e][s] = prefix - (uint32_t)__shfl_up(prefix, 1 << s);
      span_right[e][s] = (uint32_t)__shfl_down(before, 1 << s) - before;
    }
  }
  volatile uint32_t * const live = &val[0][0];               // every pass reads the words as they are
  // One row of a pass: the pull from the eight neighbours in LDS, then the sweep along the row in registers -- a min-plus scan by
  // doubling, to the right and to the left, which carries a value across a whole stretch of the row in one pass where the pulls alone
  // carry it one cell.  Every candidate is the cost of a real path.  Every lane of the wave takes part in the shuffles.
  bool changed = false;
  const auto relax_row = [&](const int32_t e) {
    const int32_t r = 4 * wave + e + 1;
    const uint32_t now = live[r * kHaloW + c], cost5 = 5u * weight[e], cost7 = 7u * weight[e];
    uint32_t best = now;
#pragma unroll
    for (int32_t n = 0; n < 8; ++n) {
      if (!((steps[e] >> n) & 1u)) {continue;}
      const uint32_t there = live[(r + travel_dj(n)) * kHaloW + c + travel_di(n)];
      const uint32_t through = there + (n < 4 ? cost5 : cost7);
      if (there != kFar && through < best) {best = through;}
    }
#pragma unroll
    for (int32_t s = 0; s < 6; ++s) {
      const uint32_t there = __shfl_up(best, 1 << s), through = there + span_left[e][s];
      if (run_left[e] > (1u << s) && there != kFar && through < best) {best = through;}
    }
#pragma unroll
    for (int32_t s = 0; s < 6; ++s) {
      const uint32_t there = __shfl_down(best, 1 << s), through = there + span_right[e][s];
      if (run_right[e] > (1u << s) && there != kFar && through < best) {best = through;}
    }
    if (best < now) {live[r * kHaloW + c] = best; changed = true;}
  };
  // The rows of a wave go top-down in odd passes and bottom-up in even ones: a row reads what the row before it has just stored, so
  // a value crosses the wave's four rows in one pass either way.
  bool lost = false;
  for (int32_t pass = 1; ; ++pass) {
    changed = false;
    if (pass & 1) {
      relax_row(0); relax_row(1); relax_row(2); relax_row(3);
    } else {
      relax_row(3); relax_row(2); relax_row(1); relax_row(0);
    }
    if (!__syncthreads_or(changed ? 1 : 0)) {break;}
    if (pass > kTravelTileCells) {lost = true; break;}
  }
  uint32_t lowered = 0u;
#pragma unroll
  for (int32_t e = 0; e < 4; ++e) {
    const int32_t row = 4 * wave + e, r = row + 1, i = x0 + lane, j = y0 + row;
    const uint32_t now = val[r][c];
    if (now < first[e]) {
      job.v[(int64_t)j * width + i] = now;                   // a lowered cell is a traversable window cell
      const bool right = lane == kTravelTileW - 1, left = lane == 0, bottom = row == kTravelTileH - 1, top = row == 0;
      lowered |= (right ? 1u : 0u) | (bottom ? 2u : 0u) | (left ? 4u : 0u) | (top ? 8u : 0u) | (right && bottom ? 16u : 0u) | (left && bottom ? 32u : 0u) |
                 (left && top ? 64u : 0u) | (right && top ? 128u : 0u);
    }
  }
  if (lowered) {atomicOr(&lowered_bits, lowered);}           // an OR in LDS: no order shows in it
  __syncthreads();
  if (threadIdx.x < 8) {
    const int32_t n = (int32_t)threadIdx.x;
    if ((travel_flagged(tx, ty, tiles_x, tiles_y, conn8, lowered_bits) >> n) & 1u) {
      job.flags[(int64_t)(parity ^ 1u) * tiles + (int64_t)(ty + travel_dj(n)) * tiles_x + (tx + travel_di(n))] = 1u;
      *any = 1u;
    }
  }
  if (lost && threadIdx.x == 0) {travel_lost(job.counters);}
}

// the cells that hold a value and the largest of the values: one atomic per wave and counter
__global__ __launch_bounds__(256) void k_travel_count(TravelJob job, int64_t cells)
{
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t value = x < cells ? job.v[x] : kFar;
  const unsigned long long reached = __ballot(value != kFar);
  if (!reached) {return;}
  uint32_t top = value != kFar ? value : 0u;
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {top = max(top, (uint32_t)__shfl_xor(top, d));}
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&job.counters[kTravelReached], (unsigned long long)__builtin_popcountll(reached));
    atomicMax(&job.counters[kTravelMaxValue], (unsigned long long)top);
  }
}

// The value at a point: k_field_lookup's cell and guards, then the snap square's key minimum; one thread per point.
__global__ __launch_bounds__(256) void k_travel_lookup(TravelJob job, int32_t n, const double * __restrict__ xy, int32_t snap, TravelAt * __restrict__ out)
{
  const int32_t k = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (k >= n) {return;}
  const PointCell p = point_cell(job.f, xy[2 * (int64_t)k], xy[2 * (int64_t)k + 1]);
  TravelAt a{KH_TRAVEL_AT_OUTSIDE, kFar, 0, 0};
  if (p.inside) {
    const unsigned long long key = nearest_valued(job, p.wx, p.wy, snap);
    a.status = KH_TRAVEL_AT_UNREACHED;
    if (key != ~0ull) {
      const uint32_t index = (uint32_t)(key & 0xFFFFFFFFull);
      a = TravelAt{KH_TRAVEL_AT_OK, (uint32_t)(key >> 32), job.f.ox + (int32_t)(index % (uint32_t)job.f.width), job.f.oy + (int32_t)(index / (uint32_t)job.f.width)};
    }
  }
  out[k] = a;
}

// The paths: one lane per start walks its path -- a chain of dependent loads, latency-bound like k_map_raycast, and the lanes of a
// wave wait for its longest path.  From the lookup's cell; at every cell the allowed directions are worked out from the weights around
// it as the relaxation does, and the walk takes the first that explains the cell's value.  V falls with every step, so the walk ends; a
// cell that no neighbour explains cannot occur in a solved field: the walk ends there and the error word is set.
__global__ __launch_bounds__(64) void k_travel_paths(TravelJob job, int32_t n, const double * __restrict__ xy, int32_t snap, int32_t max_cells,
  TravelHead * __restrict__ heads, int32_t * __restrict__ cells)
{
  const int32_t k = (int32_t)(blockIdx.x * 64 + threadIdx.x);
  if (k >= n) {return;}
  const int32_t width = job.f.width, height = job.f.height;
  const PointCell p = point_cell(job.f, xy[2 * (int64_t)k], xy[2 * (int64_t)k + 1]);
  TravelHead head{KH_TRAVEL_PATH_OUTSIDE, 0, kFar, kFar};
  if (p.inside) {
    const unsigned long long key = nearest_valued(job, p.wx, p.wy, snap);
    head.status = KH_TRAVEL_PATH_UNREACHED;
    if (key != ~0ull) {
      head.start_cell = (uint32_t)(key & 0xFFFFFFFFull); head.cost = (uint32_t)(key >> 32);
      int32_t i = (int32_t)(head.start_cell % (uint32_t)width), j = (int32_t)(head.start_cell / (uint32_t)width);
      uint32_t value = head.cost;
      int32_t * const mine = cells ? cells + 2 * (int64_t)k * max_cells : nullptr;
      const bool conn8 = job.conn8 != 0, cut = job.cut_corners != 0;
      for (;;) {
        if (mine) {mine[2 * (int64_t)head.n_cells] = job.f.ox + i; mine[2 * (int64_t)head.n_cells + 1] = job.f.oy + j;}
        ++head.n_cells;
        if (value == 0u) {head.status = KH_TRAVEL_PATH_OK; break;}
        if (head.n_cells == max_cells) {head.status = KH_TRAVEL_PATH_TRUNCATED; break;}
        const auto weight_at = [&](int32_t di, int32_t dj) {
          const int32_t a = i + di, b = j + dj;
          return a >= 0 && a < width && b >= 0 && b < height ? (uint32_t)job.q[(int64_t)b * width + a] : 0u;
        };
        const uint32_t steps = allowed_steps(weight_at, conn8, cut), q = weight_at(0, 0);
        int32_t next = -1;
        uint32_t there = 0u;
        for (int32_t s = 0; s < 8 && next < 0; ++s) {
          if (!((steps >> s) & 1u)) {continue;}
          there = job.v[(int64_t)(j + travel_dj(s)) * width + (i + travel_di(s))];
          if (there != kFar && there + travel_length(s) * q == value) {next = s;}
        }
        if (next < 0) {travel_lost(job.counters); head.status = KH_TRAVEL_PATH_UNREACHED; break;}
        i += travel_di(next); j += travel_dj(next); value = there;
      }
    }
  }
  heads[k] = head;
}

namespace
{
int64_t cells_of(const TravelJob & job) {return static_cast<int64_t>(job.f.width) * job.f.height;}
dim3 per_cell(const TravelJob & job) {return dim3(static_cast<unsigned>((cells_of(job) + 255) / 256));}
}  // namespace

void travel_weights(void * stream, const TravelJob & job, uint32_t rc2, const uint8_t * d_table, uint32_t rt2, uint32_t neutral_cost, uint32_t cost_weight)
{
  hipLaunchKernelGGL(k_travel_weights, per_cell(job), dim3(256), 0, static_cast<hipStream_t>(stream), job, rc2, d_table, rt2, neutral_cost, cost_weight);
}

void travel_goals(void * stream, const TravelJob & job, int32_t n, const double * d_xy, int32_t snap, int32_t * d_status, uint32_t * d_cell)
{
  hipLaunchKernelGGL(k_travel_goals, dim3(static_cast<unsigned>((n + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), job, n, d_xy, snap, d_status, d_cell);
}

void travel_relax(void * stream, const TravelJob & job, uint32_t round, uint32_t * d_any)
{
  const TravelGrid g = travel_grid(job.f.width, job.f.height);
  hipLaunchKernelGGL(k_travel_relax, dim3(static_cast<unsigned>(g.tiles_x), static_cast<unsigned>(g.tiles_y)), dim3(256), 0, static_cast<hipStream_t>(stream), job,
    round & 1u, d_any);
}

void travel_count(void * stream, const TravelJob & job)
{
  hipLaunchKernelGGL(k_travel_count, per_cell(job), dim3(256), 0, static_cast<hipStream_t>(stream), job, cells_of(job));
}

void travel_lookup(void * stream, const TravelJob & job, int32_t n, const double * d_xy, int32_t snap, TravelAt * d_out)
{
  hipLaunchKernelGGL(k_travel_lookup, dim3(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), job, n,
    d_xy, snap, d_out);
}

void travel_paths(void * stream, const TravelJob & job, int32_t n, const double * d_xy, int32_t snap, int32_t max_cells, TravelHead * d_heads, int32_t * d_cells)
{
  hipLaunchKernelGGL(k_travel_paths, dim3(static_cast<unsigned>((static_cast<int64_t>(n) + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), job, n, d_xy,
    snap, max_cells, d_heads, d_cells);
}
}  // namespace kh
