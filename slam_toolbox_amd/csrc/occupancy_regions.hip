// Map regions (kh_map_regions_*): connected-component labelling of two masks of a distance field's window --
// the traversable cells (state 255, d2 >= Rc * Rc) and the frontier cells (state 255 next to an unknown cell) -- and what is kept
// of the components: ids in root order, one record each, the region at a world point.  The rule, as tests/map_regions_rule.py
// states it:
//   N          the 4 or the 8 neighbours of a cell; cells outside the window do not exist, the row padding of the field's arrays is
//              never read and never connects anything
//   label      the root of a component: the window index j * width + i of its smallest cell
//   kept       a component of at least `minimum` cells among the first `maximum` such components in root order, numbered 0, 1, ...
//   id grid    the kept id, KH_REGION_NONE off the mask, KH_REGION_DROPPED for a component too small or past the cap
//   record     root, n_cells, box, sum_i, sum_j, max_d2 (KH_FIELD_FAR is the largest uint32: a plain maximum), n_other (members set
//              in the other mask), link (the smallest kept id of the other set among the members), the anchor key
//              dist2 << 32 | index to the centroid cell ((2 sum_i + n) / (2 n), (2 sum_j + n) / (2 n))
// The pipeline: k_region_tiles labels both masks inside every 64 x 16 tile in LDS; k_region_seams unites cells across tile borders
// by union-find on the global label array; k_region_flatten replaces every parent by the root and counts cells per root;
// k_region_roots / the unit scan / k_region_ids number the kept roots in row-major order with no atomic deciding a position
// (k_map_changed's idiom); k_region_records and k_region_anchor fill the records; k_region_lookup answers points.
// A union links the LARGER root under the smaller one by atomicMin, so a parent is never above its child, a tree's root is its
// smallest cell, and every step of a find or a union moves to a strictly smaller index: every loop ends by construction.  On top of
// that a watchdog count no correct run can reach (the window's cell count) sets the error word and leaves.  No workgroup waits for
// another inside a launch: launch boundaries are the only synchronisation.  Every result is an integer sum, minimum or maximum:
// none depends on the order of an atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/karto_hip.h"
#include "map_regions_plan.hpp"
#include "occupancy_walk.hpp"

namespace kh
{
namespace
{
constexpr uint32_t kNone = KH_REGION_NONE, kDropped = KH_REGION_DROPPED;
constexpr int32_t kTileCells = kRegionTileW * kRegionTileH;

// The label array is written by other workgroups (other waves, for the LDS copy) while a find reads it: every read is an agent-scope
// atomic load, never a plain one that may be served from a stale L1 line.
__device__ __forceinline__ uint32_t label_load(const uint32_t * p) {return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);}

// the root above x; a parent that is not below its child ends the walk
__device__ __forceinline__ uint32_t region_find(const uint32_t * label, uint32_t x, uint32_t limit, bool & lost)
{
  for (uint32_t n = 0; ; ++n) {
    const uint32_t p = label_load(label + x);
    if (p >= x) {return x;}
    if (n >= limit) {lost = true; return x;}
    x = p;
  }
}

// a and b are cells of one component: their trees become one.  Either the larger root takes the smaller as its parent, or another
// union got there first and the walk goes on from what that one left -- a strictly smaller index.
__device__ __forceinline__ void region_unite(uint32_t * label, uint32_t a, uint32_t b, uint32_t limit, bool & lost)
{
  for (uint32_t n = 0; ; ++n) {
    a = region_find(label, a, limit, lost); b = region_find(label, b, limit, lost);
    if (a == b || lost) {return;}
    if (a < b) {const uint32_t t = a; a = b; b = t;}
    const uint32_t old = atomicMin(label + a, b);
    if (old == a) {return;}
    if (n >= limit) {lost = true; return;}
    a = old;
  }
}

__device__ __forceinline__ void region_lost(unsigned long long * counters) {atomicMax(&counters[kRegionError], 1ull);}

__device__ __forceinline__ bool bit_of(unsigned long long m, int32_t lane) {return (m >> lane) & 1ull;}
}  // namespace

// Both masks and their tile-local labels: one workgroup per 64 x 16 tile, wave w takes rows 4 w .. 4 w + 3, a lane one column.  A
// lane reads its cell's state and value and, for a free cell, the states of N (the one-cell halo of the frontier mask, clipped to
// the window).  A tile row is one ballot; a cell's first label is the first cell of its row run, found by bit operations on the
// ballot.  Runs of adjacent rows are joined in LDS: the first lane of every stretch where both rows are set unites with the cell
// above; under 8 neighbours a cell unites with a diagonal cell above only where neither the cell above nor the one beside it already
// makes that connection.  Then every cell follows its chain and stores the GLOBAL index of its tile-local root.
__global__ __launch_bounds__(256) void k_region_tiles(RegionJob job)
{
  __shared__ uint32_t lab[2][kTileCells];
  const FieldWindow & f = job.f;
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t i = (int32_t)blockIdx.x * kRegionTileW + lane, j0 = (int32_t)blockIdx.y * kRegionTileH;
  const bool conn8 = job.conn8 != 0;
  unsigned long long rows[2][4];
  uint32_t n_set[2] = {0u, 0u};
#pragma unroll
  for (int32_t q = 0; q < 4; ++q) {
    const int32_t r = 4 * wave + q, j = j0 + r;
    bool set[2] = {false, false};
    if (i < f.width && j < f.height) {
      const int64_t at = (int64_t)j * f.ws + i;
      if (f.cells[at] == 255u) {
        set[0] = f.d2[at] >= job.rc2;
#pragma unroll
        for (int32_t dj = -1; dj <= 1; ++dj) {
#pragma unroll
          for (int32_t di = -1; di <= 1; ++di) {
            if ((di == 0 && dj == 0) || (!conn8 && di != 0 && dj != 0)) {continue;}
            const int32_t ni = i + di, nj = j + dj;
            if (ni >= 0 && ni < f.width && nj >= 0 && nj < f.height) {
              const uint32_t s = f.cells[(int64_t)nj * f.ws + ni];
              set[1] = set[1] || (s != 100u && s != 255u);
            }
          }
        }
      }
    }
#pragma unroll
    for (int32_t w = 0; w < 2; ++w) {
      const unsigned long long m = __ballot(set[w]);
      const unsigned long long gaps_below = ~m & ((1ull << lane) - 1ull);
      const int32_t start = gaps_below ? 64 - __builtin_clzll(gaps_below) : 0;
      lab[w][r * kRegionTileW + lane] = set[w] ? (uint32_t)(r * kRegionTileW + start) : kNone;
      rows[w][q] = m;
      n_set[w] += (uint32_t)__builtin_popcountll(m);
    }
  }
  const uint32_t mine = lane == 0 ? n_set[0] : n_set[1];       // kRegionTraversable, kRegionFrontierCells: one atomic per wave and counter
  if (lane < 2 && mine) {atomicAdd(&job.counters[kRegionTraversable + lane], (unsigned long long)mine);}
  __syncthreads();
  bool lost = false;
#pragma unroll
  for (int32_t q = 0; q < 4; ++q) {
    const int32_t r = 4 * wave + q;
    if (r == 0) {continue;}
    const uint32_t me = (uint32_t)(r * kRegionTileW + lane);
#pragma unroll
    for (int32_t w = 0; w < 2; ++w) {
      const unsigned long long m = rows[w][q], up = __ballot(label_load(&lab[w][me - kRegionTileW]) != kNone);
      const unsigned long long both = m & up;
      if (bit_of(both & ~(both << 1), lane)) {region_unite(lab[w], me, me - kRegionTileW, kTileCells, lost);}
      if (conn8) {
        if (bit_of(m & (up << 1) & ~up & ~(m << 1), lane)) {region_unite(lab[w], me, me - kRegionTileW - 1, kTileCells, lost);}
        if (bit_of(m & (up >> 1) & ~up & ~(m >> 1), lane)) {region_unite(lab[w], me, me - kRegionTileW + 1, kTileCells, lost);}
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int32_t q = 0; q < 4; ++q) {
    const int32_t r = 4 * wave + q, j = j0 + r;
    if (i >= f.width || j >= f.height) {continue;}
#pragma unroll
    for (int32_t w = 0; w < 2; ++w) {
      uint32_t out = kNone;
      if (bit_of(rows[w][q], lane)) {
        const uint32_t root = region_find(lab[w], (uint32_t)(r * kRegionTileW + lane), kTileCells, lost);
        out = (uint32_t)(j0 + (int32_t)(root / kRegionTileW)) * (uint32_t)f.width + (uint32_t)((int32_t)blockIdx.x * kRegionTileW + (int32_t)(root % kRegionTileW));
      }
      job.set[w].label[(int64_t)j * f.width + i] = out;
    }
  }
  if (lost) {region_lost(job.counters);}
}

// The unions across tile borders, one thread per cell that begins a tile row (but the first) or a tile column (but the first).  The
// first kind looks up -- and under 8 neighbours up-left and up-right, the corner diagonals among them --, the second looks left --
// and left-up and left-down.  Every pair of neighbours in different tiles is met at least once.  Other workgroups link the same
// words in this launch: every access to the label array is an agent-scope atomic (label_load, atomicMin).
__global__ __launch_bounds__(256) void k_region_seams(uint32_t * label, int32_t width, int32_t height, int32_t conn8, int64_t n_rows, int64_t n_all,
  uint32_t limit, unsigned long long * counters)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_all) {return;}
  int32_t i, j, ni[3], nj[3];
  if (t < n_rows) {
    i = (int32_t)(t % width); j = kRegionTileH * (int32_t)(t / width + 1);
    ni[0] = i; ni[1] = i - 1; ni[2] = i + 1; nj[0] = nj[1] = nj[2] = j - 1;
  } else {
    const int64_t u = t - n_rows;
    j = (int32_t)(u % height); i = kRegionTileW * (int32_t)(u / height + 1);
    ni[0] = ni[1] = ni[2] = i - 1; nj[0] = j; nj[1] = j - 1; nj[2] = j + 1;
  }
  const uint32_t me = (uint32_t)j * (uint32_t)width + (uint32_t)i;
  if (label_load(label + me) == kNone) {return;}
  bool lost = false;
#pragma unroll
  for (int32_t k = 0; k < 3; ++k) {
    if ((k > 0 && !conn8) || ni[k] < 0 || ni[k] >= width || nj[k] < 0 || nj[k] >= height) {continue;}
    const uint32_t other = (uint32_t)nj[k] * (uint32_t)width + (uint32_t)ni[k];
    if (label_load(label + other) != kNone) {region_unite(label, me, other, limit, lost);}
  }
  if (lost) {region_lost(counters);}
}

// Every cell follows its chain to the root and stores it (another thread may read the word meanwhile: it finds the old parent or the
// root, both above it in the tree), and the roots count their cells: a wave whose cells share one root adds once.
__global__ __launch_bounds__(256) void k_region_flatten(uint32_t * label, uint32_t * __restrict__ count, int64_t cells, uint32_t limit,
  unsigned long long * counters)
{
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t lane = threadIdx.x & 63;
  bool lost = false;
  const bool member = x < cells && label_load(label + x) != kNone;
  uint32_t root = kNone;
  if (member) {
    root = region_find(label, (uint32_t)x, limit, lost);
    __hip_atomic_store(label + x, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const unsigned long long members = __ballot(member);
  if (members) {
    const int32_t first = __builtin_ctzll(members);
    const uint32_t shared = __shfl(root, first);
    if (__ballot(member && root != shared) == 0ull) {
      if (lane == first) {atomicAdd(count + shared, (uint32_t)__builtin_popcountll(members));}
    } else if (member) {
      atomicAdd(count + root, 1u);
    }
  }
  if (lost) {region_lost(counters);}
}

// The roots that pass the minimum, numbered in row-major order: a wave takes a unit of 64 consecutive window indices; its ballot's
// popcount is the unit's count (count phase), the unit scan turns the counts into their exclusive prefix, and the fill phase repeats
// the ballot: root `lane` of unit u is number prefix[u] + the set bits below the lane.  A number below the maximum is the id and
// begins the record; count[root] becomes the id, or KH_REGION_DROPPED.  Only a root has a count.
template <bool kFill>
__global__ __launch_bounds__(256) void k_region_roots(RegionSet s, int32_t which, int64_t cells, int64_t n_units, int32_t * __restrict__ unit,
  unsigned long long * counters)
{
  const int32_t lane = threadIdx.x & 63;
  const int64_t first = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), step = (int64_t)gridDim.x * 4;
  for (int64_t u = first; u < n_units; u += step) {
    const int64_t x = 64 * u + lane;
    const uint32_t c = x < cells ? s.count[x] : 0u;
    const bool passing = c > 0u && c >= s.minimum;
    const unsigned long long mask = __ballot(passing);
    if (!kFill) {
      const int32_t roots = __builtin_popcountll(__ballot(c > 0u));
      if (lane == 0) {
        unit[u] = __builtin_popcountll(mask);
        if (roots) {atomicAdd(&counters[kRegionTotal + which], (unsigned long long)roots);}
      }
    } else {
      if (u == 0 && lane == 0) {counters[kRegionPassing + which] = (unsigned long long)unit[n_units];}
      if (c > 0u) {
        uint32_t id = kDropped;
        if (passing) {
          const uint32_t at = (uint32_t)unit[u] + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
          if (at < s.maximum) {
            id = at;
            s.records[at] = RegionRecord{(uint32_t)x, c, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, 0ull, 0ull, 0u, 0u, kNone, 0u, ~0ull};
          }
        }
        s.count[x] = id;
      }
    }
  }
}

// label = the id of the cell's root
__global__ __launch_bounds__(256) void k_region_ids(RegionSet s, int64_t cells)
{
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= cells) {return;}
  const uint32_t root = s.label[x];
  if (root != kNone) {s.label[x] = s.count[root];}
}

namespace
{
// The lanes of a wave as runs: consecutive members (id < KH_REGION_DROPPED) that hold one id.  `head`: this lane is the first of its
// run; `last`: the last lane of this lane's run.  A reduction over the runs takes lane + d where that lane is at most `last`, for
// d = 1, 2, 4, ..., 32: afterwards the head holds its run's result.  A wave of one id without a gap is one run.
struct WaveRun {bool head; int32_t last;};
__device__ __forceinline__ WaveRun wave_run(bool member, uint32_t id, int32_t lane)
{
  const uint32_t before = __shfl_up(id, 1);
  const bool head = member && (lane == 0 || before != id);
  const unsigned long long above = __ballot(head || !member) & ~((2ull << lane) - 1ull);
  return WaveRun{head, above ? __builtin_ctzll(above) - 1 : 63};
}
}  // namespace

namespace
{
// what a record gathers of some of its members, and the neutral element of each
struct RegionPart
{
  int32_t x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
  uint32_t sum_i = 0u, sum_j = 0u, max_d2 = 0u, n_other = 0u, link = kNone;      // (a wave's 512 cells x 32767 fit)
  __device__ __forceinline__ void add(int32_t i, int32_t j, uint32_t value, uint32_t other)
  {
    x0 = min(x0, i); y0 = min(y0, j); x1 = max(x1, i); y1 = max(y1, j);
    sum_i += (uint32_t)i; sum_j += (uint32_t)j;
    max_d2 = max(max_d2, value); n_other += other != kNone ? 1u : 0u; link = min(link, other < kDropped ? other : kNone);
  }
  __device__ __forceinline__ void add(const RegionPart & o)
  {
    x0 = min(x0, o.x0); y0 = min(y0, o.y0); x1 = max(x1, o.x1); y1 = max(y1, o.y1);
    sum_i += o.sum_i; sum_j += o.sum_j;
    max_d2 = max(max_d2, o.max_d2); n_other += o.n_other; link = min(link, o.link);
  }
  __device__ __forceinline__ RegionPart down(int32_t d) const
  {
    RegionPart o;
    o.x0 = __shfl_down(x0, d); o.y0 = __shfl_down(y0, d); o.x1 = __shfl_down(x1, d); o.y1 = __shfl_down(y1, d);
    o.sum_i = __shfl_down(sum_i, d); o.sum_j = __shfl_down(sum_j, d);
    o.max_d2 = __shfl_down(max_d2, d); o.n_other = __shfl_down(n_other, d); o.link = __shfl_down(link, d);
    return o;
  }
  // one atomic per counter that can change
  __device__ __forceinline__ void into(RegionRecord * r) const
  {
    atomicMin(&r->x0, x0); atomicMin(&r->y0, y0); atomicMax(&r->x1, x1); atomicMax(&r->y1, y1);
    if (sum_i) {atomicAdd(&r->sum_i, (unsigned long long)sum_i);}
    if (sum_j) {atomicAdd(&r->sum_j, (unsigned long long)sum_j);}
    if (max_d2) {atomicMax(&r->max_d2, max_d2);}
    if (n_other) {atomicAdd(&r->n_other, n_other);}
    if (link != kNone) {atomicMin(&r->link, link);}
  }
};
constexpr int32_t kRecordCells = 8;          // consecutive window indices per thread of k_region_records and k_region_anchor
}  // namespace

// The records of both sets, after both id grids exist.  A thread takes kRecordCells consecutive cells -- their ids and values are
// fetched together, before the first is looked at -- and gathers them in registers while the id stays the same (where it changes
// inside the thread, the part gathered so far goes to its record); then the wave reduces the lanes' last parts per run of one id by
// shuffles -- a wave whose lanes all hold one id is one run -- and the head of a run issues one atomic per counter.  What is merged
// are members of one component, adjacent or not: every counter is an integer add, min or max.
__global__ __launch_bounds__(256) void k_region_records(RegionJob job, int64_t cells)
{
  const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kRecordCells;
  const int32_t lane = threadIdx.x & 63, width = job.f.width;
  const int32_t j0 = first < cells ? (int32_t)(first / width) : 0, i0 = first < cells ? (int32_t)(first - (int64_t)j0 * width) : 0;
  uint32_t ids[2][kRecordCells], value[kRecordCells];
  {
    int32_t i = i0, j = j0;
#pragma unroll
    for (int32_t e = 0; e < kRecordCells; ++e) {
      const bool inside = first + e < cells;
      ids[0][e] = inside ? job.set[0].label[first + e] : kNone;
      ids[1][e] = inside ? job.set[1].label[first + e] : kNone;
      value[e] = inside ? job.f.d2[(int64_t)j * job.f.ws + i] : 0u;
      if (++i == width) {i = 0; ++j;}
    }
  }
#pragma unroll
  for (int32_t w = 0; w < 2; ++w) {
    RegionPart part;
    uint32_t mine = kNone;                   // the id `part` belongs to; KH_REGION_NONE: none yet
    int32_t i = i0, j = j0;
#pragma unroll
    for (int32_t e = 0; e < kRecordCells; ++e) {
      const uint32_t id = ids[w][e];
      if (id < kDropped) {
        if (id != mine) {
          if (mine != kNone) {part.into(job.set[w].records + mine);}
          part = RegionPart();
          mine = id;
        }
        part.add(i, j, value[e], ids[1 - w][e]);
      }
      if (++i == width) {i = 0; ++j;}
    }
    const bool member = mine != kNone;
    if (__ballot(member) == 0ull) {continue;}
    const WaveRun run = wave_run(member, mine, lane);
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
      const RegionPart o = part.down(d);
      if (lane + d <= run.last) {part.add(o);}
    }
    if (run.head) {part.into(job.set[w].records + mine);}
  }
}

// The anchors, once the sums are whole: the 64-bit key minimum dist2 << 32 | index (k_map_seeds' idiom).  k_region_records' shape: a
// thread takes kRecordCells consecutive cells and keeps the least key while the id stays the same -- the centroid cell, two 64-bit
// divisions, is worked out where the id changes, not per cell --, the wave reduces per run of one id, one atomic per run.
__global__ __launch_bounds__(256) void k_region_anchor(RegionJob job, int64_t cells)
{
  const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kRecordCells;
  const int32_t lane = threadIdx.x & 63, width = job.f.width;
  const int32_t j0 = first < cells ? (int32_t)(first / width) : 0, i0 = first < cells ? (int32_t)(first - (int64_t)j0 * width) : 0;
  uint32_t ids[2][kRecordCells];
#pragma unroll
  for (int32_t e = 0; e < kRecordCells; ++e) {
    const bool inside = first + e < cells;
    ids[0][e] = inside ? job.set[0].label[first + e] : kNone;
    ids[1][e] = inside ? job.set[1].label[first + e] : kNone;
  }
#pragma unroll
  for (int32_t w = 0; w < 2; ++w) {
    unsigned long long key = ~0ull;
    uint32_t mine = kNone;
    int64_t ci = 0, cj = 0;
    int32_t i = i0, j = j0;
#pragma unroll
    for (int32_t e = 0; e < kRecordCells; ++e) {
      const uint32_t id = ids[w][e];
      if (id < kDropped) {
        if (id != mine) {
          if (mine != kNone) {atomicMin(&job.set[w].records[mine].anchor_key, key);}
          const RegionRecord * const r = job.set[w].records + id;
          ci = (int64_t)centroid_cell(r->sum_i, r->n_cells); cj = (int64_t)centroid_cell(r->sum_j, r->n_cells);
          key = ~0ull;
          mine = id;
        }
        const int64_t di = i - ci, dj = j - cj;
        const unsigned long long k = ((unsigned long long)(di * di + dj * dj) << 32) | (unsigned long long)(first + e);
        key = k < key ? k : key;
      }
      if (++i == width) {i = 0; ++j;}
    }
    const bool member = mine != kNone;
    if (__ballot(member) == 0ull) {continue;}
    const WaveRun run = wave_run(member, mine, lane);
#pragma unroll
    for (int32_t d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_down(key, d);
      if (lane + d <= run.last && o < key) {key = o;}
    }
    if (run.head) {atomicMin(&job.set[w].records[mine].anchor_key, key);}
  }
}

// The region at a point: k_field_lookup's cell and guards, the id grid's dense index.
__global__ __launch_bounds__(256) void k_region_lookup(FieldWindow f, const uint32_t * __restrict__ ids, int32_t n, const double * __restrict__ xy,
  uint32_t * __restrict__ id, int32_t * __restrict__ status)
{
  const int32_t k = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (k >= n) {return;}
  const int32_t cx = occ_cell(xy[2 * (int64_t)k], f.ax, f.scale), cy = occ_cell(xy[2 * (int64_t)k + 1], f.ay, f.scale);
  const int32_t limit = 1 << 30;
  uint32_t v = kNone;
  int32_t code = KH_REGION_OUTSIDE;
  if (cx >= -limit && cx <= limit && cy >= -limit && cy <= limit) {
    const CellAt at = cell_at(f, cx, cy);
    if (at.inside) {
      v = ids[at.wx + at.wy * f.width];
      code = v == kNone ? KH_REGION_AT_NONE : v == kDropped ? KH_REGION_AT_DROPPED : KH_REGION_AT_OK;
    }
  }
  id[k] = v;
  status[k] = code;
}

namespace
{
int64_t cells_of(const RegionJob & job) {return static_cast<int64_t>(job.f.width) * job.f.height;}
dim3 per_cell(const RegionJob & job) {return dim3(static_cast<unsigned>((cells_of(job) + 255) / 256));}
uint32_t watchdog(const RegionJob & job) {return static_cast<uint32_t>(cells_of(job)) + 1u;}
}  // namespace

void region_tiles(void * stream, const RegionJob & job)
{
  const RegionGrid g = region_grid(job.f.width, job.f.height);
  hipLaunchKernelGGL(k_region_tiles, dim3(static_cast<unsigned>(g.tiles_x), static_cast<unsigned>(g.tiles_y)), dim3(256), 0, static_cast<hipStream_t>(stream), job);
}

void region_seams(void * stream, const RegionJob & job)
{
  const RegionGrid g = region_grid(job.f.width, job.f.height);
  if (g.seam_threads == 0) {return;}
  const int64_t n_rows = static_cast<int64_t>(g.tiles_y - 1) * job.f.width;
  for (const RegionSet & s : job.set) {
    hipLaunchKernelGGL(k_region_seams, dim3(static_cast<unsigned>((g.seam_threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), s.label,
      job.f.width, job.f.height, job.conn8, n_rows, g.seam_threads, watchdog(job), job.counters);
  }
}

void region_flatten(void * stream, const RegionJob & job)
{
  for (const RegionSet & s : job.set) {
    hipLaunchKernelGGL(k_region_flatten, per_cell(job), dim3(256), 0, static_cast<hipStream_t>(stream), s.label, s.count, cells_of(job), watchdog(job),
      job.counters);
  }
}

void region_compact(void * stream, const RegionJob & job)
{
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n_units = region_grid(job.f.width, job.f.height).units;
  const dim3 blocks(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n_units + 3) / 4, 1024))));
  for (int32_t which = 0; which < 2; ++which) {
    hipLaunchKernelGGL(k_region_roots<false>, blocks, dim3(256), 0, s, job.set[which], which, cells_of(job), n_units, job.unit, job.counters);
    unit_scan(s, job.unit, n_units);
    hipLaunchKernelGGL(k_region_roots<true>, blocks, dim3(256), 0, s, job.set[which], which, cells_of(job), n_units, job.unit, job.counters);
    hipLaunchKernelGGL(k_region_ids, per_cell(job), dim3(256), 0, s, job.set[which], cells_of(job));
  }
}

void region_records(void * stream, const RegionJob & job)
{
  const int64_t threads = (cells_of(job) + kRecordCells - 1) / kRecordCells;
  hipLaunchKernelGGL(k_region_records, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), job, cells_of(job));
}

void region_anchors(void * stream, const RegionJob & job)
{
  const int64_t threads = (cells_of(job) + kRecordCells - 1) / kRecordCells;
  hipLaunchKernelGGL(k_region_anchor, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), job, cells_of(job));
}

void region_lookup(void * stream, const FieldWindow & f, const uint32_t * d_ids, int32_t n, const double * d_xy, uint32_t * d_id, int32_t * d_status)
{
  hipLaunchKernelGGL(k_region_lookup, dim3(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), f,
    d_ids, n, d_xy, d_id, d_status);
}
}  // namespace kh
