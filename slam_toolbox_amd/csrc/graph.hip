// Loop-closure candidate enumeration on the GPU: the part of
// karto::MapperGraph that feeds the batched scan matcher.
//
//   FindNearLinkedScans      Mapper.cpp:1795-1806 (BreadthFirstTraversal Mapper.cpp:1263-1297 with
//                            NearScanVisitor Mapper.cpp:1311-1333 over Vertex::GetAdjacentVertices Mapper.h:338-361)
//   FindPossibleLoopClosure  Mapper.cpp:1960-2010, all the chains successive calls return (TryCloseLoop's
//                            enumeration loop, Mapper.cpp:1500-1560), for a BATCH of query scans at once
//
// The reference walks all N scans per query on the CPU (distance test per scan) and runs a BFS with
// std::set / std::find membership tests; with matching at ~30 us per candidate that walk becomes the
// bottleneck.  Here the graph store (reference positions + CSR adjacency) is resident in HBM and one
// workgroup per query does: (1) the two distance tests for every scan -- the same IEEE operations as the
// reference (dx*dx + dy*dy, compiled without FMA contraction), so the flags are bit-exact; (2) the BFS
// restricted to "visitable" vertices, level-synchronous, frontier in global scratch; (3) the run
// segmentation that replaces the sequential chain state machine: a maximal run of (in range, not linked)
// scans is a chain iff it is terminated by an out-of-range scan and is long enough, or by the end of the
// list; a run terminated by a linked scan is discarded (chain.clear(), Mapper.cpp:1993-1996).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "graph_internal.hpp"
#include "host_common.hpp"

namespace kh
{
constexpr double kTol = 1e-06;      // KT_TOLERANCE, Math.h:41
constexpr uint8_t kInRange = 1;     // squaredDistance <  maxDistance^2 + KT_TOLERANCE   (Mapper.cpp:1988-1990)
constexpr uint8_t kVisitable = 2;   // squaredDistance <= maxDistance^2 - KT_TOLERANCE   (Mapper.cpp:1326-1327)
constexpr uint8_t kLinked = 4;      // member of FindNearLinkedScans' result
constexpr uint8_t kSeen = 8;

struct GraphDev
{
  int32_t n;
  const double * xy;
  const int32_t * adj_ptr;
  const int32_t * adj_idx;
};

// The gated squared distance: delta^T (I + s D)^-1 delta with s = chi2 / r^2 and D = [[dxx dxy], [dxy dyy]]
// the covariance of the displacement, so that `q < r^2` is the ellipse delta^T (r^2 I + chi2 D)^-1 delta < 1 -- the search disk
// widened by the chi2 ellipse.  Every operation is rounded on its own, on the device and on the host alike.  D = 0 or s = 0 gives
// a = c = det = 1, b = 0 and q = dx * dx + dy * dy to the bit; a row that is not a covariance (negative diagonal, det <= 0, NaN,
// infinity) or a quotient that is not finite falls back to that plain distance.
__host__ __device__ __forceinline__ double gated_dist_sq(double dx, double dy, double s, double dxx, double dxy, double dyy)
{
#pragma clang fp contract(off)
  const double a = 1.0 + s * dxx, c = 1.0 + s * dyy, b = s * dxy;
  const double det = a * c - b * b;
  const double num = (c * (dx * dx) - 2.0 * b * (dx * dy)) + a * (dy * dy);
  const double q = num / det;
  const bool plain = !(det > 0.0) || !(a >= 1.0) || !(c >= 1.0) || !__builtin_isfinite(q);
  return plain ? dx * dx + dy * dy : q;
}

// kGated: stage (1) tests gated_dist_sq instead of the plain squared distance; `gate` holds, per query, three planes of n doubles
// (dxx, dxy, dyy of every scan: lane i reads gate[.. + i], a wave 512 bytes in a row per plane).  Stages (2) and (3) are shared.
template <bool kGated>
__global__ __launch_bounds__(256) void k_loop_candidates(
  GraphDev g, const int32_t * __restrict__ queries, const int32_t * __restrict__ starts, double max_sq_plus, double max_sq_minus,
  int32_t min_chain, int32_t n_visit, uint8_t * flags_all, int32_t * frontier_all, int32_t * chain_count, int32_t * chains, int32_t cap_per_query,
  const double * __restrict__ gate, double gate_s)
{
  const int qi = blockIdx.x;
  const int q = queries[qi];
  // FindPossibleLoopClosure resumes at rStartNum with an EMPTY chain (Mapper.cpp:1966, 1976): scans before it neither
  // form chains nor extend one
  const int start = starts ? starts[qi] : 0;
  const int n = g.n;
  uint8_t * flags = flags_all + (size_t)qi * ((n + 3) & ~3);       // word-aligned rows: bits are set with 32-bit atomics
  int32_t * cur = frontier_all + (size_t)qi * 2 * n;
  int32_t * nxt = cur + n;
  __shared__ int32_t s_cur_n, s_nxt_n, s_out_n, s_stop;
  const double qx = g.xy[2 * q], qy = g.xy[2 * q + 1];
  // (1) distance flags
  const double * gxx = kGated ? gate + (size_t)qi * 3 * n : nullptr;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double dx = g.xy[2 * i] - qx, dy = g.xy[2 * i + 1] - qy;
    double d2;
    if constexpr (kGated) {
      d2 = gated_dist_sq(dx, dy, gate_s, gxx[i], gxx[(size_t)n + i], gxx[2 * (size_t)n + i]);
    } else {
      d2 = dx * dx + dy * dy;
    }
    uint8_t f = 0;
    if (d2 < max_sq_plus) {f |= kInRange;}
    if (d2 <= max_sq_minus) {f |= kVisitable;}
    flags[i] = f;
  }
  if (threadIdx.x == 0) {s_cur_n = 1; s_nxt_n = 0; s_out_n = 0; s_stop = n_visit; cur[0] = q;}
  __syncthreads();
  if (threadIdx.x == 0) {flags[q] |= kSeen;}
  __syncthreads();
  // (2) BFS over visitable vertices: a popped vertex is valid iff visitable, only valid ones expand
  while (s_cur_n > 0) {
    const int cn = s_cur_n;
    for (int t = threadIdx.x; t < cn; t += blockDim.x) {
      const int v = cur[t];
      if (!(flags[v] & kVisitable)) {continue;}
      atomicOr(reinterpret_cast<unsigned int *>(flags + (v & ~3)), (unsigned int)kLinked << (8 * (v & 3)));
      for (int k = g.adj_ptr[v]; k < g.adj_ptr[v + 1]; ++k) {
        const int w = g.adj_idx[k];
        const unsigned int bit = (unsigned int)kSeen << (8 * (w & 3));
        const unsigned int old = atomicOr(reinterpret_cast<unsigned int *>(flags + (w & ~3)), bit);
        if (!(old & bit)) {nxt[atomicAdd(&s_nxt_n, 1)] = w;}
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {s_cur_n = s_nxt_n; s_nxt_n = 0;}
    int32_t * tmp = cur; cur = nxt; nxt = tmp;
    __syncthreads();
  }
  // (3) chains = maximal runs of good scans with the right terminator
  int32_t * out = chains + (size_t)qi * cap_per_query * 2;
  // loop_match_minimum_chain_size 0: `chain.size() >= 0` (Mapper.cpp:2001) holds for the EMPTY chain too, so the reference returns at
  // the first out-of-range scan at or behind `start` with whatever it holds and does not advance; its next call returns the empty
  // chain from that same scan and TryCloseLoop stops (Mapper.cpp:1508).  The walk ends there: at most one chain per query.
  if (min_chain <= 0) {
    for (int i = min(start, n_visit) + threadIdx.x; i < n_visit; i += blockDim.x) {
      if (!(flags[i] & kInRange)) {atomicMin(&s_stop, i);}
    }
    __syncthreads();
  }
  const int stop = s_stop;
  // the walk ends at n_visit (the reference's loop bound is the scan MAP's size, which falls behind the largest id
  // once scans have been removed, Mapper.cpp:1974-1976): whatever chain is open there is returned
  for (int i = threadIdx.x; i < stop; i += blockDim.x) {
    const uint8_t f = flags[i];
    const bool good = i >= start && (f & kInRange) && !(f & kLinked);
    if (!good) {continue;}
    bool emit;
    int len_needed;
    if (i == n_visit - 1) {
      emit = true; len_needed = 1;                       // end of the list: whatever is left is returned
    } else {
      const uint8_t fn = flags[i + 1];
      const bool next_good = (fn & kInRange) && !(fn & kLinked);
      if (next_good) {continue;}                         // not the end of its run
      emit = !(fn & kInRange);                           // out of range: chain returned if long enough; linked: cleared
      len_needed = min_chain;
    }
    if (!emit) {continue;}
    int s = i;
    while (s > start) {
      const uint8_t fp = flags[s - 1];
      if ((fp & kInRange) && !(fp & kLinked)) {--s;} else {break;}
    }
    if (i - s + 1 >= len_needed) {
      const int slot = atomicAdd(&s_out_n, 1);
      if (slot < cap_per_query) {out[2 * slot] = s; out[2 * slot + 1] = i;}
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {chain_count[qi] = s_out_n;}
}

template <class T>
static int ensure(T *& p, size_t & cap, size_t need)
{
  if (need <= cap) {return KH_OK;}
  if (p) {(void)hipFree(p); p = nullptr;}
  const size_t n = std::max(need, cap + cap / 2);
  if (hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T)) != hipSuccess) {set_error("hipMalloc failed (graph store)"); cap = 0; return KH_ERR_HIP;}
  cap = n;
  return KH_OK;
}

// ---- nearest vertex / vertices within a radius of a pose --------------------------------------------------------------
// MapperGraph::FindNearByScan (Mapper.cpp:1877-1912) and FindNearByVertices (:1837-1875) build a nanoflann KD-tree over
// GetCorrectedPose() of every vertex (nanoflann_adaptors.h:44-49) on every call and ask it one question.  The store keeps
// those points in HBM; a pass over all of them is 16 bytes per vertex (800 KB at 50 000 vertices) and latency-bound, so
// there is no tree: one workgroup per query reads every point once.
//
// nanoflann's L2_Simple_Adaptor::evalMetric (nanoflann.hpp:475-485) sums (a - b)^2 per dimension: (dx * dx) + (dy * dy), each
// operation rounded on its own -- an FMA here would change the last bit and with it the order of near ties.
__device__ __forceinline__ double near_by_dist_sq(double qx, double qy, double2 p)
{
#pragma clang fp contract(off)
  const double dx = qx - p.x, dy = qy - p.y;
  const double xx = dx * dx, yy = dy * dy;
  return xx + yy;
}

// (distance, index) order of the library: the smaller distance, and the lower index between equal distances
__device__ __forceinline__ bool near_by_less(double da, int32_t ia, double db, int32_t ib) {return da < db || (da == db && ia < ib);}

// One workgroup of 256 per query: lane t looks at vertices t, t + 256, ... (one 16-byte load each, a wave reads 1 KB in a row),
// keeps its best (distance, index); the wave reduces over its 64 lanes with cross-lane shuffles, the four waves through LDS.
// nearest[q] = -1 and dist_sq[q] = +inf for an empty store.
__global__ __launch_bounds__(256) void k_near_by_scan(
  const double2 * __restrict__ pose, int32_t n, const double2 * __restrict__ queries, int32_t * __restrict__ nearest, double * __restrict__ dist_sq)
{
  const int qi = blockIdx.x;
  const double2 q = queries[qi];
  double best = HUGE_VAL;
  int32_t best_i = 0x7fffffff;
  // four loads in flight per lane (the pass is a chain of load latencies); an index past the end reads the last vertex and is not used
  for (int32_t base = threadIdx.x; base < n; base += 1024) {
    double2 p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {p[k] = pose[min(base + 256 * k, n - 1)];}
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t i = base + 256 * k;
      const double d = near_by_dist_sq(q.x, q.y, p[k]);
      if (i < n && (d < best || best_i == 0x7fffffff)) {best = d; best_i = i;}       // ascending i: the first of equal distances stays
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(best, off, 64);
    const int32_t oi = __shfl_xor(best_i, off, 64);
    if (near_by_less(od, oi, best, best_i)) {best = od; best_i = oi;}
  }
  __shared__ double s_d[4];
  __shared__ int32_t s_i[4];
  if ((threadIdx.x & 63) == 0) {s_d[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = best_i;}
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      if (near_by_less(s_d[w], s_i[w], best, best_i)) {best = s_d[w]; best_i = s_i[w];}
    }
    nearest[qi] = best_i == 0x7fffffff ? -1 : best_i;
    if (dist_sq) {dist_sq[qi] = best_i == 0x7fffffff ? HUGE_VAL : best;}
  }
}

// radiusSearch as FindNearByVertices calls it: every vertex with dist_sq < radius (see kh_graph_find_near_by_vertices), as a
// compacted list of (index, dist_sq) in no particular order -- the slot counter is a 32-bit integer atomic, one per wave that
// has a hit; the host sorts the few hits.  hit_idx / hit_d2 hold n entries, so every hit has a slot.
__global__ __launch_bounds__(256) void k_near_by_radius(
  const double2 * __restrict__ pose, int32_t n, double qx, double qy, double radius, int32_t * __restrict__ count,
  int32_t * __restrict__ hit_idx, double * __restrict__ hit_d2)
{
  for (int32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
    const int32_t i = base + threadIdx.x;
    double d = 0.0;
    bool hit = false;
    if (i < n) {d = near_by_dist_sq(qx, qy, pose[i]); hit = d < radius;}
    const unsigned long long votes = __ballot(hit);
    if (votes == 0) {continue;}
    const int lane = threadIdx.x & 63;
    int32_t first = 0;
    if (lane == 0) {first = atomicAdd(count, __popcll(votes));}
    first = __shfl(first, 0, 64);
    if (hit) {
      const int32_t slot = first + __popcll(votes & ((1ull << lane) - 1ull));
      if (slot < n) {hit_idx[slot] = i; hit_d2[slot] = d;}
    }
  }
}

// ---- relocalization candidates: where in the map to try a scan that comes without a pose -------------
// Seeds: a lattice of side `spacing` over the plane; the cell of a vertex is (floor(x / spacing), floor(y / spacing)), an FP64 divide
// and floor (a negative coordinate goes down, -0.0 and +0.0 compare equal as cells); the seed of a cell is its vertex with the LOWEST
// list index.  Base of a seed: every vertex j with (dx * dx) + (dy * dy) < R * R + KT_TOLERANCE from it, in list order, every s-th one
// when there are more than max_base.  Positions are the store's poses (GetCorrectedPose() x, y), as for the near-by queries.
__device__ __forceinline__ double2 seed_cell(double2 p, double spacing) {return make_double2(floor(p.x / spacing), floor(p.y / spacing));}

// flag[i] = 1 iff no vertex j < i lies in vertex i's cell, and vertex i passes the region test (use_region: dist_sq to the centre <
// region_sq_plus = radius^2 + KT_TOLERANCE); a cell's seed that fails the region test is dropped, no other vertex takes its place.
// One thread per vertex; the cells of the vertices before it pass through LDS in tiles of 256 (block b reads tiles 0 .. b), so the
// answer is a pure function of the list: the lowest index wins whatever order the blocks run in.
__global__ __launch_bounds__(256) void k_seed_cover(
  const double2 * __restrict__ pose, int32_t n, double spacing, int32_t use_region, double cx, double cy, double region_sq_plus,
  int32_t * __restrict__ flag)
{
  __shared__ double2 s_cell[256];
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  const double2 p = pose[min(i, n - 1)];
  const double2 mine = seed_cell(p, spacing);
  bool first = true;
  for (int32_t tile = 0; tile <= static_cast<int32_t>(blockIdx.x); ++tile) {
    const int32_t j0 = tile * 256;
    s_cell[threadIdx.x] = seed_cell(pose[min(j0 + static_cast<int32_t>(threadIdx.x), n - 1)], spacing);
    __syncthreads();
    const int32_t count = min(256, i - j0);                 // only vertices before i (<= 0 in the block's own tile for its first thread)
    for (int32_t k = 0; k < count; ++k) {
      const double2 c = s_cell[k];
      if (c.x == mine.x && c.y == mine.y) {first = false;}
    }
    __syncthreads();
  }
  if (i < n) {
    bool keep = first;
    if (use_region) {keep = keep && near_by_dist_sq(cx, cy, p) < region_sq_plus;}
    flag[i] = keep ? 1 : 0;
  }
}

// exclusive prefix sum of value[0 .. n) by ONE workgroup of 256, in list order: begin[i] = value[0] + ... + value[i - 1], begin[n] =
// the total (begin may be NULL); with `list`, the indices i whose value is not zero are written to list[begin[i]] -- the seeds in
// ascending list index out of k_seed_cover's flags.  Per 256 values: an inclusive scan over the wave's 64 lanes with shuffles, the four
// wave totals through LDS.  No atomics: the order is the list's.
__global__ __launch_bounds__(256) void k_prefix_list(const int32_t * __restrict__ value, int32_t n, int32_t * __restrict__ begin, int32_t * __restrict__ list)
{
  __shared__ int32_t s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t running = 0;
  for (int32_t base = 0; base < n; base += 256) {
    const int32_t i = base + threadIdx.x;
    const int32_t v = i < n ? value[i] : 0;
    int32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
      const int32_t up = __shfl_up(incl, off, 64);
      if (lane >= off) {incl += up;}
    }
    if (lane == 63) {s_wave[wave] = incl;}
    __syncthreads();
    int32_t before = running;
    for (int w = 0; w < wave; ++w) {before += s_wave[w];}
    const int32_t excl = before + incl - v;
    if (i < n) {
      if (begin) {begin[i] = excl;}
      if (list && v != 0) {list[excl] = i;}
    }
    running += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (begin && threadIdx.x == 0) {begin[n] = running;}
}

// how many entries of an ordered list of c are kept, and the stride between them: all of them up to max_base, otherwise entries
// 0, s, 2s, ... with s = ceil(c / max_base)
__device__ __forceinline__ int32_t base_stride(int32_t c, int32_t max_base) {return c <= max_base ? 1 : (c + max_base - 1) / max_base;}

// One wave per seed (four seeds per workgroup) over all n vertices, 64 at a time: lane t tests vertex base + t, the wave's ballot
// gives every hit its rank in list order.  fill = 0: raw[k] = the number of vertices in range, kept[k] = how many of them the stride
// rule keeps.  fill = 1 (after k_prefix_list has turned kept into base_begin): the hit of rank r with r % s == 0 goes to
// base_idx[base_begin[k] + r / s].  Two passes instead of an atomically appended list: the order is the list's.
__global__ __launch_bounds__(256) void k_base_gather(
  const double2 * __restrict__ pose, int32_t n, const int32_t * __restrict__ seeds, int32_t n_seeds, double range_sq_plus, int32_t max_base,
  int32_t fill, int32_t * __restrict__ raw, int32_t * __restrict__ kept, const int32_t * __restrict__ base_begin, int32_t * __restrict__ base_idx)
{
  const int lane = threadIdx.x & 63;
  const int32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_seeds) {return;}                              // (the whole wave leaves: no barrier in this kernel)
  const int32_t seed = seeds[k];
  if (seed < 0 || seed >= n) {return;}
  const double2 q = pose[seed];
  int32_t stride = 1, first = 0, room = 0;
  if (fill) {
    stride = base_stride(raw[k], max_base);
    first = base_begin[k];
    room = base_begin[k + 1] - first;
  }
  int32_t count = 0;
  for (int32_t base = 0; base < n; base += 64) {
    const int32_t i = base + lane;
    const bool hit = i < n && near_by_dist_sq(q.x, q.y, pose[min(i, n - 1)]) < range_sq_plus;
    const unsigned long long votes = __ballot(hit);
    if (fill && hit) {
      const int32_t rank = count + __popcll(votes & ((1ull << lane) - 1ull));
      const int32_t slot = rank / stride;
      if (rank % stride == 0 && slot < room) {base_idx[first + slot] = i;}
    }
    count += __popcll(votes);
  }
  if (!fill && lane == 0) {
    raw[k] = count;
    const int32_t s = base_stride(count, max_base);
    kept[k] = (count + s - 1) / s;
  }
}

}  // namespace kh

using namespace kh;

struct kh_graph
{
  int32_t device = 0;
  hipStream_t stream = nullptr;
  int32_t n = 0;
  bool device_stale = false;   // the host copy is newer than the device arrays (uploaded by the next enumeration kernel)
  int32_t n_visit = 0;     // scans the candidate walks visit (kh_graph_set_scan_limit; = n unless scans were removed)
  double * d_xy = nullptr; size_t cap_xy = 0;
  int32_t * d_adj_ptr = nullptr; size_t cap_ptr = 0;
  int32_t * d_adj_idx = nullptr; size_t cap_idx = 0;
  int32_t * d_queries = nullptr; size_t cap_q = 0;
  uint8_t * d_flags = nullptr; size_t cap_flags = 0;
  int32_t * d_frontier = nullptr; size_t cap_frontier = 0;
  int32_t * d_count = nullptr; size_t cap_count = 0;
  int32_t * d_chains = nullptr; size_t cap_chains = 0;
  double * d_gate = nullptr; size_t cap_gate = 0;      // kh_graph_find_loop_candidates_gated: per query the planes dxx | dxy | dyy (3n)
  std::vector<double> h_gate;                          // ... as packed for the upload
  double last_ms = 0.0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  // host copy of the store: the neighbourhood walks of FindNearChains touch tens of vertices (no kernel)
  std::vector<double> h_xy;
  std::vector<int32_t> h_adj_ptr, h_adj_idx;
  // the second per-vertex point: GetCorrectedPose() x, y, what the near-by queries measure to (ref_xy is the pose or the barycentre).
  // Host copy + device copy with a stale flag of its own: a near-by query uploads 16 bytes per vertex, not the adjacency.
  std::vector<double> h_pose;
  bool has_poses = true;        // every vertex of the store has its pose (an empty store has; kh_graph_set / the pose-less append clear it)
  bool pose_stale = false;
  double * d_pose = nullptr; size_t cap_pose = 0;
  double * d_nb_query = nullptr; size_t cap_nb_query = 0;      // queries (2q), behind them dist_sq (q)
  int32_t * d_nb_idx = nullptr; size_t cap_nb_idx = 0;         // nearest (q) / radius hits (n) + their count (1)
  double * d_nb_d2 = nullptr; size_t cap_nb_d2 = 0;            // dist_sq of the radius hits (n)
  double last_near_by_ms = 0.0;
  // relocalization candidates (k_seed_cover / k_prefix_list / k_base_gather): seed flags (n), their prefix (n + 1), seeds (n); per seed
  // the raw and the kept base count (2s), base_begin (s + 1); base_idx (its total)
  int32_t * d_rl_flag = nullptr; size_t cap_rl_flag = 0;
  int32_t * d_rl_prefix = nullptr; size_t cap_rl_prefix = 0;
  int32_t * d_rl_seeds = nullptr; size_t cap_rl_seeds = 0;
  int32_t * d_rl_count = nullptr; size_t cap_rl_count = 0;
  int32_t * d_rl_begin = nullptr; size_t cap_rl_begin = 0;
  int32_t * d_rl_idx = nullptr; size_t cap_rl_idx = 0;
  double last_relocalize_ms = 0.0;
};

extern "C" {

int kh_graph_create(int32_t device, kh_graph ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    set_error("no usable HIP device (libkartohip has no CPU fallback)");
    return KH_ERR_NO_DEVICE;
  }
  kh_graph * g = new kh_graph();
  g->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
    hipEventCreate(&g->ev[0]) != hipSuccess || hipEventCreate(&g->ev[1]) != hipSuccess)
  {
    set_error("HIP stream/event creation failed");
    delete g;
    return KH_ERR_HIP;
  }
  *out = g;
  return KH_OK;
}

void kh_graph_destroy(kh_graph * g)
{
  if (!g) {return;}
  (void)hipSetDevice(g->device);
  if (g->stream) {(void)hipStreamSynchronize(g->stream);}
  (void)hipFree(g->d_xy); (void)hipFree(g->d_adj_ptr); (void)hipFree(g->d_adj_idx); (void)hipFree(g->d_queries);
  (void)hipFree(g->d_flags); (void)hipFree(g->d_frontier); (void)hipFree(g->d_count); (void)hipFree(g->d_chains);
  (void)hipFree(g->d_pose); (void)hipFree(g->d_nb_query); (void)hipFree(g->d_nb_idx); (void)hipFree(g->d_nb_d2);
  (void)hipFree(g->d_rl_flag); (void)hipFree(g->d_rl_prefix); (void)hipFree(g->d_rl_seeds); (void)hipFree(g->d_rl_count);
  (void)hipFree(g->d_rl_begin); (void)hipFree(g->d_rl_idx); (void)hipFree(g->d_gate);
  if (g->ev[0]) {(void)hipEventDestroy(g->ev[0]);}
  if (g->ev[1]) {(void)hipEventDestroy(g->ev[1]);}
  if (g->stream) {(void)hipStreamDestroy(g->stream);}
  delete g;
}

int kh_graph_set(kh_graph * g, int32_t n_scans, const double * ref_xy, const int32_t * adj_ptr, const int32_t * adj_idx)
{
  if (!g || n_scans < 0 || (n_scans > 0 && (!ref_xy || !adj_ptr))) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t n = static_cast<size_t>(n_scans);
  const size_t n_adj = n ? static_cast<size_t>(adj_ptr[n]) : 0;
  if (n_adj > 0 && !adj_idx) {return KH_ERR_INVALID_ARG;}
  for (size_t k = 0; k < n_adj; ++k) {
    if (adj_idx[k] < 0 || adj_idx[k] >= n_scans) {set_error("kh_graph_set: adjacency index out of range"); return KH_ERR_INVALID_ARG;}
  }
  // the neighbourhood walks (near chains, near linked) read the host copy; the device arrays are refreshed when an
  // enumeration kernel next needs them (a mapper sets the graph several times per scan and enumerates once)
  g->device_stale = true;
  g->n = n_scans; g->n_visit = n_scans;
  g->h_xy.assign(ref_xy, ref_xy + 2 * n);
  g->h_adj_ptr.assign(adj_ptr, adj_ptr + (n ? n + 1 : 0));
  g->h_adj_idx.assign(adj_idx, adj_idx + n_adj);
  g->h_pose.clear(); g->has_poses = n_scans == 0; g->pose_stale = true;      // kh_graph_set_poses follows for the near-by queries
  return KH_OK;
}

}  // extern "C"
namespace kh
{
// (library-internal, the mapper's sync_graph) kh_graph_set without the copies: the store takes the caller's arrays and hands its old
// ones back (same capacity next time); the caller built adj_idx from its own tables, so the range check is skipped.  A lifelong mapper
// rebuilds the store after every node removal -- once per accepted scan, 18 000 scans alive in the 50 000-scan replay.
int graph_swap(kh_graph * g, int32_t n_scans, std::vector<double> & ref_xy, std::vector<int32_t> & adj_ptr, std::vector<int32_t> & adj_idx,
  std::vector<double> & pose_xy)
{
  if (!g || n_scans < 0 || ref_xy.size() != 2 * static_cast<size_t>(n_scans) || adj_ptr.size() != static_cast<size_t>(n_scans) + 1 ||
    pose_xy.size() != ref_xy.size()) {return KH_ERR_INVALID_ARG;}
  g->device_stale = true;
  g->n = n_scans; g->n_visit = n_scans;
  g->h_xy.swap(ref_xy); g->h_adj_ptr.swap(adj_ptr); g->h_adj_idx.swap(adj_idx);
  g->h_pose.swap(pose_xy); g->has_poses = true; g->pose_stale = true;
  return KH_OK;
}
}  // namespace kh
extern "C" {

int kh_graph_append_scan(kh_graph * g, const double ref_xy[2])
{
  if (!g || !ref_xy) {return KH_ERR_INVALID_ARG;}
  if (g->h_adj_ptr.empty()) {g->h_adj_ptr.push_back(0);}
  g->h_xy.push_back(ref_xy[0]); g->h_xy.push_back(ref_xy[1]);
  g->h_adj_ptr.push_back(g->h_adj_ptr.back());
  if (g->n_visit == g->n) {++g->n_visit;}
  ++g->n;
  g->device_stale = true;
  g->has_poses = false;                  // this vertex has no pose: kh_graph_append_scan_with_pose is the form that keeps the near-by queries
  return KH_OK;
}

int kh_graph_append_scan_with_pose(kh_graph * g, const double ref_xy[2], const double pose_xy[2])
{
  if (!g || !ref_xy || !pose_xy) {return KH_ERR_INVALID_ARG;}
  const bool had_poses = g->has_poses;
  const int rc = kh_graph_append_scan(g, ref_xy);
  if (rc) {return rc;}
  if (had_poses) {
    g->h_pose.push_back(pose_xy[0]); g->h_pose.push_back(pose_xy[1]);
    g->has_poses = true; g->pose_stale = true;
  }
  return KH_OK;
}

int kh_graph_set_poses(kh_graph * g, int32_t n_scans, const double * pose_xy)
{
  if (!g || n_scans != g->n || (n_scans > 0 && !pose_xy)) {return KH_ERR_INVALID_ARG;}
  g->h_pose.assign(pose_xy, pose_xy + 2 * static_cast<size_t>(n_scans));
  g->has_poses = true; g->pose_stale = true;
  return KH_OK;
}

int kh_graph_set_pose(kh_graph * g, int32_t scan, const double pose_xy[2])
{
  if (!g || !pose_xy || scan < 0 || scan >= g->n || !g->has_poses) {return KH_ERR_INVALID_ARG;}
  g->h_pose[2 * static_cast<size_t>(scan)] = pose_xy[0]; g->h_pose[2 * static_cast<size_t>(scan) + 1] = pose_xy[1];
  g->pose_stale = true;
  return KH_OK;
}

int kh_graph_add_edge(kh_graph * g, int32_t scan_a, int32_t scan_b)
{
  if (!g || scan_a < 0 || scan_b < 0 || scan_a >= g->n || scan_b >= g->n || scan_a == scan_b) {return KH_ERR_INVALID_ARG;}
  auto append = [&](int32_t at, int32_t what) {
    g->h_adj_idx.insert(g->h_adj_idx.begin() + g->h_adj_ptr[static_cast<size_t>(at) + 1], what);
    for (size_t k = static_cast<size_t>(at) + 1; k < g->h_adj_ptr.size(); ++k) {++g->h_adj_ptr[k];}
  };
  append(scan_a, scan_b);
  append(scan_b, scan_a);
  g->device_stale = true;
  return KH_OK;
}

int kh_graph_set_position(kh_graph * g, int32_t scan, const double ref_xy[2])
{
  if (!g || !ref_xy || scan < 0 || scan >= g->n) {return KH_ERR_INVALID_ARG;}
  g->h_xy[2 * static_cast<size_t>(scan)] = ref_xy[0]; g->h_xy[2 * static_cast<size_t>(scan) + 1] = ref_xy[1];
  g->device_stale = true;
  return KH_OK;
}

int kh_graph_set_positions(kh_graph * g, int32_t n_scans, const double * ref_xy)
{
  if (!g || !ref_xy || n_scans != g->n) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  g->h_xy.assign(ref_xy, ref_xy + 2 * static_cast<size_t>(n_scans));
  g->device_stale = true;
  return KH_OK;
}

int kh_graph_find_loop_candidates(
  kh_graph * g, int32_t n_queries, const int32_t * query_scans, double max_distance, int32_t min_chain_size,
  int32_t * chain_begin, int32_t * chains, int32_t cap_chains, int32_t * n_chains)
{
  return kh_graph_find_loop_candidates_from(g, n_queries, query_scans, nullptr, max_distance, min_chain_size, chain_begin, chains,
           cap_chains, n_chains);
}

}  // extern "C"
// One query, answered from the host copy of the store: the same three steps as k_loop_candidates -- the same IEEE
// operations for the two distance tests, the breadth-first marking of the linked scans, the run rule per scan -- in ~20 us
// for an 18 000-scan store, where the device round trip (upload of the edited store, launch, two downloads, a stream drain)
// is ~150 us.  A mapper asks exactly one such question per processed scan; batches of queries go to the kernel.
// kGated: gate = the query's row as the caller gave it (9 doubles per scan), gate_s = chi2 / r^2 (see gated_dist_sq)
template <bool kGated>
static void loop_candidates_host(const kh_graph * g, int32_t q, int32_t start, double max_sq_plus, double max_sq_minus, int32_t min_chain,
                                 std::vector<std::pair<int32_t, int32_t>> & out, const double * gate = nullptr, double gate_s = 0.0)
{
  const int32_t n = g->n, n_visit = g->n_visit;
  static thread_local std::vector<uint8_t> flags;
  static thread_local std::vector<int32_t> cur, nxt;
  flags.assign(static_cast<size_t>(n), 0);
  const double * xy = g->h_xy.data();
  const double qx = xy[2 * q], qy = xy[2 * q + 1];
  for (int32_t i = 0; i < n; ++i) {
    const double dx = xy[2 * i] - qx, dy = xy[2 * i + 1] - qy;
    double d2;
    if constexpr (kGated) {
      const double * row = gate + 9 * static_cast<size_t>(i);
      d2 = gated_dist_sq(dx, dy, gate_s, row[0], row[1], row[4]);
    } else {
      d2 = dx * dx + dy * dy;
    }
    uint8_t f = 0;
    if (d2 < max_sq_plus) {f |= kInRange;}
    if (d2 <= max_sq_minus) {f |= kVisitable;}
    flags[i] = f;
  }
  cur.assign(1, q); nxt.clear();
  flags[q] |= kSeen;
  while (!cur.empty()) {
    for (int32_t v : cur) {
      if (!(flags[v] & kVisitable)) {continue;}
      flags[v] |= kLinked;
      for (int32_t k = g->h_adj_ptr[v]; k < g->h_adj_ptr[v + 1]; ++k) {
        const int32_t w = g->h_adj_idx[k];
        if (!(flags[w] & kSeen)) {flags[w] |= kSeen; nxt.push_back(w);}
      }
    }
    cur.swap(nxt);
    nxt.clear();
  }
  out.clear();
  auto good_at = [&](int32_t i) {return (flags[i] & kInRange) && !(flags[i] & kLinked);};
  for (int32_t i = std::max(start, 0); i < n_visit; ++i) {
    if (min_chain <= 0 && !(flags[i] & kInRange)) {break;}     // minimum chain size 0: the walk ends at the first out-of-range scan (see k_loop_candidates)
    if (!good_at(i)) {continue;}
    bool emit;
    int32_t len_needed;
    if (i == n_visit - 1) {
      emit = true; len_needed = 1;                       // end of the list: whatever is left is returned
    } else {
      if (good_at(i + 1)) {continue;}                    // not the end of its run
      emit = !(flags[i + 1] & kInRange);                 // out of range: chain returned if long enough; linked: cleared
      len_needed = min_chain;
    }
    if (!emit) {continue;}
    int32_t s0 = i;
    while (s0 > start && good_at(s0 - 1)) {--s0;}
    if (i - s0 + 1 >= len_needed) {out.push_back({s0, i});}
  }
}

// kh_graph_find_loop_candidates_from (gate = NULL) and kh_graph_find_loop_candidates_gated (gate = n_queries rows of 9 n_scans doubles)
static int find_loop_candidates(
  kh_graph * g, int32_t n_queries, const int32_t * query_scans, const int32_t * start_scans, double max_distance,
  int32_t min_chain_size, const double * gate, double chi2, int32_t * chain_begin, int32_t * chains, int32_t cap_chains, int32_t * n_chains)
{
  if (!g || n_queries < 0 || !chain_begin || !n_chains || (n_queries > 0 && !query_scans) || cap_chains < 0 || (cap_chains > 0 && !chains)) {
    return KH_ERR_INVALID_ARG;
  }
  *n_chains = 0;
  chain_begin[0] = 0;
  if (n_queries == 0) {return KH_OK;}
  if (g->n <= 0) {set_error("kh_graph_find_loop_candidates: empty graph"); return KH_ERR_NOT_FOUND;}
  for (int32_t i = 0; i < n_queries; ++i) {
    if (query_scans[i] < 0 || query_scans[i] >= g->n) {set_error("kh_graph_find_loop_candidates: unknown scan"); return KH_ERR_NOT_FOUND;}
  }
  if (n_queries == 1) {
    if (start_scans && start_scans[0] < 0) {set_error("kh_graph_find_loop_candidates_from: negative start"); return KH_ERR_INVALID_ARG;}
    const double sq1 = max_distance * max_distance;
    std::vector<std::pair<int32_t, int32_t>> v;
    if (gate) {
      loop_candidates_host<true>(g, query_scans[0], start_scans ? start_scans[0] : 0, sq1 + kTol, sq1 - kTol, min_chain_size, v, gate, chi2 / sq1);
    } else {
      loop_candidates_host<false>(g, query_scans[0], start_scans ? start_scans[0] : 0, sq1 + kTol, sq1 - kTol, min_chain_size, v);
    }
    int32_t total1 = 0;
    for (const auto & ch : v) {                            // already in scan order
      if (total1 < cap_chains) {chains[2 * total1] = ch.first; chains[2 * total1 + 1] = ch.second;}
      ++total1;
    }
    chain_begin[1] = total1;
    *n_chains = total1;
    g->last_ms = 0.0;
    return KH_OK;
  }
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  if (g->device_stale) {
    const size_t ns = static_cast<size_t>(g->n), n_adj = g->h_adj_idx.size();
    int urc = ensure(g->d_xy, g->cap_xy, std::max<size_t>(2 * ns, 2)); if (urc) {return urc;}
    urc = ensure(g->d_adj_ptr, g->cap_ptr, ns + 1); if (urc) {return urc;}
    urc = ensure(g->d_adj_idx, g->cap_idx, std::max<size_t>(n_adj, 1)); if (urc) {return urc;}
    if (hipMemcpyAsync(g->d_xy, g->h_xy.data(), 2 * ns * sizeof(double), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(g->d_adj_ptr, g->h_adj_ptr.data(), (ns + 1) * sizeof(int32_t), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      (n_adj && hipMemcpyAsync(g->d_adj_idx, g->h_adj_idx.data(), n_adj * sizeof(int32_t), hipMemcpyHostToDevice, g->stream) != hipSuccess) ||
      hipStreamSynchronize(g->stream) != hipSuccess)
    {
      set_error("kh_graph: upload failed");
      return KH_ERR_HIP;
    }
    g->device_stale = false;
  }
  const size_t nq = static_cast<size_t>(n_queries), n = static_cast<size_t>(g->n);
  // a run needs at least one terminator, so a query has at most n / 2 + 1 chains; min_chain bounds it further
  const int32_t per_query = static_cast<int32_t>(std::min<size_t>(n / std::max(1, min_chain_size + 1) + 2, n / 2 + 1));
  int rc = ensure(g->d_queries, g->cap_q, 2 * nq); if (rc) {return rc;}
  rc = ensure(g->d_flags, g->cap_flags, nq * ((n + 3) & ~static_cast<size_t>(3)) + 4); if (rc) {return rc;}
  rc = ensure(g->d_frontier, g->cap_frontier, nq * 2 * n); if (rc) {return rc;}
  rc = ensure(g->d_count, g->cap_count, nq); if (rc) {return rc;}
  rc = ensure(g->d_chains, g->cap_chains, nq * per_query * 2); if (rc) {return rc;}
  if (hipMemcpyAsync(g->d_queries, query_scans, nq * sizeof(int32_t), hipMemcpyHostToDevice, g->stream) != hipSuccess) {return KH_ERR_HIP;}
  if (start_scans) {
    for (size_t i = 0; i < nq; ++i) {if (start_scans[i] < 0) {set_error("kh_graph_find_loop_candidates_from: negative start"); return KH_ERR_INVALID_ARG;}}
    if (hipMemcpyAsync(g->d_queries + nq, start_scans, nq * sizeof(int32_t), hipMemcpyHostToDevice, g->stream) != hipSuccess) {return KH_ERR_HIP;}
  }
  // Mapper.cpp:1988-1990 and 1326-1327: Square(maxDistance) +/- KT_TOLERANCE
  const double sq = max_distance * max_distance;
  if (gate) {
    // the three doubles of a row the test reads, as planes of n per query (dxx | dxy | dyy): a third of the bytes goes up, and lane i
    // of the kernel reads plane[i] -- consecutive lanes, consecutive addresses -- instead of three loads at a stride of 72 bytes
    g->h_gate.resize(3 * nq * n);
    for (size_t qi = 0; qi < nq; ++qi) {
      const double * row = gate + 9 * n * qi;
      double * plane = g->h_gate.data() + 3 * n * qi;
      for (size_t i = 0; i < n; ++i) {plane[i] = row[9 * i]; plane[n + i] = row[9 * i + 1]; plane[2 * n + i] = row[9 * i + 4];}
    }
    rc = ensure(g->d_gate, g->cap_gate, 3 * nq * n); if (rc) {return rc;}
    if (hipMemcpyAsync(g->d_gate, g->h_gate.data(), 3 * nq * n * sizeof(double), hipMemcpyHostToDevice, g->stream) != hipSuccess) {return KH_ERR_HIP;}
  }
  GraphDev dev{g->n, g->d_xy, g->d_adj_ptr, g->d_adj_idx};
  (void)hipEventRecord(g->ev[0], g->stream);
  if (gate) {
    hipLaunchKernelGGL(k_loop_candidates<true>, dim3(static_cast<unsigned>(nq)), dim3(256), 0, g->stream, dev, g->d_queries,
      start_scans ? g->d_queries + nq : nullptr, sq + kTol, sq - kTol, min_chain_size, g->n_visit, g->d_flags, g->d_frontier, g->d_count, g->d_chains, per_query,
      g->d_gate, chi2 / sq);
  } else {
    hipLaunchKernelGGL(k_loop_candidates<false>, dim3(static_cast<unsigned>(nq)), dim3(256), 0, g->stream, dev, g->d_queries,
      start_scans ? g->d_queries + nq : nullptr, sq + kTol, sq - kTol, min_chain_size, g->n_visit, g->d_flags, g->d_frontier, g->d_count, g->d_chains, per_query,
      nullptr, 0.0);
  }
  (void)hipEventRecord(g->ev[1], g->stream);
  std::vector<int32_t> counts(nq), all(nq * per_query * 2);
  if (hipMemcpyAsync(counts.data(), g->d_count, nq * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipMemcpyAsync(all.data(), g->d_chains, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipStreamSynchronize(g->stream) != hipSuccess)
  {
    set_error(std::string("kh_graph_find_loop_candidates: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
  g->last_ms = ms;
  int32_t total = 0;
  for (size_t qi = 0; qi < nq; ++qi) {
    const int32_t c = std::min(counts[qi], per_query);
    std::vector<std::pair<int32_t, int32_t>> v(c);
    for (int32_t k = 0; k < c; ++k) {v[k] = {all[(qi * per_query + k) * 2], all[(qi * per_query + k) * 2 + 1]};}
    std::sort(v.begin(), v.end());                       // the reference returns them in scan order
    for (const auto & ch : v) {
      if (total < cap_chains) {chains[2 * total] = ch.first; chains[2 * total + 1] = ch.second;}
      ++total;
    }
    chain_begin[qi + 1] = total;
  }
  *n_chains = total;
  return KH_OK;
}
extern "C" {

int kh_graph_find_loop_candidates_from(
  kh_graph * g, int32_t n_queries, const int32_t * query_scans, const int32_t * start_scans, double max_distance,
  int32_t min_chain_size, int32_t * chain_begin, int32_t * chains, int32_t cap_chains, int32_t * n_chains)
{
  return find_loop_candidates(g, n_queries, query_scans, start_scans, max_distance, min_chain_size, nullptr, 0.0, chain_begin, chains, cap_chains,
           n_chains);
}

int kh_graph_find_loop_candidates_gated(
  kh_graph * g, int32_t n_queries, const int32_t * query_scans, const int32_t * start_scans, double max_distance,
  int32_t min_chain_size, double chi2, const double * gate, int32_t * chain_begin, int32_t * chains, int32_t cap_chains, int32_t * n_chains)
{
  if (!gate || !(chi2 >= 0.0)) {return KH_ERR_INVALID_ARG;}          // (chi2 = NaN fails the comparison)
  return find_loop_candidates(g, n_queries, query_scans, start_scans, max_distance, min_chain_size, gate, chi2, chain_begin, chains, cap_chains,
           n_chains);
}

double kh_graph_last_kernel_ms(kh_graph * g) {return g ? g->last_ms : 0.0;}

// ---- near-by queries (k_near_by_scan / k_near_by_radius) -----------------------------------------------------------------
namespace
{
int near_by_ready(kh_graph * g, const char * who)
{
  if (!g->has_poses) {set_error(std::string(who) + ": the store has no poses (kh_graph_set_poses)"); return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  if (g->pose_stale && g->n > 0) {
    const size_t ns = static_cast<size_t>(g->n);
    const int rc = ensure(g->d_pose, g->cap_pose, 2 * ns); if (rc) {return rc;}
    if (hipMemcpyAsync(g->d_pose, g->h_pose.data(), 2 * ns * sizeof(double), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess)
    {
      set_error(std::string(who) + ": upload failed");
      return KH_ERR_HIP;
    }
  }
  g->pose_stale = false;
  return KH_OK;
}
}  // namespace

int kh_graph_find_near_by_scan(kh_graph * g, int32_t n_queries, const double * query_xy, int32_t * nearest, double * dist_sq)
{
  if (!g || n_queries < 0 || (n_queries > 0 && (!query_xy || !nearest))) {return KH_ERR_INVALID_ARG;}
  if (n_queries == 0) {return KH_OK;}
  const size_t nq = static_cast<size_t>(n_queries);
  if (g->n == 0) {                                      // FindNearByScan returns NULL (Mapper.cpp:1907-1911)
    for (size_t i = 0; i < nq; ++i) {nearest[i] = -1; if (dist_sq) {dist_sq[i] = HUGE_VAL;}}
    return KH_OK;
  }
  int rc = near_by_ready(g, "kh_graph_find_near_by_scan"); if (rc) {return rc;}
  rc = ensure(g->d_nb_query, g->cap_nb_query, 3 * nq); if (rc) {return rc;}
  rc = ensure(g->d_nb_idx, g->cap_nb_idx, nq); if (rc) {return rc;}
  double * d_d2 = g->d_nb_query + 2 * nq;
  if (hipMemcpyAsync(g->d_nb_query, query_xy, 2 * nq * sizeof(double), hipMemcpyHostToDevice, g->stream) != hipSuccess) {return KH_ERR_HIP;}
  (void)hipEventRecord(g->ev[0], g->stream);
  hipLaunchKernelGGL(k_near_by_scan, dim3(static_cast<unsigned>(nq)), dim3(256), 0, g->stream, reinterpret_cast<const double2 *>(g->d_pose),
    g->n, reinterpret_cast<const double2 *>(g->d_nb_query), g->d_nb_idx, d_d2);
  (void)hipEventRecord(g->ev[1], g->stream);
  if (hipMemcpyAsync(nearest, g->d_nb_idx, nq * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    (dist_sq && hipMemcpyAsync(dist_sq, d_d2, nq * sizeof(double), hipMemcpyDeviceToHost, g->stream) != hipSuccess) ||
    hipStreamSynchronize(g->stream) != hipSuccess)
  {
    set_error(std::string("kh_graph_find_near_by_scan: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
  g->last_near_by_ms = ms;
  return KH_OK;
}

int kh_graph_find_near_by_vertices(kh_graph * g, const double query_xy[2], double max_distance, int32_t * scans, int32_t cap, int32_t * n_found)
{
  if (!g || !query_xy || !n_found || cap < 0 || (cap > 0 && !scans)) {return KH_ERR_INVALID_ARG;}
  *n_found = 0;
  if (g->n == 0) {return KH_OK;}
  int rc = near_by_ready(g, "kh_graph_find_near_by_vertices"); if (rc) {return rc;}
  const size_t n = static_cast<size_t>(g->n);
  rc = ensure(g->d_nb_idx, g->cap_nb_idx, n + 1); if (rc) {return rc;}
  rc = ensure(g->d_nb_d2, g->cap_nb_d2, n); if (rc) {return rc;}
  int32_t * d_count = g->d_nb_idx + n;
  if (hipMemsetAsync(d_count, 0, sizeof(int32_t), g->stream) != hipSuccess) {return KH_ERR_HIP;}
  // FindNearByVertices hands maxDistance to radiusSearch (Mapper.cpp:1865) as the search RADIUS of an L2 metric, whose result set
  // keeps a point when `dist < radius` (nanoflann.hpp:274) with dist the SQUARED distance of L2_Simple_Adaptor: the reference
  // compares the squared distance with the unsquared maxDistance, strictly, and so does this
  const unsigned blocks = static_cast<unsigned>(std::min<size_t>((n + 255) / 256, 256));
  (void)hipEventRecord(g->ev[0], g->stream);
  hipLaunchKernelGGL(k_near_by_radius, dim3(blocks), dim3(256), 0, g->stream, reinterpret_cast<const double2 *>(g->d_pose), g->n,
    query_xy[0], query_xy[1], max_distance, d_count, g->d_nb_idx, g->d_nb_d2);
  (void)hipEventRecord(g->ev[1], g->stream);
  int32_t count = 0;
  if (hipMemcpyAsync(&count, d_count, sizeof(int32_t), hipMemcpyDeviceToHost, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) {
    set_error(std::string("kh_graph_find_near_by_vertices: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
  g->last_near_by_ms = ms;
  if (count < 0 || static_cast<size_t>(count) > n) {set_error("kh_graph_find_near_by_vertices: hit count out of range"); return KH_ERR_HIP;}
  std::vector<int32_t> idx(static_cast<size_t>(count));
  std::vector<double> d2(static_cast<size_t>(count));
  if (count > 0 && (hipMemcpy(idx.data(), g->d_nb_idx, idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
    hipMemcpy(d2.data(), g->d_nb_d2, d2.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
  {
    set_error("kh_graph_find_near_by_vertices: download failed");
    return KH_ERR_HIP;
  }
  // SearchParams::sorted defaults to true (nanoflann.hpp:630): radiusSearch sorts the matches by ascending distance (:1418,
  // IndexDist_Sorter :227); between equal distances the library's rule is the lower index
  std::vector<int32_t> order(static_cast<size_t>(count));
  for (int32_t k = 0; k < count; ++k) {order[k] = k;}
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {return d2[a] < d2[b] || (d2[a] == d2[b] && idx[a] < idx[b]);});
  for (int32_t k = 0; k < count && k < cap; ++k) {scans[k] = idx[order[k]];}
  *n_found = count;
  return KH_OK;
}

double kh_graph_last_near_by_kernel_ms(kh_graph * g) {return g ? g->last_near_by_ms : 0.0;}

}  // extern "C"
namespace kh
{
// kh_graph_relocalize_candidates with vectors for the answer (the mapper's kh_mapper_relocalize calls this form).  The arguments
// have been checked by the caller.
int graph_relocalize_candidates(kh_graph * g, double seed_spacing, double base_radius, int32_t max_base, const double * center_xy, double radius,
  std::vector<int32_t> & seeds, std::vector<int32_t> & base_begin, std::vector<int32_t> & base_idx)
{
  const char * who = "kh_graph_relocalize_candidates";
  seeds.clear(); base_begin.assign(1, 0); base_idx.clear();
  g->last_relocalize_ms = 0.0;
  if (g->n == 0) {return KH_OK;}
  int rc = near_by_ready(g, who); if (rc) {return rc;}
  const size_t n = static_cast<size_t>(g->n);
  rc = ensure(g->d_rl_flag, g->cap_rl_flag, n); if (rc) {return rc;}
  rc = ensure(g->d_rl_prefix, g->cap_rl_prefix, n + 1); if (rc) {return rc;}
  rc = ensure(g->d_rl_seeds, g->cap_rl_seeds, n); if (rc) {return rc;}
  const double2 * pose = reinterpret_cast<const double2 *>(g->d_pose);
  const bool use_region = center_xy && radius > 0;
  double ms_total = 0.0;
  hipError_t err = hipSuccess;
  auto failed = [&]() {
      set_error(std::string(who) + ": " + hipGetErrorString(err));
      return KH_ERR_HIP;
    };
  // the kernels launched since ev[0], then `count` int32 from `src`, and a drained stream
  auto finish = [&](int32_t * dst, const int32_t * src, size_t count) {
      (void)hipEventRecord(g->ev[1], g->stream);
      err = hipGetLastError();
      if (err == hipSuccess) {err = hipMemcpyAsync(dst, src, count * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);}
      if (err == hipSuccess) {err = hipStreamSynchronize(g->stream);}
      if (err != hipSuccess) {return false;}
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
      ms_total += ms;
      return true;
    };
  // (1) seeds: flags, then their ordered list
  (void)hipEventRecord(g->ev[0], g->stream);
  hipLaunchKernelGGL(k_seed_cover, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, g->stream, pose, g->n, seed_spacing,
    use_region ? 1 : 0, use_region ? center_xy[0] : 0.0, use_region ? center_xy[1] : 0.0, radius * radius + kTol, g->d_rl_flag);
  hipLaunchKernelGGL(k_prefix_list, dim3(1), dim3(256), 0, g->stream, g->d_rl_flag, g->n, g->d_rl_prefix, g->d_rl_seeds);
  int32_t n_seeds = 0;
  if (!finish(&n_seeds, g->d_rl_prefix + n, 1)) {return failed();}
  if (n_seeds < 0 || static_cast<size_t>(n_seeds) > n) {set_error(std::string(who) + ": seed count out of range"); return KH_ERR_HIP;}
  g->last_relocalize_ms = ms_total;
  if (n_seeds == 0) {return KH_OK;}
  // (2) per seed: how many vertices in range, how many kept; base_begin = the prefix of the kept counts
  const size_t ns = static_cast<size_t>(n_seeds);
  rc = ensure(g->d_rl_count, g->cap_rl_count, 2 * ns); if (rc) {return rc;}
  rc = ensure(g->d_rl_begin, g->cap_rl_begin, ns + 1); if (rc) {return rc;}
  int32_t * d_raw = g->d_rl_count, * d_kept = g->d_rl_count + ns;
  const double range_sq_plus = base_radius * base_radius + kTol;         // Square(maxDistance) + KT_TOLERANCE, as k_loop_candidates
  const unsigned gather_blocks = static_cast<unsigned>((ns + 3) / 4);
  (void)hipEventRecord(g->ev[0], g->stream);
  hipLaunchKernelGGL(k_base_gather, dim3(gather_blocks), dim3(256), 0, g->stream, pose, g->n, g->d_rl_seeds, n_seeds, range_sq_plus, max_base, 0,
    d_raw, d_kept, static_cast<const int32_t *>(nullptr), static_cast<int32_t *>(nullptr));
  hipLaunchKernelGGL(k_prefix_list, dim3(1), dim3(256), 0, g->stream, d_kept, n_seeds, g->d_rl_begin, static_cast<int32_t *>(nullptr));
  int32_t total = 0;
  if (!finish(&total, g->d_rl_begin + ns, 1)) {return failed();}
  if (total < 0 || static_cast<size_t>(total) > ns * static_cast<size_t>(max_base)) {set_error(std::string(who) + ": base total out of range"); return KH_ERR_HIP;}
  // (3) the base lists, in list order
  rc = ensure(g->d_rl_idx, g->cap_rl_idx, std::max<size_t>(static_cast<size_t>(total), 1)); if (rc) {return rc;}
  seeds.resize(ns); base_begin.resize(ns + 1); base_idx.resize(static_cast<size_t>(total));
  (void)hipEventRecord(g->ev[0], g->stream);
  hipLaunchKernelGGL(k_base_gather, dim3(gather_blocks), dim3(256), 0, g->stream, pose, g->n, g->d_rl_seeds, n_seeds, range_sq_plus, max_base, 1,
    d_raw, d_kept, g->d_rl_begin, g->d_rl_idx);
  if (!finish(base_begin.data(), g->d_rl_begin, ns + 1)) {return failed();}
  err = hipMemcpyAsync(seeds.data(), g->d_rl_seeds, ns * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);
  if (err == hipSuccess && total > 0) {
    err = hipMemcpyAsync(base_idx.data(), g->d_rl_idx, static_cast<size_t>(total) * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);
  }
  if (err == hipSuccess) {err = hipStreamSynchronize(g->stream);}
  if (err != hipSuccess) {return failed();}
  g->last_relocalize_ms = ms_total;
  return KH_OK;
}
}  // namespace kh
extern "C" {

int kh_graph_relocalize_candidates(kh_graph * g, double seed_spacing, double base_radius, int32_t max_base, const double * center_xy, double radius,
  int32_t * seeds, int32_t cap_seeds, int32_t * n_seeds, int32_t * base_begin, int32_t * base_idx, int32_t cap_base, int32_t * n_base)
{
  if (!g || !n_seeds || !n_base || !base_begin || !(seed_spacing > 0) || !std::isfinite(seed_spacing) || !std::isfinite(base_radius) || base_radius < 0 ||
    max_base < 1 || radius != radius || cap_seeds < 0 || cap_base < 0 || (cap_seeds > 0 && !seeds) || (cap_base > 0 && !base_idx) ||
    (center_xy && !(std::isfinite(center_xy[0]) && std::isfinite(center_xy[1])))) {return KH_ERR_INVALID_ARG;}
  *n_seeds = 0; *n_base = 0; base_begin[0] = 0;
  std::vector<int32_t> s, b, idx;
  const int rc = kh::graph_relocalize_candidates(g, seed_spacing, base_radius, max_base, center_xy, radius, s, b, idx);
  if (rc) {return rc;}
  *n_seeds = static_cast<int32_t>(s.size()); *n_base = static_cast<int32_t>(idx.size());
  const size_t ws = std::min(s.size(), static_cast<size_t>(cap_seeds));
  std::copy(s.begin(), s.begin() + static_cast<std::ptrdiff_t>(ws), seeds);
  std::copy(b.begin(), b.begin() + static_cast<std::ptrdiff_t>(ws + 1), base_begin);
  std::copy(idx.begin(), idx.begin() + static_cast<std::ptrdiff_t>(std::min(idx.size(), static_cast<size_t>(cap_base))), base_idx);
  return KH_OK;
}

double kh_graph_last_relocalize_kernel_ms(kh_graph * g) {return g ? g->last_relocalize_ms : 0.0;}

int kh_graph_set_scan_limit(kh_graph * g, int32_t n_visit)
{
  if (!g || n_visit < 0 || n_visit > g->n) {return KH_ERR_INVALID_ARG;}
  g->n_visit = n_visit;
  return KH_OK;
}

// ---- host-side members of the row (exact reference arithmetic, O(neighbourhood) work) ---------------------
namespace
{
constexpr double kTolerance = 1e-06;      // KT_TOLERANCE, Math.h:41

inline double squared_distance(const double * a, const double * b)     // Vector2::SquaredDistance
{
  const double dx = a[0] - b[0], dy = a[1] - b[1];
  return dx * dx + dy * dy;
}

// BreadthFirstTraversal::TraverseForVertices with NearScanVisitor (Mapper.cpp:1263-1297, 1311-1333): valid
// vertices in visit order; the start vertex is visited like any other
void near_linked(const kh_graph * g, int32_t q, double max_distance, std::vector<int32_t> & valid)
{
  const double lim = max_distance * max_distance - kTolerance;       // Visit(): squaredDistance <= max^2 - tol
  const double * centre = &g->h_xy[2 * static_cast<size_t>(q)];
  std::vector<int32_t> queue(1, q);
  std::vector<uint8_t> seen(static_cast<size_t>(g->n), 0);
  seen[q] = 1;
  for (size_t h = 0; h < queue.size(); ++h) {
    const int32_t v = queue[h];
    if (squared_distance(&g->h_xy[2 * static_cast<size_t>(v)], centre) <= lim) {
      valid.push_back(v);
      for (int32_t k = g->h_adj_ptr[v]; k < g->h_adj_ptr[v + 1]; ++k) {
        const int32_t w = g->h_adj_idx[k];
        if (!seen[w]) {seen[w] = 1; queue.push_back(w);}
      }
    }
  }
}

void matrix3_inverse(const double * m, double * inv)    // Karto.h:2533-2577 (row-major 3x3)
{
  inv[0] = m[4] * m[8] - m[5] * m[7];
  inv[1] = m[2] * m[7] - m[1] * m[8];
  inv[2] = m[1] * m[5] - m[2] * m[4];
  inv[3] = m[5] * m[6] - m[3] * m[8];
  inv[4] = m[0] * m[8] - m[2] * m[6];
  inv[5] = m[2] * m[3] - m[0] * m[5];
  inv[6] = m[3] * m[7] - m[4] * m[6];
  inv[7] = m[1] * m[6] - m[0] * m[7];
  inv[8] = m[0] * m[4] - m[1] * m[3];
  const double det = m[0] * inv[0] + m[1] * inv[3] + m[2] * inv[6];
  if (std::fabs(det) <= 1e-14) {return;}      // assert(false) is compiled out in Release
  const double inv_det = 1.0 / det;
  for (int i = 0; i < 9; ++i) {inv[i] *= inv_det;}
}

double normalize_angle(double angle)   // math::NormalizeAngle, Math.h:181-202
{
  const double pi = 3.14159265358979323846, two_pi = 6.28318530717958647692;
  while (angle < -pi) {
    if (angle < -two_pi) {angle += static_cast<uint32_t>(angle / -two_pi) * two_pi;} else {angle += two_pi;}
  }
  while (angle > pi) {
    if (angle > two_pi) {angle -= static_cast<uint32_t>(angle / two_pi) * two_pi;} else {angle -= two_pi;}
  }
  return angle;
}
}  // namespace

int kh_graph_find_near_chains(
  kh_graph * g, int32_t query_scan, double link_scan_maximum_distance, int32_t * chains, int32_t cap_chains,
  int32_t * n_chains)
{
  if (!g || !n_chains || query_scan < 0 || query_scan >= g->n || (cap_chains > 0 && !chains)) {return KH_ERR_INVALID_ARG;}
  const double * pose = &g->h_xy[2 * static_cast<size_t>(query_scan)];
  const double lim = link_scan_maximum_distance * link_scan_maximum_distance + kTolerance;     // Mapper.cpp:1735-1737
  std::vector<int32_t> linked;
  near_linked(g, query_scan, link_scan_maximum_distance, linked);
  std::vector<uint8_t> processed(static_cast<size_t>(g->n), 0);
  int32_t total = 0;
  for (int32_t near : linked) {
    if (near == query_scan || processed[near]) {continue;}
    processed[near] = 1;
    bool valid = true;
    int32_t first = near, last = near;
    for (int32_t c = near - 1; c >= 0; --c) {                        // scans before (Mapper.cpp:1715-1746)
      if (c == query_scan) {valid = false;}
      if (squared_distance(pose, &g->h_xy[2 * static_cast<size_t>(c)]) < lim) {first = c; processed[c] = 1;} else {break;}
    }
    for (int32_t c = near + 1; c < g->n_visit; ++c) {                // scans after (Mapper.cpp:1751-1780); bound = scan map size
      if (c == query_scan) {valid = false;}
      if (squared_distance(pose, &g->h_xy[2 * static_cast<size_t>(c)]) < lim) {last = c; processed[c] = 1;} else {break;}
    }
    if (valid) {
      if (total < cap_chains) {chains[2 * total] = first; chains[2 * total + 1] = last;}
      ++total;
    }
  }
  *n_chains = total;
  return KH_OK;
}

int kh_graph_find_near_linked(kh_graph * g, int32_t query_scan, double max_distance, int32_t * scans, int32_t cap, int32_t * n_found)
{
  if (!g || !n_found || query_scan < 0 || query_scan >= g->n || (cap > 0 && !scans)) {return KH_ERR_INVALID_ARG;}
  std::vector<int32_t> valid;
  near_linked(g, query_scan, max_distance, valid);
  *n_found = static_cast<int32_t>(valid.size());
  for (int32_t k = 0; k < *n_found && k < cap; ++k) {scans[k] = valid[k];}
  return KH_OK;
}

int kh_graph_closest_scan_to_pose(kh_graph * g, const int32_t * scans, int32_t n, const double pose_xy[2], int32_t * closest)
{
  if (!g || !closest || !pose_xy || n < 0 || (n > 0 && !scans)) {return KH_ERR_INVALID_ARG;}
  int32_t best = -1;
  double best_d = 1.7976931348623157e308;                            // DBL_MAX
  for (int32_t k = 0; k < n; ++k) {
    if (scans[k] < 0 || scans[k] >= g->n) {return KH_ERR_INVALID_ARG;}
    const double d = squared_distance(pose_xy, &g->h_xy[2 * static_cast<size_t>(scans[k])]);
    if (d < best_d) {best_d = d; best = scans[k];}
  }
  *closest = best;                                                   // NULL (-1) for an empty chain
  return KH_OK;
}

int kh_weighted_mean(int32_t n, const double * means, const double * covariances, double mean[3])
{
  if (n <= 0 || !means || !covariances || !mean) {return KH_ERR_INVALID_ARG;}
  std::vector<double> inverses(9 * static_cast<size_t>(n));
  double sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int32_t k = 0; k < n; ++k) {
    double * inv = &inverses[9 * static_cast<size_t>(k)];
    for (int i = 0; i < 9; ++i) {inv[i] = 0.0;}
    matrix3_inverse(covariances + 9 * static_cast<size_t>(k), inv);
    for (int i = 0; i < 9; ++i) {sum[i] += inv[i];}
  }
  double inv_sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  matrix3_inverse(sum, inv_sum);
  double ax = 0.0, ay = 0.0, ah = 0.0, theta_x = 0.0, theta_y = 0.0;
  for (int32_t k = 0; k < n; ++k) {
    const double * p = means + 3 * static_cast<size_t>(k);
    const double * inv = &inverses[9 * static_cast<size_t>(k)];
    double sin_h, cos_h;
    ::sincos(p[2], &sin_h, &cos_h);          // one sincos like the reference's GCC build (see ref_sincos in matcher_host.cpp)
    theta_x += cos_h;
    theta_y += sin_h;
    double w[9];                                                     // inverseOfSumOfInverses * inverse, Karto.h:2634-2647
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        w[3 * r + c] = inv_sum[3 * r] * inv[c] + inv_sum[3 * r + 1] * inv[3 + c] + inv_sum[3 * r + 2] * inv[6 + c];
      }
    }
    // weight * pose (Karto.h:2654-2666), then Pose2::operator+= (Karto.h:2196-2200)
    ax += w[0] * p[0] + w[1] * p[1] + w[2] * p[2];
    ay += w[3] * p[0] + w[4] * p[1] + w[5] * p[2];
    ah = normalize_angle(ah + (w[6] * p[0] + w[7] * p[1] + w[8] * p[2]));
  }
  theta_x /= static_cast<double>(static_cast<size_t>(n));
  theta_y /= static_cast<double>(static_cast<size_t>(n));
  (void)ah;
  mean[0] = ax; mean[1] = ay; mean[2] = std::atan2(theta_y, theta_x);
  return KH_OK;
}

}  // extern "C"
