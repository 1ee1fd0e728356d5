// Visibility on a map (kh_map_visibility_*): what a sensor standing at a pose would see of a map view -- the
// distinct window cells its beams visit, by state, and those among them no committed viewpoint has seen.  The rule
// (tests/map_visibility_rule.py states it in numpy):
//
//   beam cells   beam b of sensor pose p walks TraceLine(c0, c1) outward as k_map_raycast does -- same states, same budget of unknown
//                cells, same early leave outside the window -- and leaves at step s_end; its visited cells are those of s = 0 .. s_end,
//                the leaving cell included: the HIT cell, the unknown cell that exceeded the budget, or c1 on FREE
//   Seen(p)      the WINDOW cells among the visited cells of all beams of p, each once; state 100 is occupied, 255 free, any other
//                unknown; the sensor's own cell is treated like any other
//   covered      one bit per window cell (bit row * width + column); a commit ORs Seen(p) into it
//   record       seen_* over Seen(p), new_* over Seen(p) minus covered, gain = w_unknown new_unknown + w_free new_free + w_occupied
//                new_occupied, beams_* by KH_RAY_ code
//   reach        floor(range_threshold * scale) + 2 bounds the Chebyshev distance from c0 to any c1; at most 511
//   select       k rounds of: gain of every unpicked candidate, the largest (ties to the smallest index), below min_gain the end,
//                else the pick recorded and committed
//
// The walk is the one walk of section 7m (RayWalk, cell_at, walk_bounded, occ_cell: occupancy_walk.hpp and occupancy_device.hpp).
// Sets, ORs and integer sums: no execution order shows in any result.  The handle: map_visibility.cpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "../../include/karto_hip.h"
#include "lds_attr.hpp"
#include "map_visibility_plan.hpp"
#include "occupancy_walk.hpp"

namespace kh
{
// One workgroup of four waves per pose.  Dynamic LDS: the bitmap of (2 reach + 1)^2 bits around the sensor cell, bit row * side +
// column, then the reduction's 4 x 9 words.  The workgroup clears the bitmap, takes the pose's beams in runs of 256 -- a lane walks
// its beam and sets the bit of every visited window cell with an LDS OR (Skip: a plain read first, the OR left out where the bit is
// set: the 64 lanes of a wave stand on the same cell at s = 0) --, and after a barrier shares out the bitmap's words: thread t takes
// words t, t + 256, ..; consecutive bits are consecutive cells of a row, so a wave's threads read neighbouring map bytes and mask
// words, and an empty word costs one LDS read.  Counting (Commit = false): per set bit the cell's state and its covered bit, six
// counters a lane; with the lane's three beam counters: lanes -> wave by shuffles, the waves through LDS, thread 0 writes the pose's
// record with plain stores -- one workgroup owns one record.  Committing: the set bits go into the global mask by atomicOr (several
// poses may commit at once), gathered per mask word first.  A far cell beyond the reach cannot occur (the host's bound); the lane
// that meets one sets head->error and stops.  In a select a picked candidate leaves at once, and every workgroup once done is set:
// both are known before the first barrier, to the whole workgroup.
template <bool Commit, bool Skip>
__global__ __launch_bounds__(256) void k_vis_gain(VisJob q, kh_visibility_t * __restrict__ out, int32_t from_head)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t vis_lds[];
  int32_t pose = (int32_t)blockIdx.x;
  if (q.picked != nullptr || from_head) {
    if (q.head->done != 0u) {return;}
    if (from_head) {pose = (int32_t)q.head->current;} else if (q.picked[pose] != 0u) {return;}
  }
  const MapWindow & g = q.g;
  const int32_t reach = q.reach, side = 2 * reach + 1;
  const uint32_t words = ((uint32_t)side * (uint32_t)side + 31u) >> 5;
  uint32_t * const bitmap = vis_lds;
  uint32_t * const part = vis_lds + words;
  for (uint32_t w = threadIdx.x; w < words; w += 256u) {bitmap[w] = 0u;}
  __syncthreads();

  const double sx = q.sensors[2 * (int64_t)pose], sy = q.sensors[2 * (int64_t)pose + 1];
  const int32_t x0 = occ_cell(sx, g.ax, g.scale), y0 = occ_cell(sy, g.ay, g.scale);
  uint32_t beams_free = 0u, beams_hit = 0u, beams_unknown = 0u;
  for (int32_t i = (int32_t)threadIdx.x; i < q.n_beams; i += 256) {
    const double * const p = q.points + 2 * ((int64_t)pose * q.n_beams + i);
    const int32_t x1 = occ_cell(p[0], g.ax, g.scale), y1 = occ_cell(p[1], g.ay, g.scale);
    const int64_t ex = (int64_t)x1 - x0, ey = (int64_t)y1 - y0;
    int32_t code = KH_RAY_FREE;
    if (walk_bounded(x0, y0, x1, y1)) {
      if (ex < -reach || ex > reach || ey < -reach || ey > reach) {q.head->error = 1u; continue;}
      RayWalk walk(x0, y0, x1, y1);
      const int32_t length = walk.length();
      int32_t unknown = 0;
      for (int32_t s = 0; s <= length; ++s, walk.next()) {
        const int32_t cx = walk.x(), cy = walk.y();
        const CellAt at = cell_at(g, cx, cy);
        uint32_t state = 0u;
        if (at.inside) {
          state = g.cells[at.k];
          // (|cx - x0| <= |ex| <= reach: the bit exists)
          const uint32_t bit = (uint32_t)(cy - y0 + reach) * (uint32_t)side + (uint32_t)(cx - x0 + reach);
          const uint32_t m = 1u << (bit & 31u);
          if (!Skip || (__hip_atomic_load(&bitmap[bit >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & m) == 0u) {atomicOr(&bitmap[bit >> 5], m);}
        } else if (q.max_unknown < 0 && ((at.wx < 0 && ex <= 0) || (at.wx >= g.width && ex >= 0) || (at.wy < 0 && ey <= 0) || (at.wy >= g.height && ey >= 0))) {
          break;
        }
        if (state == 100u) {code = KH_RAY_HIT; break;}
        if (state != 255u) {
          ++unknown;
          if (q.max_unknown >= 0 && unknown > q.max_unknown) {code = KH_RAY_UNKNOWN; break;}
        }
      }
    }
    beams_free += code == KH_RAY_FREE; beams_hit += code == KH_RAY_HIT; beams_unknown += code == KH_RAY_UNKNOWN;
  }
  __syncthreads();

  // the bitmap's first cell on the lattice, as window column / row (64-bit: the sensor may stand anywhere)
  const int64_t wx0 = (int64_t)x0 - reach - g.ox, wy0 = (int64_t)y0 - reach - g.oy;
  uint32_t seen_free = 0u, seen_occupied = 0u, seen_unknown = 0u, new_free = 0u, new_occupied = 0u, new_unknown = 0u;
  uint32_t pending_word = 0xFFFFFFFFu, pending_bits = 0u;      // Commit: the bits gathered for one word of the mask
  for (uint32_t w = threadIdx.x; w < words; w += 256u) {
    uint32_t v = bitmap[w];
    if (v == 0u) {continue;}
    uint32_t row = (w << 5) / (uint32_t)side, col = (w << 5) - row * (uint32_t)side;      // of the word's bit 0
    uint32_t at_bit = 0u;
    while (v != 0u) {
      const uint32_t b = (uint32_t)__ffs((int32_t)v) - 1u;
      v &= v - 1u;
      col += b - at_bit; at_bit = b;
      while (col >= (uint32_t)side) {col -= (uint32_t)side; ++row;}
      const int64_t wx = wx0 + col, wy = wy0 + row;
      if (wx < 0 || wx >= g.width || wy < 0 || wy >= g.height) {continue;}       // (only window cells were set: a guard)
      const uint32_t mi = (uint32_t)(wy * g.width + wx);
      if (Commit) {
        if ((mi >> 5) != pending_word) {
          if (pending_bits != 0u) {atomicOr(&q.mask[pending_word], pending_bits);}
          pending_word = mi >> 5; pending_bits = 0u;
        }
        pending_bits |= 1u << (mi & 31u);
      } else {
        const uint32_t state = g.cells[wx + wy * g.ws];
        const uint32_t fresh = ((q.mask[mi >> 5] >> (mi & 31u)) & 1u) ^ 1u;
        const uint32_t occupied = state == 100u, is_free = state == 255u, unknown = (occupied | is_free) ^ 1u;
        seen_free += is_free; seen_occupied += occupied; seen_unknown += unknown;
        new_free += is_free & fresh; new_occupied += occupied & fresh; new_unknown += unknown & fresh;
      }
    }
  }
  if (Commit) {
    if (pending_bits != 0u) {atomicOr(&q.mask[pending_word], pending_bits);}
    return;
  }
  const uint32_t n[kVisCounters] = {seen_free, seen_occupied, seen_unknown, new_free, new_occupied, new_unknown, beams_free, beams_hit, beams_unknown};
  const int32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int32_t k = 0; k < kVisCounters; ++k) {
    uint32_t v = n[k];
#pragma unroll
    for (int32_t d = 32; d >= 1; d >>= 1) {v += __shfl_xor(v, d);}
    if (lane == 0) {part[(threadIdx.x >> 6) * kVisCounters + k] = v;}
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s[kVisCounters];
#pragma unroll
    for (int32_t k = 0; k < kVisCounters; ++k) {s[k] = part[k] + part[kVisCounters + k] + part[2 * kVisCounters + k] + part[3 * kVisCounters + k];}
    kh_visibility_t r;
    r.seen_free = s[0]; r.seen_occupied = s[1]; r.seen_unknown = s[2]; r.new_free = s[3]; r.new_occupied = s[4]; r.new_unknown = s[5];
    r.gain = q.w_unknown * s[5] + q.w_free * s[3] + q.w_occupied * s[4];
    r.beams_free = s[6]; r.beams_hit = s[7]; r.beams_unknown = s[8];
    out[pose] = r;
  }
}

// One workgroup: the maximum of the 64-bit key gain << 32 | (0xFFFFFFFF - index) over the candidates whose picked word is not set --
// the largest gain, ties to the smallest index; lanes -> wave by shuffles, the waves through LDS.  Thread 0 records the pick, or sets
// done where its gain is below min_gain.  Nothing once done is set.  (k <= n: a round always finds an unpicked candidate; key 0 would
// be "none", and is treated as a gain of 0.)
__global__ __launch_bounds__(256) void k_vis_best(const kh_visibility_t * __restrict__ records, int32_t n, uint32_t min_gain, uint32_t * __restrict__ picked,
  VisHead * __restrict__ head, uint32_t * __restrict__ picks, uint32_t * __restrict__ gains)
{
  __shared__ unsigned long long part[4];
  if (head->done != 0u) {return;}
  unsigned long long key = 0ull;
  for (int32_t p = (int32_t)threadIdx.x; p < n; p += 256) {
    if (picked[p] == 0u) {
      const unsigned long long k = ((unsigned long long)records[p].gain << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)p);
      key = k > key ? k : key;
    }
  }
#pragma unroll
  for (int32_t d = 32; d >= 1; d >>= 1) {
    const unsigned long long other = __shfl_xor(key, d);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) {part[threadIdx.x >> 6] = key;}
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int32_t k = 1; k < 4; ++k) {key = part[k] > key ? part[k] : key;}
    const uint32_t gain = (uint32_t)(key >> 32), index = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    if (key == 0ull || gain < min_gain) {
      head->done = 1u;
    } else {
      const uint32_t slot = head->n_picked;
      picks[slot] = index; gains[slot] = gain;
      picked[index] = 1u;
      head->current = index; head->n_picked = slot + 1u;
    }
  }
}

namespace
{
// the launch of one instantiation: its dynamic-LDS limit once per device, then the kernel
template <bool Commit, bool Skip>
bool vis_launch(hipStream_t stream, const VisJob & job, unsigned blocks, kh_visibility_t * d_out, int32_t from_head)
{
  static std::atomic<unsigned long long> allowed{0};
  const int32_t bytes = vis_lds_bytes(job.reach);
  if (job.reach < 0 || job.reach > kVisMaxReach || bytes > kVisMaxLdsBytes) {return false;}
  allow_dynamic_lds(reinterpret_cast<const void *>(&k_vis_gain<Commit, Skip>), vis_lds_bytes(kVisMaxReach), allowed);
  hipLaunchKernelGGL((k_vis_gain<Commit, Skip>), dim3(blocks), dim3(256), static_cast<size_t>(bytes), stream, job, d_out, from_head);
  return true;
}
}  // namespace

bool vis_gain(void * stream, const VisJob & job, int32_t n_poses, bool skip, kh_visibility_t * d_out)
{
  hipStream_t s = static_cast<hipStream_t>(stream);
  return skip ? vis_launch<false, true>(s, job, static_cast<unsigned>(n_poses), d_out, 0) : vis_launch<false, false>(s, job, static_cast<unsigned>(n_poses), d_out, 0);
}

bool vis_commit(void * stream, const VisJob & job, int32_t n_poses, bool skip, bool from_head)
{
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned blocks = from_head ? 1u : static_cast<unsigned>(n_poses);
  return skip ? vis_launch<true, true>(s, job, blocks, nullptr, from_head ? 1 : 0) : vis_launch<true, false>(s, job, blocks, nullptr, from_head ? 1 : 0);
}

void vis_best(void * stream, const kh_visibility_t * d_records, int32_t n, uint32_t min_gain, uint32_t * d_picked, VisHead * d_head, uint32_t * d_picks,
  uint32_t * d_gains)
{
  hipLaunchKernelGGL(k_vis_best, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d_records, n, min_gain, d_picked, d_head, d_picks, d_gains);
}
}  // namespace kh
