// K6 of the pose-graph SPA solver (hot path B), the LEVEL PIPELINE behind the pivot blocks (k_potrf, spa_potrf.hip, whose opening
// comment describes the pipeline as a whole): with W = L11^-T of every front of a level in winv,
//   k_trsm<32|64>        L21 = F21 W over row slabs of every front, chip-wide, and the forward solve's upd -= L21 y1
//   k_syrk<32|64>        F22 -= L21 L21^T over tiles of every front, chip-wide; the result goes into the parent front (scatter mode)
//   k_front_update       both of the above for one front per workgroup with L21 resident in LDS (the wide levels of small fronts)
//   k_backward3<narrow>  backward solve of a level, two matrix-vector products with W and L21
//   k_zero_update_blocks, k_count_nonzero   self-cleaning fronts: the blocks nobody else zeroes, and the debug check of it
// Launchers: spa_launch_update_level, spa_launch_front_update (+ spa_front_update_lds, asked by spa_problem.cpp),
// spa_launch_backward3_level, spa_launch_zero_update_blocks, spa_launch_count_nonzero; called by spa_compute.cpp, the zeroing also
// by spa_covariance.cpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "lds_attr.hpp"
#include "spa_device.hpp"

#pragma clang fp contract(fast)

namespace kh
{

// rows [prow0, prow0 + R) x columns [0, nsp) of the panel columns of a front -> LDS rows of stride LD (zeros outside
// nr rows / ns columns), LU loads in flight per thread; with kids, the children's update matrices are added (the
// same thread handles the same entry in every pass: no barrier in between).  R is a constant for the slab kernels and
// the front's whole padded F21 (column by column) for k_front_update.
template <int LU>
__device__ __forceinline__ void stage_rows(double * S, int LD, int R, const SpaDev & d, const FrontDesc & fd, int prow0, int nr, int ns, int nsp, int nkids,
                                           const double * Bfront, int tid, int nthreads)
{
  const int m = fd.m, mp = m / 3;
  const double * Fcol0 = d.fronts + fd.off + prow0;
  const double * Bcol0 = Bfront ? Bfront + prow0 : nullptr;
  for (int base = 0; base < R * nsp; base += LU * nthreads) {
    double v[LU];
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int idx = base + u * nthreads + tid;
      const int c = idx / R, i = idx - c * R;
      const bool want = idx < R * nsp && i < nr && c < ns;
      v[u] = *(want ? Fcol0 + i + (int64_t)c * m : Fcol0);
    }
    if (Bcol0) {
#pragma unroll
      for (int u = 0; u < LU; ++u) {
        const int idx = base + u * nthreads + tid;
        const int c = idx / R, i = idx - c * R;
        const bool want = idx < R * nsp && i < nr && c < ns;
        const double * bp = want ? Bcol0 + i + (int64_t)c * m : Bcol0;
        v[u] += *bp;
        if (want) {*const_cast<double *>(bp) = 0.0;}          // self-cleaning (buffer A's entries become L21)
      }
    }
    for (int s = 0; s < nkids; ++s) {
      const ChildInfo ci = child_info(d, fd, s);
      const int32_t * inv = d.cinv + fd.cinv_ptr + s * mp;
#pragma unroll
      for (int u = 0; u < LU; ++u) {
        const int idx = base + u * nthreads + tid;
        const int c = idx / R, i = idx - c * R;
        const bool want = idx < R * nsp && i < nr && c < ns;
        const double g = gather_entry(d.fronts, ci, inv, want ? prow0 + i : 0, want ? c : 0);
        v[u] += want ? g : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int idx = base + u * nthreads + tid;
      const int c = idx / R, i = idx - c * R;
      if (idx < R * nsp) {S[(size_t)i * LD + c] = (i < nr && c < ns) ? v[u] : 0.0;}
    }
  }
}

// L21 = F21 W for a slab of R rows of one front (grid: front x slab), then upd -= L21 y1.  A wave owns column blocks
// of 16: the W entries of a block -- up to 128 k x 16 columns, 32 loads per lane -- are all requested before the first
// MFMA (a loop over k blocks with its loads inside is a chain of L2 latencies), and serve the R / 16 row tiles of the slab.
template <int R>
__global__ __launch_bounds__(512) void k_trsm(SpaDev d, int first_front, const double * __restrict__ rhs, double * upd, int lds_nsp)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  const int r0 = R * (int)blockIdx.y;
  if (r0 >= nu) {return;}
  const int nr = min(R, nu - r0);
  const int nsp = (ns + NB - 1) & ~(NB - 1), nt = nsp >> 4, LD = nsp + 2;
  double * F = d.fronts + fd.off;
  const double * W = d.winv + fd.woff;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  extern __shared__ double smem[];
  double * S = smem;                                         // [R][LD] the slab of F21
  double * yv = smem + (size_t)R * (lds_nsp + 2);            // [lds_nsp] y1
  double * red = yv + lds_nsp;                               // [8][R] per-wave partial sums of L21 y1 (four or eight waves)
  const int first = 3 * fd.first;
  constexpr int RT = R / NB;
  constexpr int NTMAX = kPotrfMaxNs / NB;
  double * uk = upd + 3 * (int64_t)fd.rows_ptr;
  const double uold = tid < nr ? uk[r0 + tid] : 0.0;
  for (int j = tid; j < nsp; j += nthreads) {yv[j] = j < ns ? rhs[first + j] : 0.0;}
  for (int j = tid; j < 8 * R; j += nthreads) {red[j] = 0.0;}
  stage_rows<16>(S, LD, R, d, fd, ns + r0, nr, ns, nsp, front_nkids(d, fd), front_b(d, fd), tid, nthreads);
  __syncthreads();
  double part[RT];
#pragma unroll
  for (int it = 0; it < RT; ++it) {part[it] = 0.0;}
  for (int q = wave; q < nt; q += nwaves) {
    const int J = (q & 1) ? nt - 1 - (q >> 1) : (q >> 1);      // long and short K ranges alternate
    const double * wcol = W + (NB * J + lr);                   // (L^-T)[k][16 J + lr] = W[(16 J + lr) + k * nsp]
    double a[NTMAX][4];
#pragma unroll
    for (int K = 0; K < NTMAX; ++K) {
      const int Kc = K <= J ? K : 0;                           // always a valid address: no load under a branch
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {a[K][kk] = wcol[(int64_t)(NB * Kc + 4 * lk + kk) * nsp];}
    }
    v4d acc[RT];
#pragma unroll
    for (int it = 0; it < RT; ++it) {acc[it] = v4d{0.0, 0.0, 0.0, 0.0};}
#pragma unroll
    for (int K = 0; K < NTMAX; ++K) {
      if (K <= J) {                                            // wave-uniform
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
          for (int it = 0; it < RT; ++it) {
            acc[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[K][kk], S[(NB * it + lr) * LD + NB * K + 4 * lk + kk], acc[it], 0, 0, 0);
          }
        }
      }
    }
    // lane (lr, lk) holds L21[16 it + lr][16 J + lk + 4 r]
#pragma unroll
    for (int it = 0; it < RT; ++it) {
      const int row = NB * it + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = NB * J + lk + 4 * r;
        if (row < nr && col < ns) {F[(ns + r0 + row) + (int64_t)col * m] = acc[it][r];}
        part[it] += acc[it][r] * yv[col];                      // yv is zero on the padding columns
      }
    }
  }
  // forward solve: upd[row] -= sum_j L21[row][j] y1[j]; the four lane groups and the waves add up in a fixed order
#pragma unroll
  for (int it = 0; it < RT; ++it) {
    double p = part[it];
    p += __shfl_xor(p, 16);
    p += __shfl_xor(p, 32);
    if (lk == 0) {red[wave * R + NB * it + lr] = p;}
  }
  __syncthreads();
  if (tid < nr) {
    uk[r0 + tid] = uold - (((red[tid] + red[R + tid]) + (red[2 * R + tid] + red[3 * R + tid])) +
                           ((red[4 * R + tid] + red[5 * R + tid]) + (red[6 * R + tid] + red[7 * R + tid])));
  }
}

// F22 -= L21 L21^T, one TS x TS tile of the lower triangle per workgroup (grid: front x tile).  TS = 64: eight waves,
// each with a pair of 16 x 16 sub-tiles that share the row operand (two independent accumulators: the matrix pipe sees
// back-to-back MFMAs while the next operands arrive from LDS); TS = 32: four waves, one sub-tile each.
template <int TS>
__global__ __launch_bounds__(TS * 8) void k_syrk(SpaDev d, int first_front, int lds_nsp)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  const int ntm = (nu + TS - 1) / TS;
  const int t = blockIdx.y;
  if (t >= ntm * (ntm + 1) / 2) {return;}
  int I = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  I -= (I * (I + 1) / 2 > t) ? 1 : 0;
  I += ((I + 1) * (I + 2) / 2 <= t) ? 1 : 0;
  const int J = t - I * (I + 1) / 2;
  const int nsp = (ns + NB - 1) & ~(NB - 1), LD = nsp + 2;
  double * F = d.fronts + fd.off;
  const double * Bf = front_b(d, fd);
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  extern __shared__ double smem[];
  double * XA = smem;                                               // rows of tile row I: [TS][LD]
  double * XB = (I == J) ? XA : smem + (size_t)TS * (lds_nsp + 2);  // rows of tile column J
  constexpr int UT = TS / 32;                  // sub-tiles per wave (side by side)
  constexpr int PW = (TS / NB) / UT;           // waves per sub-tile row
  const int si = wave / PW, sj0 = UT * (wave - si * PW);
  // accumulators first: their loads fly while the panel rows are staged
  // (own entries + buffer B, self-cleaning: written out a second time in front_update_body's syrk phase -- change both)
  v4d acc[UT];
  bool live[UT];
  const int row = TS * I + NB * si + lr;
#pragma unroll
  for (int u = 0; u < UT; ++u) {
    const int sj = sj0 + u;
    live[u] = !(I == J && sj > si);
    const int col0 = TS * J + NB * sj + lk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = col0 + 4 * r;
      const bool ok = live[u] && row < nu && col <= row;
      const int64_t at = ok ? (ns + row) + (int64_t)(ns + col) * m : 0;
      double v = F[at];
      if (Bf) {v += Bf[at];}
      acc[u][r] = ok ? v : 0.0;
      if (d.scatter && ok) {                                   // self-cleaning: the tile leaves for the parent front (or is stored below)
        F[at] = 0.0;
        if (Bf) {const_cast<double *>(Bf)[at] = 0.0;}
      }
    }
  }
  // where the tile goes: into the parent front (round 6), or back where it came from
  const int mode = d.scatter ? (fd.flags & 3) : 0;
  int prow = 0, pcol[UT][4];
  int64_t pm = 0;
  double * P = nullptr;
  if (mode != 0) {
    const FrontDesc & pd = d.desc[fd.parent];
    const int32_t * rp = d.relpos + fd.relpos_ptr;
    const int rowc = min(row, nu - 1);
    prow = 3 * rp[rowc / 3] + rowc % 3;
#pragma unroll
    for (int u = 0; u < UT; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int colc = min(TS * J + NB * (sj0 + u) + lk + 4 * r, nu - 1);
        pcol[u][r] = 3 * rp[colc / 3] + colc % 3;
      }
    }
    pm = pd.m;
    P = (mode == 1 ? d.fronts : d.fronts_b) + pd.off;
  }
  {
    // the children's update matrices join here (the front's own F22 holds only its assembled entries)
    // (the same walk is in front_update_body's syrk phase -- change both)
    const int nkids = front_nkids(d, fd), mp = m / 3;
    for (int s = 0; s < nkids; ++s) {
      const ChildInfo ci = child_info(d, fd, s);
      const int32_t * inv = d.cinv + fd.cinv_ptr + s * mp;
#pragma unroll
      for (int u = 0; u < UT; ++u) {
        const int col0 = TS * J + NB * (sj0 + u) + lk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = col0 + 4 * r;
          const bool ok = live[u] && row < nu && col <= row;
          const double g = gather_entry(d.fronts, ci, inv, ok ? ns + row : 0, ok ? ns + col : 0);
          acc[u][r] += ok ? g : 0.0;
        }
      }
    }
  }
  stage_rows<16>(XA, LD, TS, d, fd, ns + TS * I, min(TS, nu - TS * I), ns, nsp, 0, nullptr, tid, nthreads);      // L21 is final: no children
  if (I != J) {stage_rows<16>(XB, LD, TS, d, fd, ns + TS * J, min(TS, nu - TS * J), ns, nsp, 0, nullptr, tid, nthreads);}
  __syncthreads();
  if (live[0]) {            // (the one- or two-tile rank-k loop is also front_update_body's -- change both)
    const double * xb = XA + (NB * si + lr) * LD + 4 * lk;
    const double * xa0 = XB + (NB * sj0 + lr) * LD + 4 * lk;
    if (UT == 2 && live[UT - 1]) {
      const double * xa1 = xa0 + NB * LD;
      for (int K = 0; K < nsp; K += NB) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const double b = xb[K + kk];
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa0[K + kk], b, acc[0], 0, 0, 0);
          acc[UT - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa1[K + kk], b, acc[UT - 1], 0, 0, 0);
        }
      }
    } else {
      for (int K = 0; K < nsp; K += NB) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa0[K + kk], xb[K + kk], acc[0], 0, 0, 0);}
      }
    }
  }
  // (the parent scatter is also front_update_body's, with the rows' places read from LDS there -- change both)
#pragma unroll
  for (int u = 0; u < UT; ++u) {
    const int col0 = TS * J + NB * (sj0 + u) + lk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = col0 + 4 * r;
      if (live[u] && row < nu && col <= row) {
        if (mode != 0) {
          unsafeAtomicAdd(P + prow + pcol[u][r] * pm, acc[u][r]);
        } else {
          F[(ns + row) + (int64_t)(ns + col) * m] = acc[u][r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_front_update (round 6): k_trsm AND k_syrk of one front in ONE workgroup, L21 resident in LDS.
//
// On the wide levels of the tree (hundreds of fronts of 200-300 rows with 60-80 pivots) the split kernels are bound by what
// they re-read: every 64 x 64 tile of k_syrk stages its two 64-row slabs of L21 from the L2 again (level 0 of the 10k-node
// graph: 282 MB of slabs + 135 MB of update blocks + 67 MB of scatter in 61 us = the L2's rate, for 0.5 GFLOP), after k_trsm
// has written L21 and before that staged F21 once per slab.  A front of such a level fits one compute unit's LDS whole:
//   stage   F21 (both buffers, and the children read in place) -> S [nup][LD], W -> Wl [nsp][LDW], y1, the rows' places in the
//           parent
//   trsm    a wave per 16-row tile: L21 = F21 W with one accumulator per column block (independent MFMAs back to back),
//           written over the tile's own rows of S, to the front (the backward sweep reads it) and into upd -= L21 y1
//   syrk    16 x 16 sub-tiles of F22 -= L21 L21^T, two at a time per wave (they share the row operand), operands straight from
//           S; initial values from the front (both buffers), results added into the parent (or stored, Symbolic::scatter_mode)
// so F21, W and F22 are read once and L21 is written once.  The host sends the fronts of a level that fit (front_update_fits)
// here when there are enough of them to fill the chip; the larger ones (the head of the level: fronts are sorted by size) keep
// k_trsm / k_syrk.
constexpr int kFuThreads = 1024, kFuWaves = kFuThreads / 64;
constexpr int kFuMaxNt = 5;          // pivot blocks of up to 80 columns (the leaves of the dissection: 24 nodes = 72): one accumulator per column
                                     // block in the trsm phase, and 1024 threads leave a lane 128 registers

static size_t front_update_lds_bytes(int m, int ns)
{
  const int nu = m - ns, nup = (nu + NB - 1) & ~(NB - 1), nsp = (ns + NB - 1) & ~(NB - 1);
  return sizeof(double) * ((size_t)nup * (nsp + 2) + (size_t)nsp * (nsp + 4) + nsp + 8) + sizeof(int32_t) * (size_t)(nup / 3 + 8);
}
// LDS a front takes in k_front_update, 0 when it does not fit (or has no rows below the pivot block: nothing to do)
size_t spa_front_update_lds(int32_t m, int32_t ns)
{
  if (ns > NB * kFuMaxNt || m <= ns) {return 0;}
  const size_t b = front_update_lds_bytes(m, ns);
  return b <= 160 * 1024 - 512 ? b : 0;
}

template <int kWaves, int kMaxNt>
__device__ __forceinline__ void front_update_body(const SpaDev & d, const FrontDesc & fd, const double * rhs, double * upd)
{
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  if (nu <= 0) {return;}
  const int nsp = (ns + NB - 1) & ~(NB - 1), nt = nsp >> 4, LD = nsp + 2, LDW = nsp + 4;
  const int nup = (nu + NB - 1) & ~(NB - 1), nrt = nup >> 4;
  double * F = d.fronts + fd.off;
  const double * Bf = front_b(d, fd);
  const double * W = d.winv + fd.woff;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  extern __shared__ double smem[];
  double * S = smem;                                   // [nup][LD]   F21, then L21
  double * Wl = S + (size_t)nup * LD;                  // [nsp][LDW]  Wl[k][j] = (L^-T)[k][j]
  double * yv = Wl + (size_t)nsp * LDW;                // [nsp]       y1
  int32_t * rpp = reinterpret_cast<int32_t *>(yv + nsp + 8);       // [nup / 3 + 1]  the struct rows' places in the parent (node units)
  const int first = 3 * fd.first;
  const int nkids = front_nkids(d, fd), mp = m / 3;
  const int mode = d.scatter ? (fd.flags & 3) : 0;
  // ---- stage ----
  for (int j = tid; j < nsp; j += nthreads) {yv[j] = j < ns ? rhs[first + j] : 0.0;}
  if (mode != 0) {
    const int32_t * rp = d.relpos + fd.relpos_ptr;
    for (int j = tid; j < nup / 3 + 1; j += nthreads) {rpp[j] = rp[min(j, nu / 3 - 1)];}
  }
  for (int idx = tid; idx < nsp * nsp; idx += nthreads) {
    const int k = idx / nsp, j = idx - k * nsp;
    Wl[k * LDW + j] = j >= (k & ~(NB - 1)) ? W[j + (int64_t)k * nsp] : 0.0;      // (left of the diagonal block W holds nothing)
  }
  stage_rows<8>(S, LD, nup, d, fd, ns, nu, ns, nsp, nkids, Bf, tid, nthreads);
  __syncthreads();
  // ---- trsm ----
  double * uk = upd + 3 * (int64_t)fd.rows_ptr;
  for (int it = wave; it < nrt; it += kWaves) {
    v4d acc[kMaxNt];
#pragma unroll
    for (int J = 0; J < kMaxNt; ++J) {acc[J] = v4d{0.0, 0.0, 0.0, 0.0};}
    const double * srow = S + (size_t)(NB * it + lr) * LD + 4 * lk;
#pragma unroll
    for (int K = 0; K < kMaxNt; ++K) {
      if (K < nt) {
        double b[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {b[kk] = srow[NB * K + kk];}
        const double * wk = Wl + (size_t)(NB * K + 4 * lk) * LDW + lr;
#pragma unroll
        for (int J = K; J < kMaxNt; ++J) {
          if (J < nt) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(wk[kk * LDW + NB * J], b[kk], acc[J], 0, 0, 0);}
          }
        }
      }
    }
    // lane (lr, lk) holds L21[16 it + lr][16 J + lk + 4 r]: over the tile's own rows of S (nobody else reads them before the
    // barrier), to the front, and into the forward solve
    const int row = NB * it + lr;
    double part = 0.0;
#pragma unroll
    for (int J = 0; J < kMaxNt; ++J) {
      if (J < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = NB * J + lk + 4 * r;
          S[(size_t)row * LD + col] = acc[J][r];
          if (row < nu && col < ns) {F[(ns + row) + (int64_t)col * m] = acc[J][r];}
          part += acc[J][r] * yv[col];                             // yv is zero on the padding columns
        }
      }
    }
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    if (lk == 0 && row < nu) {uk[row] -= part;}
  }
  __syncthreads();
  // ---- syrk ----
  const FrontDesc * pd = mode != 0 ? d.desc + fd.parent : nullptr;
  const int64_t pm = pd ? pd->m : 0;
  double * P = pd ? (mode == 1 ? d.fronts : d.fronts_b) + pd->off : nullptr;
  // units: (si, pair of sub-tile columns 2 u, 2 u + 1), si = 0 .. nrt - 1, u = 0 .. si / 2, numbered row by row
  int unit = wave;
  int si = 0, ubase = 0;                               // ubase = units before tile row si
  const int nunits = [&]() {int n = 0; for (int q = 0; q < nrt; ++q) {n += q / 2 + 1;} return n;}();
  for (; unit < nunits; unit += kWaves) {
    while (unit >= ubase + si / 2 + 1) {ubase += si / 2 + 1; ++si;}
    const int sj0 = 2 * (unit - ubase);
    const bool two = sj0 + 1 <= si;
    const int row = NB * si + lr;
    // The four pieces from here to the end of the loop -- own entries + buffer B with the self-cleaning stores, the children read
    // in place, the one- or two-tile rank-k loop, the parent scatter -- are k_syrk's, written out a second time: change both.  (As
    // shared __forceinline__ helpers each of them compiled to a different instruction stream in both kernels.)
    v4d acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = NB * (sj0 + u) + lk + 4 * r;
        const bool ok = (u == 0 || two) && row < nu && col <= row;
        const int64_t at = ok ? (ns + row) + (int64_t)(ns + col) * m : 0;
        double v = F[at];
        if (Bf) {v += Bf[at];}
        acc[u][r] = ok ? v : 0.0;
        if (d.scatter && ok) {
          F[at] = 0.0;
          if (Bf) {const_cast<double *>(Bf)[at] = 0.0;}
        }
      }
    }
    for (int s = 0; s < nkids; ++s) {
      const ChildInfo ci = child_info(d, fd, s);
      const int32_t * inv = d.cinv + fd.cinv_ptr + s * mp;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = NB * (sj0 + u) + lk + 4 * r;
          const bool ok = (u == 0 || two) && row < nu && col <= row;
          const double g = gather_entry(d.fronts, ci, inv, ok ? ns + row : 0, ok ? ns + col : 0);
          acc[u][r] += ok ? g : 0.0;
        }
      }
    }
    const double * xb = S + (size_t)(NB * si + lr) * LD + 4 * lk;
    const double * xa0 = S + (size_t)(NB * sj0 + lr) * LD + 4 * lk;
    const double * xa1 = xa0 + (two ? NB * LD : 0);
    if (two) {
      for (int K = 0; K < nsp; K += NB) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const double b = xb[K + kk];
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa0[K + kk], b, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa1[K + kk], b, acc[1], 0, 0, 0);
        }
      }
    } else {
      for (int K = 0; K < nsp; K += NB) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa0[K + kk], xb[K + kk], acc[0], 0, 0, 0);}
      }
    }
    const int rowc = min(row, nu - 1);
    const int64_t prow = mode != 0 ? 3 * (int64_t)rpp[rowc / 3] + rowc % 3 : 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = NB * (sj0 + u) + lk + 4 * r;
        if ((u == 0 || two) && row < nu && col <= row) {
          if (mode != 0) {
            const int64_t pcol = 3 * (int64_t)rpp[col / 3] + col % 3;
            unsafeAtomicAdd(P + prow + pcol * pm, acc[u][r]);
          } else {
            F[(ns + row) + (int64_t)(ns + col) * m] = acc[u][r];
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(kFuThreads) void k_front_update(SpaDev d, int first_front, const double * __restrict__ rhs, double * upd)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  front_update_body<kFuWaves, kFuMaxNt>(d, fd, rhs, upd);
}

void spa_launch_front_update(const SpaDev & d, int32_t first_front, int32_t n, size_t lds_bytes, const double * rhs, double * upd, void * stream)
{
  if (n <= 0) {return;}
  static std::atomic<unsigned long long> done{0};
  allow_dynamic_lds(reinterpret_cast<const void *>(k_front_update), 160 * 1024 - 256, done);
  hipLaunchKernelGGL(k_front_update, dim3(n), dim3(kFuThreads), lds_bytes, (hipStream_t)stream, d, first_front, rhs, upd);
}

// Backward solve of a level with W = L11^-T:  x1 = W (y1 - L21^T x2), two sets of independent dot products, one wave per
// pair of columns.  (A variant that requested every entry of L21 and W a wave needs right after the descriptor -- 80 loads
// per lane, fully unrolled -- was SLOWER, 306 us per sweep against 177: these kernels run once per level, and a long
// straight-line body is paid for in instruction fetch.)
template <bool kNarrow>
__global__ __launch_bounds__(1024) void k_backward3(SpaDev d, int first_front, double * rhs)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  const int nsp = (ns + NB - 1) & ~(NB - 1);
  const double * F = d.fronts + fd.off;
  const double * W = d.winv + fd.woff;
  const int first = 3 * fd.first;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
  extern __shared__ double sb[];                 // [m] : w (pivots) | x2 (struct rows), then [nsp] x1
  double * xo = sb + m;
  const int32_t * rows = d.front_rows + fd.rows_ptr;
  for (int t = tid; t < ns; t += nthreads) {sb[t] = rhs[first + t];}
  for (int q = tid; q < nu; q += nthreads) {sb[ns + q] = rhs[3 * rows[q / 3] + q % 3];}
  __syncthreads();
  if (kNarrow) {
    // NARROW levels (a handful of fronts: latency is everything).  Eight lanes per column, 128 columns at a time: every column
    // of the pivot block is in flight at once (with a wave per pair of columns a 126-pivot front took its 63 pairs in four
    // rounds of sixteen, each round a memory latency of its own).  On the wide levels the 64-byte pieces of this form cost more
    // than the rounds (measured: 17.6 -> 21.0 us on the 69-front level), so they keep the wave per pair.
    const int grp = tid >> 3, sub = tid & 7, ngrp = nthreads >> 3;
    // w[c] = y1[c] - L21[:, c] . x2
    for (int c = grp; c < ns; c += ngrp) {
      const double * col = F + ns + (int64_t)c * m;
      double a0 = 0.0;
#pragma unroll 4
      for (int i = sub; i < nu; i += 8) {
        a0 += col[i] * sb[ns + i];
        if (d.scatter) {const_cast<double *>(col)[i] = 0.0;}        // self-cleaning fronts: this was the last reader of L21
      }
      a0 += __shfl_xor(a0, 1); a0 += __shfl_xor(a0, 2); a0 += __shfl_xor(a0, 4);
      if (sub == 0) {sb[c] -= a0;}
    }
    __syncthreads();
    // x1[c] = sum_{j >= c} (L^-T)[c][j] w[j],  (L^-T)[c][j] = W[j + c * nsp]  (zeros left of the diagonal)
    for (int c = grp; c < ns; c += ngrp) {
      const double * w0 = W + (int64_t)c * nsp;
      double a0 = 0.0;
#pragma unroll 4
      for (int j = c + sub; j < ns; j += 8) {a0 += w0[j] * sb[j];}
      a0 += __shfl_xor(a0, 1); a0 += __shfl_xor(a0, 2); a0 += __shfl_xor(a0, 4);
      if (sub == 0) {xo[c] = a0;}
    }
  } else {
    // w[c] = y1[c] - L21[:, c] . x2
    for (int c = 2 * wave; c < ns; c += 2 * nwaves) {
      const double * col0 = F + ns + (int64_t)c * m;
      const double * col1 = col0 + (c + 1 < ns ? m : 0);
      double a0 = 0.0, a1 = 0.0;
      for (int i = lane; i < nu; i += 64) {
        const double x = sb[ns + i];
        a0 += col0[i] * x;
        a1 += col1[i] * x;
        if (d.scatter) {                        // self-cleaning fronts: this was the last reader of L21
          const_cast<double *>(col0)[i] = 0.0;
          if (c + 1 < ns) {const_cast<double *>(col1)[i] = 0.0;}
        }
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {a0 += __shfl_xor(a0, s); a1 += __shfl_xor(a1, s);}
      if (lane == 0) {sb[c] -= a0; if (c + 1 < ns) {sb[c + 1] -= a1;}}
    }
    __syncthreads();
    // x1[c] = sum_{j >= c} (L^-T)[c][j] w[j],  (L^-T)[c][j] = W[j + c * nsp]  (zeros left of the diagonal)
    for (int c = 2 * wave; c < ns; c += 2 * nwaves) {
      const double * w0 = W + (int64_t)c * nsp;
      const double * w1 = w0 + (c + 1 < ns ? nsp : 0);
      double a0 = 0.0, a1 = 0.0;
      for (int j = c + lane; j < ns; j += 64) {
        const double wj = sb[j];
        a0 += w0[j] * wj;
        a1 += j > c ? w1[j] * wj : 0.0;       // row c + 1 starts at column c + 1: left of it W holds nothing (not even zeros when
      }                                        // c + 1 opens a new block of 16)
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {a0 += __shfl_xor(a0, s); a1 += __shfl_xor(a1, s);}
      if (lane == 0) {xo[c] = a0; if (c + 1 < ns) {xo[c + 1] = a1;}}
    }
  }
  __syncthreads();
  for (int t = tid; t < ns; t += nthreads) {rhs[first + t] = xo[t];}
}

// self-cleaning fronts: the update matrices that stayed in place (children their parent reads through cinv) are zeroed here,
// after the factorisation; list = those fronts, one workgroup per (front, 16 columns)
__global__ __launch_bounds__(256) void k_zero_update_blocks(SpaDev d, const int32_t * __restrict__ list)
{
  const FrontDesc fd = d.desc[list[blockIdx.x]];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  double * U = d.fronts + fd.off + ns + (int64_t)ns * m;
  for (int c = 16 * (int)blockIdx.y + ((int)threadIdx.x >> 4); c < nu; c += 16 * (int)gridDim.y) {
    for (int i = c + ((int)threadIdx.x & 15); i < nu; i += 16) {U[i + (int64_t)c * m] = 0.0;}
  }
}
void spa_launch_zero_update_blocks(const SpaDev & d, const int32_t * list, int32_t n, int32_t max_m, void * stream)
{
  if (n <= 0) {return;}
  hipLaunchKernelGGL(k_zero_update_blocks, dim3(n, std::max(1, std::min(16, max_m / 16))), dim3(256), 0, (hipStream_t)stream, d, list);
}

// debugging aid (kh_spa_set_debug bit 0): entries of a buffer that are not zero (bit pattern), counted into *count
__global__ __launch_bounds__(256) void k_count_nonzero(const double * __restrict__ p, int64_t n, int32_t * count)
{
  int mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    mine += __double_as_longlong(p[i]) != 0 ? 1 : 0;
  }
  if (mine) {atomicAdd(count, mine);}
}
void spa_launch_count_nonzero(const double * p, int64_t n, int32_t * count, void * stream)
{
  hipLaunchKernelGGL(k_count_nonzero, dim3(1024), dim3(256), 0, (hipStream_t)stream, p, n, count);
}

static void pipeline_attributes()
{
  // (per device: the attribute is kept per device, and solvers of several devices may live in one process)
  const int big = 160 * 1024 - 256;
  static std::atomic<unsigned long long> done[4] = {{0}, {0}, {0}, {0}};
  allow_dynamic_lds(reinterpret_cast<const void *>(k_trsm<32>), big, done[0]);
  allow_dynamic_lds(reinterpret_cast<const void *>(k_trsm<64>), big, done[1]);
  allow_dynamic_lds(reinterpret_cast<const void *>(k_syrk<32>), big, done[2]);
  allow_dynamic_lds(reinterpret_cast<const void *>(k_syrk<64>), big, done[3]);
}

void spa_launch_update_level(const SpaDev & d, int32_t first_front, int32_t n, int32_t max_m, int32_t max_ns, double * rhs, double * upd, void * stream)
{
  if (n <= 0) {return;}
  hipStream_t s = (hipStream_t)stream;
  const int nsp = (max_ns + NB - 1) & ~(NB - 1);
  pipeline_attributes();
  const int max_nu = max_m - 3;       // a front has at least one pivot node; an upper bound is enough for the grid
  if (max_nu <= 0) {return;}
  // slabs / tiles: small enough that a narrow level still spreads over the chip, large enough that a wide one does not
  // drown in workgroups
  const int slabs32 = (max_nu + 31) / 32;
  const bool r64 = (int64_t)n * slabs32 >= 1024;
  if (r64) {
    hipLaunchKernelGGL(k_trsm<64>, dim3(n, (max_nu + 63) / 64), dim3(256), sizeof(double) * ((size_t)64 * (nsp + 2) + nsp + 8 * 64 + 8), s, d, first_front, rhs, upd, nsp);
  } else {
    // a narrow level: eight waves, so that every column block of the pivots has a wave of its own (one round of W loads, not two)
    const int threads = (int64_t)n * slabs32 <= 256 ? 512 : 256;
    hipLaunchKernelGGL(k_trsm<32>, dim3(n, slabs32), dim3(threads), sizeof(double) * ((size_t)32 * (nsp + 2) + nsp + 8 * 32 + 8), s, d, first_front, rhs, upd, nsp);
  }
  const int nt32 = (max_nu + 31) / 32, nt64 = (max_nu + 63) / 64;
  const bool t64 = (int64_t)n * (nt32 * (nt32 + 1) / 2) >= 2048;
  if (t64) {
    hipLaunchKernelGGL(k_syrk<64>, dim3(n, nt64 * (nt64 + 1) / 2), dim3(512), sizeof(double) * ((size_t)2 * 64 * (nsp + 2) + 8), s, d, first_front, nsp);
  } else {
    hipLaunchKernelGGL(k_syrk<32>, dim3(n, nt32 * (nt32 + 1) / 2), dim3(256), sizeof(double) * ((size_t)2 * 32 * (nsp + 2) + 8), s, d, first_front, nsp);
  }
}

void spa_launch_backward3_level(const SpaDev & d, int32_t first_front, int32_t n, int32_t max_m, int32_t max_ns, double * rhs, void * stream)
{
  if (n <= 0) {return;}
  const int nsp = (max_ns + NB - 1) & ~(NB - 1);
  if (n <= 12) {
    hipLaunchKernelGGL(k_backward3<true>, dim3(n), dim3(1024), sizeof(double) * ((size_t)max_m + nsp + 8), (hipStream_t)stream, d, first_front, rhs);
  } else {
    hipLaunchKernelGGL(k_backward3<false>, dim3(n), dim3(max_ns <= 48 ? 256 : 1024), sizeof(double) * ((size_t)max_m + nsp + 8), (hipStream_t)stream, d, first_front, rhs);
  }
}

}  // namespace kh
