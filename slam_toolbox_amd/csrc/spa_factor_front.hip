// K6 of the pose-graph SPA solver (hot path B), the ANY-SIZE route: one workgroup per front of an elimination-tree level.
//
//   k_extend_add   the children's update matrices of a level summed into the fronts, chip-wide
//   k_factor       extend-add of the children (unless k_extend_add has run), blocked right-looking partial Cholesky in pairs of
//                  16-column panels, forward solve fused in
//   k_backward     level-scheduled backward triangular solve
//
// This is what factorises a level whose fronts do not fit the level pipeline's LDS (spa_level_pipeline_fits: more than ~2700 rows;
// the pipeline itself is spa_potrf.hip + spa_update.hip), and what `kh_spa_set_debug` factor modes 1 and 2 (the same thing) select
// so that the tests can lay an independent factorisation beside the pipeline's.  Launchers: spa_launch_extend_add, spa_launch_factor_level,
// spa_launch_backward_level, called by spa_compute.cpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "lds_attr.hpp"
#include "spa_device.hpp"

#pragma clang fp contract(fast)

namespace kh
{

// ---------------------------------------------------------------------------------------------
// K6b: multifrontal partial Cholesky, one workgroup per front.
//
// Blocked right-looking factorisation of the front's first ns columns, panel width NB = 16:
//   (a) 16x16 diagonal block: one wave, lane = row, registers + shuffles
//   (b) panel solve X = A21 L11^-T: one thread per row; X goes back to the front (it is L21) and into
//       an LDS panel (row stride XS = 33 doubles, a pair of panels side by side: conflict-free for the MFMA operand reads)
//   (c) trailing update of the lower triangle, C -= X X^T, in 16x16 tiles on the FP64 matrix cores:
//       4 x v_mfma_f64_16x16x4_f64 per tile with both operands read from the LDS panel.  The MFMA "col"
//       index (lane & 15) is mapped to the front's ROW so that every accumulator load/store of a
//       column-major front is four contiguous 128-byte segments.
// Dynamic LDS: panel of roundup16(m) rows (sized by the host for the largest front of the level).
constexpr int XS = 2 * NB + 1;               // LDS panel row stride: two 16-column panels + 1 (conflict-free MFMA operand reads)

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// 16x16 diagonal block of a panel: lane l owns row l in registers, pivot columns are broadcast with
// v_readlane.  The pivot chain is the serial part of the whole factorisation, so it is kept short:
// 1/sqrt(d) from v_rsq_f64 + two Newton steps (no f64 sqrt / divide expansions), no lane masks (the
// upper-triangle garbage a lane computes is never read by another lane).  Writes L back to the front
// and L plus the reciprocal diagonal (column NB) to the LDS copy `ld`.  Rows/columns >= nb are padded
// with the identity.  Returns true when a pivot is not positive.
__device__ __noinline__ bool factor_diag_block(double * F, int m, int jb, int nb, int lane, double * ld, double * rhs_seg)
{
  double row[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    row[c] = (lane < nb && c < nb && c <= lane) ? F[(jb + lane) + (int64_t)(jb + c) * m] : ((c == lane) ? 1.0 : 0.0);
  }
  bool bad = false;
  double rdiag = 1.0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    double djj = readlane_f64(row[j], j);
    if (!(djj > 0.0)) {bad = true; djj = 1.0;}
    double r = __builtin_amdgcn_rsq(djj);
    const double h = 0.5 * djj;
    r = r * (1.5 - h * r * r);
    r = r * (1.5 - h * r * r);
    row[j] = (lane == j) ? djj * r : row[j] * r;
    if (lane == j) {rdiag = r;}
#pragma unroll
    for (int c = j + 1; c < NB; ++c) {
      const double lcj = readlane_f64(row[j], c);       // L[c][j]
      row[c] -= row[j] * lcj;
    }
  }
  if (lane < NB) {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      ld[lane * (NB + 1) + c] = (c <= lane) ? row[c] : 0.0;
      if (lane < nb && c <= lane) {F[(jb + lane) + (int64_t)(jb + c) * m] = row[c];}
    }
    ld[lane * (NB + 1) + NB] = rdiag;
  }
  // fused forward solve: y = L11^-1 b for this panel's segment of the front's right-hand side (LDS)
  {
    double v = lane < nb ? rhs_seg[lane] : 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double yj = readlane_f64(v, j) * readlane_f64(rdiag, j);
      if (lane == j) {v = yj;} else if (lane > j) {v -= row[j] * yj;}
    }
    if (lane < nb) {rhs_seg[lane] = v;}
  }
  return bad && lane < nb;
}

// Panel solve of one row: x = a L11^-T for the nb (<= 16) columns of the panel; a = gcol[c * m].  x goes
// back to the front and into the row's LDS panel slot (zero padded to 16).  nb = 0: padding row, only
// the zero fill.  `ld` = 16 x 17 LDS copy of L11 with the reciprocal diagonal in column 16.
__device__ __noinline__ void panel_row_solve(double * gcol, int m, int nb, const double * ld, double * xrow,
                                             const double * y, double * rhs_row)
{
  double xr[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {xr[c] = (c < nb) ? gcol[(int64_t)c * m] : 0.0;}
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    // The address of row c of L11 is made to depend (through an opaque zero) on x[c-2]: without it the
    // scheduler issues all 152 LDS reads of the unrolled solve up front (304 VGPRs -> spills); with it
    // at most two rows are in flight, one ahead of the data dependency x[c] <- x[c-1] that serialises
    // the columns anyway.
    int zero = 0;
    if (c >= 2) {asm volatile("v_mov_b32 %0, 0" : "=v"(zero) : "v"(__double2loint(xr[c - 2])));}
    const double * lrow = ld + c * (NB + 1) + zero;
    double v = xr[c];
#pragma unroll
    for (int q = 0; q < c; ++q) {v -= xr[q] * lrow[q];}
    xr[c] = v * lrow[NB];
  }
  double dot = 0.0;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    if (c < nb) {gcol[(int64_t)c * m] = xr[c]; dot += xr[c] * y[c];}
    xrow[c] = xr[c];
  }
  if (nb > 0) {*rhs_row -= dot;}          // fused forward solve: b_i -= L21[i, :] . y
}

constexpr int kMaxLdsRows = 568;           // 568 * 33 * 8 B = 150 KB of the CU's 160 KB LDS

// C -= X X^T on 16x16 tiles of the trailing matrix whose row/column 0 is global row `rb`.  X has KD = 16 or 32
// columns: the LDS panel (row stride XS; columns 16..31 = the second panel of a pair) or, for fronts too large
// for it, the panel columns jb .. jb+KD-1 of the front itself.  thin: only tile column 0 (what the second panel
// of a pair needs before it can be factored); otherwise tile columns >= 1 (thin must have run first), or all
// columns when `all` is set (single panel).
template <bool kLds, int KD>
__device__ __forceinline__ void trailing_update(double * F, const double * Xs, int m, int rb, int jb, int nb_a, int nb_b,
                                                int nrows, int nrows_pad, bool thin, bool all,
                                                int lane, int wave, int nwaves)
{
  constexpr int TU = 4;       // tiles in flight per wave: their accumulator loads are issued together
  const int nt = nrows_pad >> 4;
  const int ntri = all ? nt : nt - 1;             // side of the triangle of tiles walked when not thin
  const int ntiles = thin ? nt : ntri * (ntri + 1) / 2;
  const int shift = (thin || all) ? 0 : 1;
  const int lr = lane & 15, lk = lane >> 4;
  for (int t0 = wave; t0 < ntiles; t0 += nwaves * TU) {
    v4d acc[TU];
    double * cp[TU];
    int tI[TU], tJ[TU];
    bool ok[TU][4];
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const int t = t0 + u * nwaves;
      int I, J;
      if (thin) {
        I = t; J = 0;
      } else {
        I = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
        while (I * (I + 1) / 2 > t) {--I;}
        while ((I + 1) * (I + 2) / 2 <= t) {++I;}
        J = t - I * (I + 1) / 2;
        I += shift; J += shift;
      }
      tI[u] = I; tJ[u] = J;
      const int frow = 16 * I + lr;               // row of the trailing matrix held by this lane
      const int fcol0 = 16 * J + lk;              // its column for accumulator register 0 (+4 per register)
      cp[u] = F + (rb + frow) + (int64_t)(rb + fcol0) * m;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int fc = fcol0 + 4 * r;
        ok[u][r] = t < ntiles && frow < nrows && fc < nrows && fc <= frow;
        acc[u][r] = ok[u][r] ? cp[u][(int64_t)(4 * r) * m] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      if (t0 + u * nwaves >= ntiles) {continue;}       // wave-uniform
      if (kLds) {
        const double * xa = Xs + (16 * tJ[u] + lr) * XS + lk;
        const double * xb = Xs + (16 * tI[u] + lr) * XS + lk;
#pragma unroll
        for (int kk = 0; kk < KD / 4; ++kk) {
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[4 * kk], xb[4 * kk], acc[u], 0, 0, 0);
        }
      } else {
        const int ra = 16 * tJ[u] + lr, rbw = 16 * tI[u] + lr;
#pragma unroll
        for (int kk = 0; kk < KD / 4; ++kk) {
          const int kc = 4 * kk + lk;
          // panel A = columns jb .. jb+15, panel B = jb+16 .. ; B has no rows 0..15 (its own diagonal block)
          const bool kv = kc < 16 ? kc < nb_a : (kc - 16) < nb_b;
          const double a = (ra < nrows && kv && (kc < 16 || ra >= 16)) ? F[(rb + ra) + (int64_t)(jb + kc) * m] : 0.0;
          const double b = (rbw < nrows && kv && (kc < 16 || rbw >= 16)) ? F[(rb + rbw) + (int64_t)(jb + kc) * m] : 0.0;
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a, b, acc[u], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < TU; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (ok[u][r]) {cp[u][(int64_t)(4 * r) * m] = acc[u][r];}
      }
    }
  }
}

// Extend-add of a whole level, chip-wide: workgroup (front, block of 16 destination columns).  Inside k_factor the sums
// of a 456-row front's two children took one CU 65 us per level -- a quarter of the level on the narrow upper levels,
// where most of the chip idles.  A child's struct rows map to INCREASING positions in the parent (both are in
// elimination order), so the child columns that land in this workgroup's destination block are one contiguous range;
// every entry of the block is summed by this workgroup alone, children in turn: no atomics, the same order every run.
__global__ __launch_bounds__(1024) void k_extend_add(SpaDev d, const int32_t * __restrict__ level_fronts)
{
  const int nw = (int)blockDim.x >> 6;
  const int k = level_fronts[blockIdx.x];
  const int m = d.front_m[k];
  const int c_lo = 16 * (int)blockIdx.y, c_hi = min(m, c_lo + 16);
  if (c_lo >= m) {return;}
  double * F = d.fronts + d.front_off[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int32_t s_rp[2048];            // the child's struct rows' block positions in this front (m <= 8000 -> < 2667 blocks)
  // the children's descriptors first, all at once: fetched one child after the other they are a chain of six dependent
  // memory latencies per child, which was most of this kernel's 30 us
  constexpr int kBatch = 8;
  const int ci0 = d.child_ptr[k], ci1 = d.child_ptr[k + 1];
  for (int cb = ci0; cb < ci1; cb += kBatch) {
  int cid[kBatch], cm[kBatch], cns[kBatch], crp[kBatch];
  long long coff[kBatch];
#pragma unroll
  for (int q = 0; q < kBatch; ++q) {cid[q] = cb + q < ci1 ? d.child_list[cb + q] : -1;}
#pragma unroll
  for (int q = 0; q < kBatch; ++q) {
    const int c = cid[q] < 0 ? 0 : cid[q];
    cm[q] = d.front_m[c]; cns[q] = d.front_ns[c]; coff[q] = d.front_off[c]; crp[q] = d.relpos_ptr[c];
  }
#pragma unroll
  for (int q = 0; q < kBatch; ++q) {
    if (cid[q] < 0) {continue;}
    const int mc = cm[q], nsc = cns[q], nuc = mc - nsc;
    const double * Uc = d.fronts + coff[q] + nsc + (int64_t)nsc * mc;
    const int32_t * rp = d.relpos + crp[q];
    const int nblk = nuc / 3;
    const bool staged = nblk <= 2048;       // staged in LDS: the two bisections below are chains of dependent reads
    if (staged) {for (int i = threadIdx.x; i < nblk; i += blockDim.x) {s_rp[i] = rp[i];}}
    __syncthreads();
    auto pos = [&](int a) {return 3 * (staged ? s_rp[a / 3] : rp[a / 3]) + a % 3;};
    // first child column with pos >= c_lo, first with pos >= c_hi
    int lo = 0, hi = nuc;
    while (lo < hi) {const int mid = (lo + hi) >> 1; if (pos(mid) < c_lo) {lo = mid + 1;} else {hi = mid;}}
    const int b_lo = lo;
    hi = nuc;
    while (lo < hi) {const int mid = (lo + hi) >> 1; if (pos(mid) < c_hi) {lo = mid + 1;} else {hi = mid;}}
    const int b_hi = lo;
    for (int b = b_lo + wave; b < b_hi; b += nw) {
      double * dst = F + (int64_t)pos(b) * m;
      const double * src = Uc + (int64_t)b * mc;
      for (int a0 = b; a0 < nuc; a0 += 256) {
        // four rows per lane in flight: unconditional loads at a clamped row (as `a < nuc ? load : 0` every load sat in a branch
        // of its own with a wait behind it: twelve dependent round trips per 256 rows where two do)
        double u[4], f[4];
        int pa[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ac = min(a0 + lane + 64 * q, nuc - 1);
          pa[q] = pos(ac);
          u[q] = src[ac];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {f[q] = dst[pa[q]];}
#pragma unroll
        for (int q = 0; q < 4; ++q) {if (a0 + lane + 64 * q < nuc) {dst[pa[q]] = f[q] + u[q];}}
      }
    }
    __syncthreads();       // the next child may add into the same entries (and restages s_rp)
  }
  }
}

void spa_launch_extend_add(const SpaDev & d, const int32_t * level_fronts, int32_t n, int32_t max_m, void * stream)
{
  if (n <= 0) {return;}
  // one wave per destination column of the block of 16 (with four waves a workgroup walked its columns four at a time, each
  // walk a round trip to memory); wide levels keep the small workgroups
  const int threads = (int64_t)n * ((max_m + 15) / 16) > 512 ? 256 : 1024;
  hipLaunchKernelGGL(k_extend_add, dim3(n, (max_m + 15) / 16), dim3(threads), 0, (hipStream_t)stream, d, level_fronts);
}

// The any-size factorisation of one level: one workgroup per front (blockIdx.x = the front's slot in level_fronts), no
// hand-offs between workgroups.  The workgroup extend-adds the children (their forward-solve contributions always, their
// update matrices unless k_extend_add has done that: matrix_added), then runs the blocked right-looking partial Cholesky
// of the front's ns pivot columns with the forward solve fused in.  Fronts of up to kMaxLdsRows rows keep the solved
// panel pair in LDS (lds_rows rows of XS doubles); larger ones read it back from the front itself.
__global__ __launch_bounds__(1024) void k_factor(SpaDev d, const int32_t * __restrict__ level_fronts, int32_t * fail_flag,
              double * rhs, double * upd, int lds_rows, int matrix_added)
{
  const int k = level_fronts[blockIdx.x];
  const int m = d.front_m[k], ns = d.front_ns[k];
  double * F = d.fronts + d.front_off[k];
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
  extern __shared__ double smem[];
  double * Xs = smem;                       // [rows below the first panel of a pair, padded to 16][XS]
  const bool use_lds = m <= kMaxLdsRows;    // larger fronts read the panel back from the front itself (L2)
  __shared__ double Ld[NB][NB + 1];
  __shared__ int s_fail;
  // Fused forward solve (K6c, first half): the front's slice of the right-hand side lives in LDS next to the
  // panel -- pivots from rhs (elimination order), struct rows accumulate the children's contributions -- and
  // every panel applies y = L11^-1 b, b_below -= L21 y while L11 and L21 are still on chip.
  double * sb = use_lds ? smem + (size_t)lds_rows * XS : smem;
  const int first = 3 * d.front_first[k];
  for (int t = tid; t < m; t += nthreads) {sb[t] = t < ns ? rhs[first + t] : 0.0;}
  __syncthreads();

  // 1. extend-add the children's update matrices (lower triangles).  Children are taken one after the
  //    other (two children may add into the same entry); within a child every wave takes columns
  //    four at a time with all loads issued before the first add, so the pass is bound by bandwidth and
  //    not by a chain of dependent L2 round trips.  The scalar row positions inside this front
  //    (3 * relpos + component) are staged in LDS once per child.
  int * pos = use_lds ? reinterpret_cast<int *>(smem) : reinterpret_cast<int *>(smem + m);
  for (int ci = d.child_ptr[k]; ci < d.child_ptr[k + 1]; ++ci) {
    const int c = d.child_list[ci];
    const int mc = d.front_m[c], nsc = d.front_ns[c], nuc = mc - nsc;
    const double * Uc = d.fronts + d.front_off[c] + nsc + (int64_t)nsc * mc;
    const int32_t * rp = d.relpos + d.relpos_ptr[c];
    for (int a = tid; a < nuc; a += nthreads) {pos[a] = 3 * rp[a / 3] + a % 3;}
    __syncthreads();
    const double * uc = upd + 3 * (int64_t)d.front_rows_ptr[c];        // the child's forward-solve contribution
    for (int a = tid; a < nuc; a += nthreads) {sb[pos[a]] += uc[a];}
    constexpr int CB = 8;
    // matrix_added: k_extend_add has already summed the children's update matrices into the front, chip-wide
    for (int b0 = wave * CB; b0 < nuc && !matrix_added; b0 += nwaves * CB) {
      for (int a0 = b0; a0 < nuc; a0 += 64) {
        const int a = a0 + lane;
        double u[CB], f[CB];
        double * dst[CB];
        bool on[CB];
        const int pa = a < nuc ? pos[a] : 0;
#pragma unroll
        for (int q = 0; q < CB; ++q) {
          const int b = b0 + q;
          on[q] = a < nuc && b < nuc && a >= b;
          dst[q] = F + pa + (int64_t)(on[q] ? pos[b] : 0) * m;
          u[q] = on[q] ? Uc[a + (int64_t)b * mc] : 0.0;
          f[q] = on[q] ? *dst[q] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < CB; ++q) {if (on[q]) {*dst[q] = f[q] + u[q];}}
      }
    }
    __syncthreads();
  }

  // 2. blocked right-looking partial Cholesky of the first ns columns
  if (tid == 0) {s_fail = 0;}
  __syncthreads();
  // Panels are taken in pairs with a delayed update: after panel A only the next 16 columns of the trailing
  // matrix are updated (thin), panel B is factored, and then BOTH panels are applied to the rest in one pass
  // with K = 32 -- half as many sweeps over the trailing matrix, twice the flops per accumulator load/store.
  auto panel = [&](int jb, int nb, int rb, double * xcols) {
    // (a) diagonal block: wave 0
    if (wave == 0) {
      if (factor_diag_block(F, m, jb, nb, lane, &Ld[0][0], sb + jb)) {s_fail = 1;}
    }
    __syncthreads();
    // (b) panel: X = F[rows, jb:jb+nb] * Ld^{-T}, rows below the diagonal block; one thread per row (out of
    //     line, see panel_row_solve); fronts too large for the LDS panel solve in place in the front instead
    const int r0 = jb + nb;
    const int nrows = m - r0;
    const int nrows_pad = (nrows + 15) & ~15;
#pragma unroll 1
    for (int i = tid; i < nrows_pad; i += nthreads) {
      double * gcol = F + (r0 + i) + (int64_t)jb * m;       // F[r0 + i][jb + c] = gcol[c * m]
      if (use_lds) {
        panel_row_solve(gcol, m, i < nrows ? nb : 0, &Ld[0][0], xcols + (size_t)(r0 - rb + i) * XS, sb + jb,
                        sb + min(r0 + i, m - 1));
      } else if (i < nrows) {
        double dot = 0.0;
#pragma unroll 1
        for (int c = 0; c < nb; ++c) {
          const double * lrow = &Ld[c][0];
          double v = gcol[(int64_t)c * m];
#pragma unroll 4
          for (int q = 0; q < c; ++q) {v -= gcol[(int64_t)q * m] * lrow[q];}
          v *= lrow[NB];
          gcol[(int64_t)c * m] = v;
          dot += v * sb[jb + c];
        }
        sb[r0 + i] -= dot;
      }
    }
    __syncthreads();
  };
  for (int jb = 0; jb < ns; ) {
    const int nb_a = min(NB, ns - jb);
    const int rb = jb + nb_a;                 // first row / column of the trailing matrix of this pair
    const int nrows = m - rb;
    const int nrows_pad = (nrows + 15) & ~15;
    // only two FULL panels pair up: the thin update covers exactly the 16 columns of the second panel, so a
    // partial second panel would leave the non-pivot columns of that tile column without its contribution
    const bool pair = jb + 2 * NB <= ns;
    if (use_lds) {
      // the second panel has no rows 0..15 (they are its diagonal block): zero that corner once per pair
      for (int t = tid; t < 16 * NB; t += nthreads) {Xs[(t >> 4) * XS + NB + (t & 15)] = 0.0;}
    }
    panel(jb, nb_a, rb, Xs);
    if (!pair) {
      if (use_lds) {
        trailing_update<true, 16>(F, Xs, m, rb, jb, nb_a, 0, nrows, nrows_pad, false, true, lane, wave, nwaves);
      } else {
        trailing_update<false, 16>(F, Xs, m, rb, jb, nb_a, 0, nrows, nrows_pad, false, true, lane, wave, nwaves);
      }
      __syncthreads();
      jb += NB;
      continue;
    }
    if (use_lds) {
      trailing_update<true, 16>(F, Xs, m, rb, jb, nb_a, 0, nrows, nrows_pad, true, false, lane, wave, nwaves);
    } else {
      trailing_update<false, 16>(F, Xs, m, rb, jb, nb_a, 0, nrows, nrows_pad, true, false, lane, wave, nwaves);
    }
    __syncthreads();
    const int nb_b = NB;
    panel(jb + NB, nb_b, rb, Xs + NB);
    if (use_lds) {
      trailing_update<true, 32>(F, Xs, m, rb, jb, nb_a, nb_b, nrows, nrows_pad, false, false, lane, wave, nwaves);
    } else {
      trailing_update<false, 32>(F, Xs, m, rb, jb, nb_a, nb_b, nrows, nrows_pad, false, false, lane, wave, nwaves);
    }
    __syncthreads();
    jb += 2 * NB;
  }
  // forward-solve results: y of the pivots back to rhs, the struct rows' partial sums to this front's slot
  for (int t = tid; t < ns; t += nthreads) {rhs[first + t] = sb[t];}
  {
    double * uk = upd + 3 * (int64_t)d.front_rows_ptr[k];
    for (int q = tid; q < m - ns; q += nthreads) {uk[q] = sb[ns + q];}
  }
  if (tid == 0 && s_fail) {atomicExch(fail_flag, 1);}
}


void spa_launch_factor_level(const SpaDev & d, const int32_t * level_fronts, int32_t n, int32_t max_m, int32_t * fail_flag,
                             double * rhs, double * upd, int32_t matrix_added, void * stream)
{
  if (n <= 0) {return;}
  const int threads = max_m <= 96 ? 256 : (max_m <= 192 ? 512 : 1024);
  const int lds_rows = ((max_m < kMaxLdsRows ? max_m : kMaxLdsRows) + 15) & ~15;
  // panel + the front's right-hand side behind it; fronts beyond the LDS panel keep only the rhs (+ the
  // extend-add position table) in LDS
  const int small_m = max_m < kMaxLdsRows ? max_m : kMaxLdsRows;
  const size_t lds = sizeof(double) * std::max((size_t)lds_rows * XS + small_m, (size_t)max_m + (max_m + 1) / 2 + 8);
  static std::atomic<unsigned long long> attr_done{0};
  allow_dynamic_lds(reinterpret_cast<const void *>(k_factor), (int)(sizeof(double) * ((size_t)kMaxLdsRows * XS + kMaxLdsRows + 16)), attr_done);
  hipLaunchKernelGGL(k_factor, dim3(n), dim3(threads), lds, (hipStream_t)stream, d, level_fronts, fail_flag, rhs, upd, lds_rows,
                     (int)matrix_added);
}

// ---------------------------------------------------------------------------------------------
// K6c: backward triangular solve, one workgroup (256 threads) per front, blocked by 16 like the
// factorisation (the forward solve is fused into k_factor: a front gathers its children's contributions --
// upd, one segment per front = its struct rows -- instead of scattering with atomics, so the solve is
// bit-reproducible).  rhs is in elimination order.  Dynamic LDS: m doubles.
__device__ __forceinline__ void load_diag_block(const double * F, int m, int jb, int nb, int lane, double (&col)[NB])
{
  // lane c holds column c of the 16x16 diagonal block: col[j] = L[jb+j][jb+c] (j >= c)
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    col[j] = (lane < nb && j < nb && j >= lane) ? F[(jb + j) + (int64_t)(jb + lane) * m] : ((j == lane) ? 1.0 : 0.0);
  }
}

// 1024 threads: the 16 columns of a block take their dot products at once (one wave each) instead of in four rounds --
// the sweep is a chain of (dot, 16 x 16 back substitution) steps, each a memory latency long, so the rounds were the time
__global__ __launch_bounds__(1024) void k_backward(SpaDev d, const int32_t * __restrict__ level_fronts, double * rhs)
{
  const int k = level_fronts[blockIdx.x];
  const int m = d.front_m[k], ns = d.front_ns[k], nu = m - ns;
  const double * F = d.fronts + d.front_off[k];
  const int first = 3 * d.front_first[k];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
  extern __shared__ double sb[];
  const int32_t * rows = d.front_rows + d.front_rows_ptr[k];
  for (int t = tid; t < ns; t += nthreads) {sb[t] = rhs[first + t];}
  for (int q = tid; q < nu; q += nthreads) {sb[ns + q] = rhs[3 * rows[q / 3] + q % 3];}
  __syncthreads();
  const int nblk = (ns + NB - 1) / NB;
  for (int blk = nblk - 1; blk >= 0; --blk) {
    const int jb = blk * NB;
    const int nb = min(NB, ns - jb);
    const int r0 = jb + nb;
    // w[t] = y[t] - sum_{i >= r0} L[i][t] x[i] : one wave per column, lanes over the rows
    for (int c = wave; c < nb; c += nwaves) {
      const double * col = F + (int64_t)(jb + c) * m;
      double acc = 0.0;
      for (int i = r0 + lane; i < m; i += 64) {acc += col[i] * sb[i];}
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {acc += __shfl_xor(acc, s);}
      if (lane == 0) {sb[jb + c] -= acc;}
    }
    __syncthreads();
    if (wave == 0) {
      double col[NB];
      load_diag_block(F, m, jb, nb, lane, col);
      double v = lane < nb ? sb[jb + lane] : 0.0;
#pragma unroll
      for (int j = NB - 1; j >= 0; --j) {
        const double xj = readlane_f64(v, j) / readlane_f64(col[j], j);   // lane j: col[j] = L[jb+j][jb+j]
        if (lane == j) {v = xj;} else if (lane < j) {v -= col[j] * xj;}    // lane c < j: col[j] = L[jb+j][jb+c]
      }
      if (lane < nb) {sb[jb + lane] = v;}
    }
    __syncthreads();
  }
  for (int t = tid; t < ns; t += nthreads) {rhs[first + t] = sb[t];}
}

void spa_launch_backward_level(const SpaDev & d, const int32_t * level_fronts, int32_t n, int32_t max_m, double * rhs, void * stream)
{
  if (n <= 0) {return;}
  hipLaunchKernelGGL(k_backward, dim3(n), dim3(1024), sizeof(double) * max_m, (hipStream_t)stream, d, level_fronts, rhs);
}

}  // namespace kh
