// The 16 x 16 diagonal block of k_potrf (spa_potrf.hip): Cholesky of the block and L^-T in the same sweep, one wave, on the matrix
// cores.  A header of its own because tools/diag_probe.hip times exactly this code against the round-3 pivot chain it replaced
// (tools/diag_chain_round3.hpp); nothing else includes it.  KH_DIAG_STAMPS (the probe's -DSTAMPS) adds shader-clock stamps.
#pragma once
#include "spa_device.hpp"

#pragma clang fp contract(fast)

namespace kh
{

constexpr int XDS = NB + 2;                // row stride of the 16 x 16 inverse of a diagonal block in LDS

// ---- the diagonal block on the matrix cores, four pivots at a time (round 6) ----
// The round-3 pivot chain (16 x 16 Cholesky in the registers of lanes 0..15, pivot columns broadcast lane to lane) issues ~670
// double-precision instructions for 16 pivots on a wave of which a quarter of the lanes work
// (3.2 us, measured: the floor under every level of the factorisation).  Here the 16 x 16 tile never leaves the accumulator
// layout of v_mfma_f64_16x16x4 -- lane (lr, lk) holds M[lr][lk + 4 r] in register r, i.e. register p IS column block p and
// its entry is exactly what the lane has to supply, as the A and as the B operand, for the rank-4 update of the columns
// behind block p:
//   gather   the 4 x 4 diagonal block of column block p: one ds_write of register p (64 doubles of scratch), ten uniform reads
//   chol4    its Cholesky factor and T = L_pp^-T in uniform registers (every lane the same ~60 operations)
//   panel    M[:, 4p .. 4p+3] <- M[:, 4p .. 4p+3] T   ONE MFMA: b = register p, a = T[lk][lr - 4p] on the lanes lr of block p
//   update   M[:, behind] -= panel panel^T             ONE MFMA: a = b = the new register p
// and the identity that rides along (E -> L^-T) takes the same two MFMAs with its own register p as b.  Entries above the
// diagonal hold garbage that stays in registers nobody reads (rows above block p only feed rows above block p); the rows
// of the diagonal block itself come out of `chol4`, not of the panel product.  ~700 clocks per four pivots.
// One over the square root to full double precision: v_rsq_f64 is good to ~2^-26 or better (tools/diag_probe.hip prints its
// worst error), so one THIRD-order step r (1 + e/2 + 3 e^2/8), e = 1 - d r^2, lands below 2^-70: five dependent operations
// where two Newton steps take seven.
__device__ __forceinline__ double rsqrt_full(double d)
{
  const double r = __builtin_amdgcn_rsq(d);
  const double e = __builtin_fma(-d * r, r, 1.0);
  const double c = __builtin_fma(e, 0.375, 0.5) * e;
  return __builtin_fma(r, c, r);
}

// T = L^-T of the 4 x 4 block a (a[i][j], j <= i), as v = L^-1 (lower): the factor itself is not formed -- nobody reads the
// diagonal tile's L (the panel product leaves the rows below it, and every consumer of the pivot block works with L^-T).
// A pivot that is not positive is reported; its reciprocal square root (NaN or infinite) flows on, the factorisation has failed
// and every number behind it is flagged by the caller's fail word.  `mid` runs after the second pivot: the place where the
// caller parks matrix-core work that must not sit between the pivots' dependent operations and their issue slots.
template <typename Mid>
__device__ __forceinline__ bool chol4_inverse(double (&m)[4][4], double (&v)[4][4], Mid mid)
{
  double r[4], l[4][4];
  double dmin = m[0][0];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j == 2) {mid();}
    dmin = fmin(dmin, m[j][j]);
    r[j] = rsqrt_full(m[j][j]);
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {l[i][j] = m[i][j] * r[j];}
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
#pragma unroll
      for (int c = j + 1; c <= i; ++c) {m[i][c] -= l[i][j] * l[c][j];}
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i][i] = r[i];
#pragma unroll
    for (int j = i - 1; j >= 0; --j) {
      double acc = l[i][j] * v[j][j];
#pragma unroll
      for (int k = j + 1; k < i; ++k) {acc += l[i][k] * v[k][j];}
      v[i][j] = -acc * r[i];
    }
  }
  return dmin > 0.0;
}

// tile: the diagonal tile in accumulator layout (lower part meaningful, identity on the padding).  Outputs: the strictly upper
// part of L^-T over the strictly upper part of blk (row stride LD; the lower triangle of blk, L itself, is left alone), all of
// L^-T to xd (16 x XDS), the reciprocal pivots (= diagonal of L^-T) to rdv.  sc: 64 doubles of LDS scratch owned by this wave.
// The identity's two matrix-core operations of block p are issued inside block p + 1 -- the panel product while the next
// block's gather is on its way through LDS, the update between its second and third pivot -- so that the matrix pipe is free
// when the tile's own panel and update arrive: those two are the only ones the next pivot waits for.
#ifdef KH_DIAG_STAMPS
#define DSTAMP(i, v) do { asm volatile("s_nop 0" : "+v"(v)); long long t_; asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
  asm volatile("s_nop 0" : "+v"(v)); g_dstamp[i] = t_; } while (0)
__device__ long long g_dstamp[32];
#else
#define DSTAMP(i, v) do {} while (0)
#endif
__device__ __forceinline__ bool potrf_diag_mfma(v4d tile, double * blk, int LD, int lane, double * xd, double * rdv, double * sc)
{
  const int lr = lane & 15, lk = lane >> 4;
  const int c4 = lr & 3, b4 = lr >> 2;
  v4d E;
#pragma unroll
  for (int r = 0; r < 4; ++r) {E[r] = (lk + 4 * r == lr) ? 1.0 : 0.0;}
  bool bad = false;
  const v4d zero = v4d{0.0, 0.0, 0.0, 0.0};
  double ta_prev = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // gather the diagonal 4 x 4 block: sc[lr + 16 lk] = M[lr][4 p + lk]
    DSTAMP(5 * p + 0, tile[p]);
    sc[lane] = tile[p];
    v4d en = zero;
    if (p > 0) {en = __builtin_amdgcn_mfma_f64_16x16x4f64(ta_prev, E[p - 1], zero, 0, 0, 0);}
    double a[4][4], v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {a[i][j] = sc[(4 * p + i) + 16 * j];}
    }
    DSTAMP(5 * p + 1, a[3][3]);
    __builtin_amdgcn_sched_barrier(0);
    const bool ok = chol4_inverse(a, v, [&]() {
      __builtin_amdgcn_sched_barrier(0);
      if (p > 0) {
        E[p - 1] = en[p - 1];
        const v4d eu = __builtin_amdgcn_mfma_f64_16x16x4f64(-tile[p - 1], E[p - 1], E, 0, 0, 0);
#pragma unroll
        for (int r = p; r < 4; ++r) {E[r] = eu[r];}
      }
    });
    if (!ok) {bad = true;}
    DSTAMP(5 * p + 2, v[3][0]);
    // T[k][c] = v[c][k] on lane (lr = 4 p + c, lk = k), zero elsewhere
    double tsel = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int k = 0; k <= c; ++k) {tsel = (c4 == c && lk == k) ? v[c][k] : tsel;}
    }
    double ta = (b4 == p) ? tsel : 0.0;
    DSTAMP(5 * p + 3, ta);
    const v4d pn = __builtin_amdgcn_mfma_f64_16x16x4f64(ta, tile[p], zero, 0, 0, 0);
    tile[p] = pn[p];
    DSTAMP(5 * p + 4, tile[p]);
    if (p < 3) {
      const v4d tu = __builtin_amdgcn_mfma_f64_16x16x4f64(-tile[p], tile[p], tile, 0, 0, 0);
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {tile[r] = tu[r];}
    }
    ta_prev = ta;
    __builtin_amdgcn_sched_barrier(0);
  }
  {
    const v4d en = __builtin_amdgcn_mfma_f64_16x16x4f64(ta_prev, E[3], zero, 0, 0, 0);
    E[3] = en[3];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = lk + 4 * r;
    if (c > lr) {blk[lr * LD + c] = E[r];}
    xd[lr * XDS + c] = E[r];
    if (c == lr) {rdv[lr] = E[r];}
  }
  return bad;
}

}  // namespace kh
