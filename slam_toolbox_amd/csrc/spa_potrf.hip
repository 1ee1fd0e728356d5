// K6 of the pose-graph SPA solver (hot path B), the LEVEL PIPELINE, first stage: k_potrf, the pivot block of every front of a
// level.  The other stages (k_trsm, k_syrk, k_front_update, k_backward3) are spa_update.hip's; the 16 x 16 diagonal block is
// spa_diag_block.hpp's.  Launcher: spa_launch_potrf_level, and spa_level_pipeline_fits (the LDS budgets of the whole pipeline),
// both called by spa_compute.cpp.  KH_SPA_TIMING in the environment prints shader-clock stamps of the first front of every launch.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "lds_attr.hpp"
#include "spa_device.hpp"
#include "spa_diag_block.hpp"

#pragma clang fp contract(fast)

namespace kh
{

// =============================================================================================
// K6, round 3: the level pipeline  potrf -> trsm -> syrk  (one launch each per level of the assembly tree).
//
// The panel-pair kernel of the any-size route (k_factor, spa_factor_front.hip) keeps a front on ONE compute unit from its first
// pivot to its last: the pivot chain, the
// row solves and the K = 32 updates of all its panel pairs run back to back, and on the upper levels of the tree -- a
// handful of fronts with 100+ pivots and 300-400 rows each -- 250 of the 256 CUs idle while those few grind through 6-7
// pairs (rocprof, round 2: 34 + 24 launches of that round's two panel-pair kernels = 1.8 ms per factorisation at 0.5 TFLOP/s).  The
// only inherently serial part of a front is the Cholesky of its ns x ns pivot block; everything else is matrix products:
//   potrf  one workgroup per front: F11 = L11 L11^T inside LDS (ns <= 128: the symbolic analysis splits larger
//          supernodes into chains), and in the SAME sweep W = L11^-T: the identity rides along as extra rows of the panel
//          (x L11^T = e_i, solved block column by block column like every other row), stored in the unused upper triangle
//          of the LDS matrix.  The 16 x 16 inverse of a diagonal block comes out of the block's own factorisation the same
//          way (potrf_diag_mfma), so every row solve of the panel is a 16 x 16 x 16 MFMA
//          product instead of a substitution.  y1 = L11^-1 b1 (forward solve) is one product with W^T.
//   trsm   L21 = F21 W, a plain GEMM over row slabs of every front of the level (chip-wide), fused with the forward-solve
//          contribution  b2 -= L21 y1.
//   syrk   F22 -= L21 L21^T over 32 x 32 / 64 x 64 tiles of every front of the level (chip-wide).
// With W the backward solve of a level is two matrix-vector products (k_backward3) instead of a chain of 16 x 16
// substitutions, each a memory latency long.  Fronts are numbered level by level, so a workgroup finds its front at
// first_front + blockIdx.x and everything it needs to know about it in ONE 128-byte descriptor (FrontDesc): on this problem size a
// dependent global load is about a microsecond, and a chain of four index look-ups was a third of a small kernel's time.

// row "solve" of one 16-row tile: T <- T Dinv^T  (Dinv^T = L_jj^-T in xd), in place, one wave
__device__ __forceinline__ v4d potrf_rowsolve_tile(double * tile, int LD, const double * xd, int lane)
{
  const int lr = lane & 15, lk = lane >> 4;
  const double * tb = tile + lr * LD + 4 * lk;         // b: T[lr][k]
  const double * xa = xd + 4 * lk * XDS + lr;          // a: (L^-T)[k][lr]
  double b[4], a[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {b[kk] = tb[kk]; a[kk] = xa[kk * XDS];}
  v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);}
  double * cp = tile + lr * LD + lk;
#pragma unroll
  for (int r = 0; r < 4; ++r) {cp[4 * r] = acc[r];}
  return acc;
}

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains the vector-memory counter, and k_potrf's waves
// keep the NEXT step's tile loads in flight across a step -- with the full barrier every step ended by sitting out a memory
// latency (1-2 us of a 3 us step)
__device__ __forceinline__ void lds_barrier() {asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");}

// KH_SPA_TIMING: shader-clock stamps of workgroup 0's thread 0, kept in LDS (behind the kernel's own dynamic LDS) and written out by
// the kernel's last statement -- stamps stored straight to host memory put a PCIe round trip into the next vector-memory wait
#define PSTAMP() do { if (tbuf && blockIdx.x == 0 && threadIdx.x == 0 && tcount < 60) {stamps[tcount++] = clock64();} } while (0)

// Initial value of the 16 x 16 tile (rows row0.., columns col0..) of the pivot block in MFMA accumulator layout: the
// front's own (assembled) entries plus the children's update matrices; identity on the padding; entries above the
// diagonal are not meaningful.  In two halves: pivot_tile_load only REQUESTS the front's entries (nothing in it touches a
// loaded value, so the wave goes on to its pivot chain while they travel -- with the padding select next to the loads, as in
// round 3, the wave sat out a full memory latency, about a microsecond, in front of every diagonal block);
// pivot_tile_finish, one step later, adds the children's entries (gather mode only) and puts the identity on the padding.
struct TileRaw {v4d a, b;};
__device__ __forceinline__ TileRaw pivot_tile_load(const FrontDesc & fd, const double * F, const double * B, bool clean, int row0, int col0, int lane)
{
  const int lr = lane & 15, lk = lane >> 4;
  const int row = row0 + lr, m = fd.m, ns = fd.ns;
  TileRaw t;
  t.b = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int col = col0 + lk + 4 * r;
    const bool want = row < ns && col <= row;
    const int64_t at = want ? row + (int64_t)col * m : 0;
    t.a[r] = F[at];
    if (B) {t.b[r] = B[at];}
    // self-cleaning fronts (round 6): what has been read is zero again for the next factorisation -- no 2 x 190 MB memset per
    // factorisation (L11 itself lives in LDS and leaves the kernel as W)
    if (clean && want) {
      const_cast<double *>(F)[at] = 0.0;
      if (B) {const_cast<double *>(B)[at] = 0.0;}
    }
  }
  return t;
}

__device__ __forceinline__ v4d pivot_tile_finish(const TileRaw & t, const SpaDev & d, const FrontDesc & fd, int nchild, int row0, int col0, int lane)
{
  v4d v = t.a + t.b;
  const int lr = lane & 15, lk = lane >> 4;
  const int row = row0 + lr, m = fd.m, ns = fd.ns, mp = m / 3;
  bool want[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int col = col0 + lk + 4 * r;
    want[r] = row < ns && col <= row;
  }
  for (int s = 0; s < nchild; ++s) {
    const ChildInfo c = child_info(d, fd, s);
    const int32_t * inv = d.cinv + fd.cinv_ptr + s * mp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = col0 + lk + 4 * r;
      const double g = gather_entry(d.fronts, c, inv, want[r] ? row : 0, want[r] ? col : 0);
      v[r] += want[r] ? g : 0.0;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int col = col0 + lk + 4 * r;
    v[r] = want[r] ? v[r] : ((row == col) ? 1.0 : 0.0);
  }
  return v;
}

// acc -= B A^T over the column blocks [p_lo, p_hi) of the LDS matrix X (row stride LD):  A = rows arow0.., B = rows brow0..
__device__ __forceinline__ void ll_accumulate(v4d & acc, const double * X, int LD, int arow0, int brow0, int p_lo, int p_hi, int lane)
{
  const int lr = lane & 15, lk = lane >> 4;
  const double * xa = X + (arow0 + lr) * LD + 4 * lk;
  const double * xb = X + (brow0 + lr) * LD + 4 * lk;
  // two column blocks at a time into two accumulators: a product is a chain of four DEPENDENT matrix-core operations (81 clocks
  // each, 64 of pipe), and a helper wave of k_potrf has up to six of them in a row per tile
  v4d other = v4d{0.0, 0.0, 0.0, 0.0};
  int p = p_lo;
  for (; p + 1 < p_hi; p += 2) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[NB * p + kk], xb[NB * p + kk], acc, 0, 0, 0);
      other = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[NB * (p + 1) + kk], xb[NB * (p + 1) + kk], other, 0, 0, 0);
    }
  }
  if (p < p_hi) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[NB * p + kk], xb[NB * p + kk], acc, 0, 0, 0);}
  }
  acc += other;
}

// Pivot block of every front of a level, LEFT-LOOKING, 512 threads (= 8 waves) per front.  Step jb (16 columns):
//   U  the tiles of column block jb get their final values: initial value (regular tiles: the front's entries + the
//      children's, requested one step ahead; identity rows: zero) minus the products with every earlier column block.
//      Wave 0 owns the DIAGONAL tile and its pivot chain (potrf_diag_mfma, with L_jj^-T riding along): the critical path of
//      the kernel.  Everything else belongs to the seven helper waves, dealt out task by task: the regular tiles (I, jb), the
//      identity-row tiles, block jb - 1 of W = L11^-T on its way to memory, the first term of the identity rows of block jb - 1
//      (the one that needs L_(jb-1)(jb-1)^-T, which only lives for one step) -- and the LOOK-AHEAD: the products of the NEXT
//      diagonal tile with the column blocks before jb, so that wave 0 opens step jb + 1 with one product instead of jb + 1.
//   R  row solves: every tile of the column times L_jj^-T (MFMA), one tile per wave.
// LDS holds only SOLVED tiles: L11 in the lower triangle, L11^-T strictly above it.
// Round 6: with four waves (round 3) every wave ran its tiles' products one after the other, each a chain of dependent
// v_mfma_f64_16x16x4 (81 clocks apiece, measured): on a 126-pivot front the three helper waves took 5-6 us per step, three
// times the pivot chain they were meant to hide behind (the kernel ran as long WITHOUT the chain).  The barriers of a step
// order LDS traffic only (lds_barrier): the next step's tile requests and the stores of W stay in flight across them.
constexpr int kPotrfThreads = 512, kPotrfHelpers = kPotrfThreads / 64 - 1;
__device__ __forceinline__ void potrf_body(const SpaDev & d, const FrontDesc & fd, int32_t * fail_flag, double * rhs, double * upd, int lds_nsp,
                                           long long * tbuf, int stamp_off)
{
  int tcount = 0;
  extern __shared__ double smem[];
  long long * stamps = reinterpret_cast<long long *>(smem) + stamp_off;
  PSTAMP();
  const int m = fd.m, ns = fd.ns;
  const int nsp = (ns + NB - 1) & ~(NB - 1), nt = nsp >> 4, LD = nsp + 2;
  const double * F = d.fronts + fd.off;
  double * W = d.winv + fd.woff;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  double * X = smem;                                               // [nsp][LD]: lower = L11, strictly upper = L11^-T
  double * rd = smem + (size_t)lds_nsp * (lds_nsp + 2);            // [lds_nsp] reciprocal diagonal of L11 = diagonal of L11^-T
  double * yv = rd + lds_nsp;                                      // [lds_nsp] y1
  double * Xd = yv + lds_nsp;                                      // [2][16][XDS] L_jj^-T of the current / previous panel
  double * sc = Xd + 2 * NB * XDS;                                 // [64] scratch of the diagonal block's wave
  double * sb = sc + 64;                                           // [m] the front's slice of the right-hand side
  __shared__ int s_fail;
  if (tid == 0) {s_fail = 0;}
  const int nchild = fd.child_end - fd.child_ptr;
  const int nkids = front_nkids(d, fd);               // children whose update matrices are read in place
  const int mp = m / 3;
  const int h = wave - 1;                             // helper number
  const double * Bf = front_b(d, fd);
  const bool clean = d.scatter != 0;
  // Tiles requested from memory one step before they are used.  Helper h opens step jb with the regular tile (jb + 1 + h, jb)
  // (nt <= 8: a column block has at most seven tiles below the diagonal); the helper that will run the look-ahead of step jb
  // holds the diagonal tile (jb + 1, jb + 1); wave 0 loads the first diagonal tile and nothing after it.
  TileRaw cur, curd;
  auto look_helper = [&](int jb) {return (nt - jb - 1) % kPotrfHelpers;};
  auto prefetch = [&](int jb) {                        // for step jb
    if (jb >= nt) {return;}
    if (wave == 0) {
      if (jb == 0) {cur = pivot_tile_load(fd, F, Bf, clean, 0, 0, lane);}
      return;
    }
    const int I = jb + 1 + h;
    if (I < nt) {cur = pivot_tile_load(fd, F, Bf, clean, NB * I, NB * jb, lane);}
    if (jb + 1 < nt && look_helper(jb) == h) {curd = pivot_tile_load(fd, F, Bf, clean, NB * (jb + 1), NB * (jb + 1), lane);}
  };
  prefetch(0);
  // right-hand side: the pivots' entries + the children's forward-solve contributions (gathered through the same maps).  A
  // chain of two dependent loads per entry that nobody needs before the epilogue: the maps are requested here, the
  // contributions after the first step, the sums are formed behind the last one (entries beyond the first 512, and children
  // beyond the third, take the loop there).
  const int first = 3 * fd.first;
  const int tn = tid / 3;
  double rv = 0.0;
  int ca[3] = {-1, -1, -1};
  double cu[3] = {0.0, 0.0, 0.0};
  if (tid < m) {
    if (tid < ns) {rv = rhs[first + tid];}
#pragma unroll
    for (int s = 0; s < 3; ++s) {if (s < nchild) {ca[s] = d.cinv[fd.cinv_ptr + s * mp + tn];}}
  }
  PSTAMP();
  v4d res = v4d{0.0, 0.0, 0.0, 0.0};      // wave 0: the solved tile (jb, jb - 1), kept in registers from the row solves of step jb - 1
  for (int jb = 0; jb < nt; ++jb) {
    const int c0 = jb * NB;
    double * xd = Xd + (jb & 1) * NB * XDS;
    const double * xp = Xd + ((jb + 1) & 1) * NB * XDS;            // L^-T of the previous diagonal block
    if (wave == 0) {
      // the diagonal tile: everything but the last product was left in the tile's own place by the look-ahead of step jb - 1;
      // the last product's operand is `res` -- register r of the accumulator layout is column block r of the tile, which is what
      // a lane supplies to the matrix core for k = lk + 4 r
      v4d acc;
      if (jb == 0) {
        acc = pivot_tile_finish(cur, d, fd, nkids, 0, 0, lane);
      } else {
        const double * sp = X + (c0 + lr) * LD + c0 + lk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {acc[r] = sp[4 * r];}
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-res[kk], res[kk], acc, 0, 0, 0);}
      }
      if (potrf_diag_mfma(acc, X + c0 * LD + c0, LD, lane, xd, rd + c0, sc)) {s_fail = 1;}
    } else {
      // regular tile (I, jb), I = jb + 1 + h
      {
        const int I = jb + 1 + h;
        if (I < nt) {
          v4d acc = pivot_tile_finish(cur, d, fd, nkids, NB * I, c0, lane);
          ll_accumulate(acc, X, LD, c0, NB * I, 0, jb, lane);
          double * cp = X + (NB * I + lr) * LD + c0 + lk;
#pragma unroll
          for (int r = 0; r < 4; ++r) {cp[4 * r] = acc[r];}
        }
      }
      // the other tasks of the step, dealt round robin starting behind the helpers that hold a regular tile
      int slot = look_helper(jb);
      auto mine = [&]() {const bool take = slot == h; slot = slot + 1 == kPotrfHelpers ? 0 : slot + 1; return take;};
      // look-ahead: the next diagonal tile's initial value - sum_{p < jb} L[jb+1][p] L[jb+1][p]^T, parked in the tile's own place
      if (jb + 1 < nt && mine()) {
        v4d acc = pivot_tile_finish(curd, d, fd, nkids, c0 + NB, c0 + NB, lane);
        ll_accumulate(acc, X, LD, c0 + NB, c0 + NB, 0, jb, lane);
        double * cp = X + (c0 + NB + lr) * LD + c0 + NB + lk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {cp[4 * r] = acc[r];}
      }
      prefetch(jb + 1);
      // identity rows (I, jb), I < jb - 1: their value so far (block I's own term, written one step after block I) minus the
      // products with the column blocks I + 1 .. jb - 1 (longest first)
      for (int I = 0; I < jb - 1; ++I) {
        if (!mine()) {continue;}
        double * cp = X + (NB * I + lr) * LD + c0 + lk;
        v4d acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {acc[r] = cp[4 * r];}
        ll_accumulate(acc, X, LD, c0, NB * I, I + 1, jb, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {cp[4 * r] = acc[r];}
      }
      if (jb > 0) {
        const int I = jb - 1;
        // block I's own term for this and the later column blocks J >= jb:  E[I][J] = -L_II^-T L[J][I]^T
        for (int J = jb; J < nt; ++J) {
          if (!mine()) {continue;}
          v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
          const double * xa = X + (NB * J + lr) * LD + NB * I + 4 * lk;
          const double * xb = xp + lr * XDS + 4 * lk;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-xa[kk], xb[kk], acc, 0, 0, 0);}
          double * cp = X + (NB * I + lr) * LD + NB * J + lk;
#pragma unroll
          for (int r = 0; r < 4; ++r) {cp[4 * r] = acc[r];}
        }
        // column block I of W is final: tiles (q <= I, I); W[(16 I + j) + (16 q + i) * nsp] = (L^-T)[16 q + i][16 I + j]
        for (int q = 0; q <= I; ++q) {
          if (!mine()) {continue;}
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int idx = lane + 64 * e, i = idx >> 4, j = idx & 15;
            W[(NB * I + j) + (int64_t)(NB * q + i) * nsp] = q == I ? xp[i * XDS + j] : X[(NB * q + i) * LD + NB * I + j];
          }
        }
      }
    }
    lds_barrier();                       // the tiles of column block jb and L_jj^-T are in place
    PSTAMP();
    if (jb == 0 && tid < m) {
      // second hop of the right-hand side's gather (the maps have long arrived)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (ca[s] >= 0) {cu[s] = upd[3 * (int64_t)fd.ch[s].rows_ptr + 3 * ca[s] + (tid - 3 * tn)];}
      }
    }
    // row solves, one 16-row tile per wave: rows below the block (L11 part) and the identity rows above it (the block's own
    // identity rows ARE xd).  Wave 0 takes the tile under the diagonal and keeps the result: its next diagonal tile needs it.
    if (wave == 0) {
      if (jb + 1 < nt) {res = potrf_rowsolve_tile(X + NB * (jb + 1) * LD + c0, LD, xd, lane);}
    } else {
      const int bi = h < jb ? h : h + 2;
      if (bi < nt) {(void)potrf_rowsolve_tile(X + NB * bi * LD + c0, LD, xd, lane);}
    }
    lds_barrier();
    PSTAMP();
  }
  // last column block of W
  {
    const int I = nt - 1;
    const double * xl = Xd + (I & 1) * NB * XDS;
    for (int q = wave; q <= I; q += kPotrfThreads / 64) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = lane + 64 * e, i = idx >> 4, j = idx & 15;
        W[(NB * I + j) + (int64_t)(NB * q + i) * nsp] = q == I ? xl[i * XDS + j] : X[(NB * q + i) * LD + NB * I + j];
      }
    }
  }
  // the right-hand side slice: the sums of the staged gather, then whatever it did not cover
  for (int t = tid; t < m; t += nthreads) {
    double v;
    int s0;
    if (t == tid) {
      v = (rv + cu[0]) + cu[1];
      v += cu[2];
      s0 = 3;
      if (nchild < 3) {v = rv; for (int s = 0; s < nchild; ++s) {v += cu[s];}}
    } else {
      v = t < ns ? rhs[first + t] : 0.0;
      s0 = 0;
    }
    const int tq = t / 3;
    for (int s = s0; s < nchild; ++s) {
      const ChildInfo c = child_info(d, fd, s);
      const int a = d.cinv[fd.cinv_ptr + s * mp + tq];
      const double u = upd[3 * (int64_t)c.rows_ptr + (a >= 0 ? 3 * a + (t - 3 * tq) : 0)];
      v += a >= 0 ? u : 0.0;
    }
    sb[t] = v;
  }
  __syncthreads();
  // y1 = L11^-1 b1 = W^T b1: four threads per entry, each with a quarter of the sum
  {
    const int j = tid >> 2, part = tid & 3;
    double acc = 0.0;
    if (j < ns) {
      // rows q < j of column j, split in four runs of equal length; the last run also takes the diagonal term
      const int q0 = (j * part) >> 2, q1 = (j * (part + 1)) >> 2;
#pragma unroll 8
      for (int q = q0; q < q1; ++q) {acc += X[q * LD + j] * sb[q];}
      if (part == 3) {acc += rd[j] * sb[j];}
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    if (j < ns && part == 0) {yv[j] = acc;}
  }
  __syncthreads();
  for (int t = tid; t < ns; t += nthreads) {rhs[first + t] = yv[t];}
  {
    double * uk = upd + 3 * (int64_t)fd.rows_ptr;
    for (int q = tid; q < m - ns; q += nthreads) {uk[q] = sb[ns + q];}
  }
  PSTAMP();
  if (tbuf && blockIdx.x == 0 && threadIdx.x == 0) {
    tbuf[0] = tcount; tbuf[63] = ((long long)m << 32) | ns;
    for (int i = 0; i < tcount; ++i) {tbuf[1 + i] = stamps[i];}
  }
  if (tid == 0 && s_fail) {atomicExch(fail_flag, 1);}
}

__global__ __launch_bounds__(kPotrfThreads) void k_potrf(SpaDev d, int first_front, int32_t * fail_flag, double * rhs, double * upd, int lds_nsp,
                                                         long long * tbuf, int stamp_off)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  potrf_body(d, fd, fail_flag, rhs, upd, lds_nsp, tbuf, stamp_off);
}

static size_t potrf_lds_bytes(int nsp, int max_m)
{
  return sizeof(double) * ((size_t)nsp * (nsp + 2) + 2 * (size_t)nsp + 2 * NB * XDS + 64 + (size_t)max_m + 8);
}

// k_potrf's LDS is the largest of the pipeline; the last term is k_backward3's (spa_update.hip), which stays under the 64 KB a
// kernel may take without an attribute
bool spa_level_pipeline_fits(int32_t max_m, int32_t max_ns)
{
  const int nsp = (max_ns + NB - 1) & ~(NB - 1);
  return max_ns <= kPotrfMaxNs && potrf_lds_bytes(nsp, max_m) <= 160 * 1024 - 256 && sizeof(double) * ((size_t)max_m + nsp + 8) <= 64 * 1024;
}

static void pipeline_attributes()
{
  // (per device: the attribute is kept per device, and solvers of several devices may live in one process)
  const int big = 160 * 1024 - 256;       // static LDS (a flag word) counts against the same 160 KB
  static std::atomic<unsigned long long> done{0};
  allow_dynamic_lds(reinterpret_cast<const void *>(k_potrf), big, done);
}

void spa_launch_potrf_level(const SpaDev & d, int32_t first_front, int32_t n, int32_t max_m, int32_t max_ns, int32_t * fail_flag,
                            double * rhs, double * upd, void * stream)
{
  if (n <= 0) {return;}
  hipStream_t s = (hipStream_t)stream;
  const int nsp = (max_ns + NB - 1) & ~(NB - 1);
  pipeline_attributes();
  static long long * tbuf = nullptr;
  static const bool timing = std::getenv("KH_SPA_TIMING") != nullptr;
  if (timing && !tbuf) {(void)hipHostMalloc(reinterpret_cast<void **>(&tbuf), 128 * sizeof(long long), hipHostMallocDefault);}
  const size_t lds = potrf_lds_bytes(nsp, max_m);
  hipLaunchKernelGGL(k_potrf, dim3(n), dim3(kPotrfThreads), lds + (timing ? 512 : 0), s, d, first_front, fail_flag, rhs, upd, nsp,
                     timing ? tbuf : (long long *)nullptr, (int)(lds / 8));
  if (timing) {
    (void)hipStreamSynchronize(s);
    std::fprintf(stderr, "[k_potrf] n=%d front0 m=%lld ns=%lld stamps (shader clocks):", n, tbuf[63] >> 32, tbuf[63] & 0xffffffff);
    for (int i = 1; i < (int)tbuf[0]; ++i) {std::fprintf(stderr, " %lld", tbuf[1 + i] - tbuf[i]);}
    std::fprintf(stderr, "\n");
  }
}

}  // namespace kh
