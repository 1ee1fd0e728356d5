// Covariance between any two poses of the SPA solver's graph (hot path B): block columns of the inverse for a handful of query
// nodes (k_cov_columns_init / _forward / _backward / _gather), and what is formed from a column and the resident marginals:
// relative covariances (k_cov_relative) and difference covariances (k_cov_difference).  Launchers: spa_launch_cov_columns_init,
// _forward, _backward, _gather, spa_launch_cov_relative, spa_launch_cov_difference, called by spa_covariance.cpp; the columns' plan
// (which fronts carry which query) is covariance_columns_plan.hpp's.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "spa_device.hpp"

#pragma clang fp contract(fast)

namespace kh
{

// ---------------------------------------------------------------------------------------------
// Covariance columns: block columns of Sigma for a handful of query nodes, A X = E_q through the factor while a covariance pass
// still has it in the fronts (G = L21 W^T where L21 was, W = L11^-T in winv).  B holds the right-hand sides, 3 n_free rows in
// elimination order x R columns, row-major: 16 consecutive columns of a row are one 128-byte piece, which is how the matrix core
// wants its B operand (lane l: row l >> 4, column l & 15) and how it hands back its result.  Per front
//   forward   Y1 = W^T B1 (in place of B1),  B[struct rows] -= G B1      only the columns of the queries whose path holds the front
//   backward  X1 = W Y1 - G^T X2             every front, every column
// a workgroup per (front, 16 columns), a wave per 16 x 16 tile of the result; both sweeps overwrite the pivot rows they read, so
// the tiles of a workgroup are all computed before the first is stored.  A front's struct rows are pivot rows of its ancestors,
// which sit on higher levels, and per column at most one front of a level is on the column's path: every (row, column) has one
// writer per launch, no atomics, and a column's bits do not depend on what else was asked for.
constexpr int kCovColThreads = 64 * (kPotrfMaxNs / NB);           // a wave per block of 16 pivot rows

__global__ __launch_bounds__(256) void k_cov_columns_init(SpaDev d, const int32_t * __restrict__ query_elim, int n_queries, int R,
                                                          const double * __restrict__ scale, double * B)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 3 * n_queries) {return;}
  const int k = t / 3, c = t - 3 * k;
  const int e = query_elim[k];
  if (e < 0) {return;}                                             // the gauge node: its column stays zeros
  B[(int64_t)(3 * e + c) * R + t] = scale[3 * d.free_of_elim[e] + c];
}
void spa_launch_cov_columns_init(const SpaDev & d, const int32_t * query_elim, int32_t n_queries, int32_t R, const double * scale, double * B, void * stream)
{
  (void)hipMemsetAsync(B, 0, sizeof(double) * 3 * (size_t)d.n_free * R, (hipStream_t)stream);
  hipLaunchKernelGGL(k_cov_columns_init, dim3((3 * n_queries + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, query_elim, n_queries, R, scale, B);
}

__global__ __launch_bounds__(kCovColThreads) void k_cov_columns_forward(SpaDev d, const int32_t * __restrict__ list, const uint64_t * __restrict__ front_mask,
                                                                        int R, double * B)
{
  const int front = list[blockIdx.x];
  const uint64_t mask = front_mask[front];
  const int j0 = NB * (int)blockIdx.y;
  // (column j belongs to query j / 3; R <= 3 * 64, so the shift stays below 64, and the padding columns are nobody's)
  auto carried = [&](int j) {return ((mask >> ((j0 + j) / 3)) & 1) != 0;};
  bool any = false;
  for (int j = 0; j < NB; ++j) {any = any || carried(j);}
  if (!any) {return;}                                              // (the whole workgroup: nothing of this tile passes through the front)
  const FrontDesc fd = d.desc[front];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  const int nsp = (ns + NB - 1) & ~(NB - 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = kCovColThreads / 64;
  const double * W = d.winv + fd.woff;                             // (L11^-T)[k][c] = W[c + k nsp] for c >= k
  const double * G = d.fronts + fd.off + ns;                       // G[i][c] = G[i + c m]
  double * B1 = B + (int64_t)3 * fd.first * R;
  const int32_t * rows = d.front_rows + fd.rows_ptr;
  auto b1 = [&](int k, int j) {const bool ok = k < ns && carried(j); const double v = B1[ok ? (int64_t)k * R + j0 + j : 0]; return ok ? v : 0.0;};
  // Y1[c][j] = sum_{k <= c} W[k][c] B1[k][j]
  const int c0 = NB * wave;
  const bool live = c0 < ns;
  v4d y = v4d{0.0, 0.0, 0.0, 0.0};
  if (live) {
    y = selinv_product(
      [&](int c, int k) {const bool ok = c0 + c < ns && k <= c0 + c; const double v = W[ok ? (c0 + c) + (int64_t)k * nsp : 0]; return ok ? v : 0.0;},
      b1, 0, c0 + NB < ns ? c0 + NB : ns, lane);
  }
  // B[row of struct i][j] -= sum_c G[i][c] B1[c][j]
  const int j = lane & 15;
  for (int i0 = NB * wave; i0 < nu; i0 += NB * nwaves) {
    const v4d acc = selinv_product(
      [&](int i, int c) {const bool ok = i0 + i < nu && c < ns; const double v = G[ok ? (i0 + i) + (int64_t)c * m : 0]; return ok ? v : 0.0;},
      b1, 0, ns, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + (lane >> 4) + 4 * r;
      if (i < nu && carried(j)) {
        double * p = B + (int64_t)(3 * rows[i / 3] + i % 3) * R + j0 + j;
        *p = *p - acc[r];
      }
    }
  }
  __syncthreads();                                                 // every tile has read B1 before Y1 goes over it
  if (live) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + (lane >> 4) + 4 * r;
      if (c < ns && carried(j)) {B1[(int64_t)c * R + j0 + j] = y[r];}
    }
  }
}
void spa_launch_cov_columns_forward(const SpaDev & d, const int32_t * list, int32_t n, const uint64_t * front_mask, int32_t R, double * B, void * stream)
{
  if (n <= 0) {return;}
  hipLaunchKernelGGL(k_cov_columns_forward, dim3(n, R / NB), dim3(kCovColThreads), 0, (hipStream_t)stream, d, list, front_mask, R, B);
}

__global__ __launch_bounds__(kCovColThreads) void k_cov_columns_backward(SpaDev d, int first_front, int R, double * B)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  const int nsp = (ns + NB - 1) & ~(NB - 1);
  const int j0 = NB * (int)blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double * W = d.winv + fd.woff;                             // (L11^-T)[c][k] = W[k + c nsp] for k >= c
  const double * G = d.fronts + fd.off + ns;
  double * B1 = B + (int64_t)3 * fd.first * R;
  const int32_t * rows = d.front_rows + fd.rows_ptr;
  const int c0 = NB * wave;
  const bool live = c0 < ns;
  v4d x = v4d{0.0, 0.0, 0.0, 0.0};
  if (live) {
    // X1[c][j] = sum_{k >= c} W[c][k] Y1[k][j] ...
    x = selinv_product(
      [&](int c, int k) {const bool ok = c0 + c < ns && k >= c0 + c && k < ns; const double v = W[ok ? k + (int64_t)(c0 + c) * nsp : 0]; return ok ? v : 0.0;},
      [&](int k, int j) {const bool ok = k < ns; const double v = B1[ok ? (int64_t)k * R + j0 + j : 0]; return ok ? v : 0.0;},
      c0, ns, lane);
    // ... - sum_i G[i][c] X2[i][j], X2 = the rows of the ancestors, final since their levels' launches
    if (nu > 0) {
      x += selinv_product(
        [&](int c, int i) {const bool ok = c0 + c < ns && i < nu; const double v = G[ok ? i + (int64_t)(c0 + c) * m : 0]; return ok ? -v : 0.0;},
        [&](int i, int j) {const bool ok = i < nu; const double v = B[ok ? (int64_t)(3 * rows[i / 3] + i % 3) * R + j0 + j : 0]; return ok ? v : 0.0;},
        0, nu, lane);
    }
  }
  __syncthreads();                                                 // every tile has read Y1 before X1 goes over it
  if (live) {
    const int j = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + (lane >> 4) + 4 * r;
      if (c < ns) {B1[(int64_t)c * R + j0 + j] = x[r];}
    }
  }
}
void spa_launch_cov_columns_backward(const SpaDev & d, int32_t first_front, int32_t n, int32_t R, double * B, void * stream)
{
  if (n <= 0) {return;}
  hipLaunchKernelGGL(k_cov_columns_backward, dim3(n, R / NB), dim3(kCovColThreads), 0, (hipStream_t)stream, d, first_front, R, B);
}

// the block columns, unscaled and in free-node order: columns[(k n_free + i) 9 + 3 r + c] = s_(i, r) X[3 elim(i) + r][3 k + c]
__global__ __launch_bounds__(256) void k_cov_columns_gather(SpaDev d, int n_queries, int R, const double * __restrict__ scale, const double * __restrict__ B,
                                                            double * columns)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)n_queries * d.n_free * 9) {return;}
  const int el = (int)(t % 9);
  const int64_t blk = t / 9;
  const int i = (int)(blk % d.n_free), k = (int)(blk / d.n_free);
  const int r = el / 3, c = el - 3 * r;
  columns[t] = B[(int64_t)(3 * d.elim_of_free[i] + r) * R + 3 * k + c] * scale[3 * i + r];
}
void spa_launch_cov_columns_gather(const SpaDev & d, int32_t n_queries, int32_t R, const double * scale, const double * B, double * columns, void * stream)
{
  const int64_t total = (int64_t)n_queries * d.n_free * 9;
  hipLaunchKernelGGL(k_cov_columns_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, n_queries, R, scale, B, columns);
}

// Relative covariances: node i's pose in the frame of the reference node r, d = R(-theta_r) (t_i - t_r), theta_i - theta_r, to
// first order: J [[S_rr S_ri], [S_ir S_ii]] J^T with J = [Jr Ji] = [dd/dr dd/di].  All 3 x 3 in registers; the two halves
// Jr S_r. + Ji S_i. are formed as separate products and added, so that for i = r (Ji = -Jr, the four blocks all S_rr) they
// cancel exactly.  No contraction here: the host's restatement (scan_solver.relative_covariance) has none either.
__device__ __forceinline__ void mat3_mul(const double (&a)[9], const double (&b)[9], double (&o)[9])
{
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];}
  }
}
__global__ __launch_bounds__(256) void k_cov_relative(SpaDev d, const double * __restrict__ cov, const double * __restrict__ column, int ref_free,
                                                      const double * __restrict__ ref_pose, const int32_t * __restrict__ free_idx,
                                                      const double * __restrict__ poses, int n, double * out)
{
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) {return;}
  const int fi = free_idx[t];
  double srr[9], sii[9], sir[9], sri[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    srr[q] = ref_free >= 0 ? cov[9 * (int64_t)d.bsr_diag_slot[ref_free] + q] : 0.0;
    sii[q] = fi >= 0 ? cov[9 * (int64_t)d.bsr_diag_slot[fi] + q] : 0.0;
    sir[q] = fi == ref_free ? srr[q] : (fi >= 0 && ref_free >= 0 ? column[9 * (int64_t)fi + q] : 0.0);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {sri[3 * r + c] = sir[3 * c + r];}
  }
  const double cs = cos(ref_pose[2]), sn = sin(ref_pose[2]);
  const double dx = poses[3 * t] - ref_pose[0], dy = poses[3 * t + 1] - ref_pose[1];
  const double jr[9] = {-cs, -sn, -sn * dx + cs * dy, sn, -cs, -cs * dx - sn * dy, 0.0, 0.0, -1.0};
  const double ji[9] = {cs, sn, 0.0, -sn, cs, 0.0, 0.0, 0.0, 1.0};
  double jrt[9], jit[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {jrt[3 * r + c] = jr[3 * c + r]; jit[3 * r + c] = ji[3 * c + r];}
  }
  // [Tr Ti] = J S
  double a[9], b[9], tr[9], ti[9];
  mat3_mul(jr, srr, a); mat3_mul(ji, sir, b);
#pragma unroll
  for (int q = 0; q < 9; ++q) {tr[q] = a[q] + b[q];}
  mat3_mul(jr, sri, a); mat3_mul(ji, sii, b);
#pragma unroll
  for (int q = 0; q < 9; ++q) {ti[q] = a[q] + b[q];}
  mat3_mul(tr, jrt, a); mat3_mul(ti, jit, b);
#pragma unroll
  for (int q = 0; q < 9; ++q) {out[9 * (int64_t)t + q] = a[q] + b[q];}
}
void spa_launch_cov_relative(const SpaDev & d, const double * cov, const double * column, int32_t ref_free, const double * ref_pose,
                             const int32_t * free_idx, const double * poses, int32_t n, double * out, void * stream)
{
  if (n <= 0) {return;}
  hipLaunchKernelGGL(k_cov_relative, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, cov, column, ref_free, ref_pose, free_idx, poses, n, out);
}

// Difference covariances: the covariance of x_i - x_r in the WORLD frame, D = S_ii + S_rr - S_ir - S_ir^T, no pose and no rotation
// (what a gate over the store's world positions wants).  One thread per listed node; the upper triangle is computed --
// ((S_ii + S_rr) - S_ir) - S_ri, entry by entry, each operation rounded on its own -- and mirrored, so D is bit-wise symmetric
// whatever the marginals are.  The gauge node's blocks are zeros; i = r is exact zeros by construction, not by cancellation.
__global__ __launch_bounds__(256) void k_cov_difference(SpaDev d, const double * __restrict__ cov, const double * __restrict__ column, int ref_free,
                                                        const int32_t * __restrict__ free_idx, int n, double * out)
{
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) {return;}
  const int fi = free_idx[t];
  double srr[9], sii[9], sir[9], o[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    srr[q] = ref_free >= 0 ? cov[9 * (int64_t)d.bsr_diag_slot[ref_free] + q] : 0.0;
    sii[q] = fi >= 0 ? cov[9 * (int64_t)d.bsr_diag_slot[fi] + q] : 0.0;
    sir[q] = fi >= 0 && ref_free >= 0 ? column[9 * (int64_t)fi + q] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = r; c < 3; ++c) {
      const double v = fi == ref_free ? 0.0 : ((sii[3 * r + c] + srr[3 * r + c]) - sir[3 * r + c]) - sir[3 * c + r];
      o[3 * r + c] = v; o[3 * c + r] = v;
    }
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) {out[9 * (int64_t)t + q] = o[q];}
}
void spa_launch_cov_difference(const SpaDev & d, const double * cov, const double * column, int32_t ref_free, const int32_t * free_idx, int32_t n,
                               double * out, void * stream)
{
  if (n <= 0) {return;}
  hipLaunchKernelGGL(k_cov_difference, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, cov, column, ref_free, free_idx, n, out);
}

}  // namespace kh
