// Pose-graph covariances of the SPA solver (hot path B): the selected inverse of the factor the level pipeline left in the
// fronts (k_selinv_head, k_selinv_z21, k_selinv_z11, k_selinv_clean), and k_cov_gather, the marginal blocks on H's own pattern.
// Launchers: spa_launch_selinv_level, spa_launch_selinv_clean, spa_launch_cov_gather, called by spa_covariance.cpp.  The tile
// product (selinv_product) is spa_device.hpp's: the covariance columns (spa_cov_columns.hip) use it too.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "spa_device.hpp"

#pragma clang fp contract(fast)

namespace kh
{

// ---------------------------------------------------------------------------------------------
// Selected inverse of the factor (Takahashi's recurrence), the walk back DOWN the assembly tree: Z = (L L^T)^-1 on the pattern of L.
// Z lives in a buffer of its own (zbuf) with the fronts' offsets and leading dimensions, every front's m x m block stored
// in full (both triangles, bit-wise symmetric: a value is computed once and stored twice), so a child reads the parent's block
// without caring which triangle an entry is in.  Per front, with W = L11^-T from the level pipeline and L21 from the fronts:
//   k_selinv_head   Z22 <- the parent's Z at this front's struct rows (relpos), and G = L21 W^T written OVER L21 (a 16-row slab per
//                   workgroup: all of its column blocks are computed before the first one is stored)
//   k_selinv_z21    Z21 = -Z22 G  (and Z12, its transpose)
//   k_selinv_z11    Z11 = W W^T - G^T Z21
// three launches per level, root level first; a wave per 16 x 16 tile, operands straight from memory (L2) into v_mfma_f64_16x16x4.
// Tiles are computed TRANSPOSED where that makes the store run along a column (lane & 15 = the row of Z).
constexpr int kSelinvHeadThreads = 64 * (kPotrfMaxNs / NB);       // a wave per column block of the pivots

// blockIdx.y < g_slabs: slab blockIdx.y of G; the other workgroups of a front share the gather of Z22
__global__ __launch_bounds__(kSelinvHeadThreads) void k_selinv_head(SpaDev d, int first_front, double * zbuf, int g_slabs)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  if (nu == 0) {return;}                                 // a root: Z11 = W W^T is all there is
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.y >= g_slabs) {
    const FrontDesc & pd = d.desc[fd.parent];
    const double * Zp = zbuf + pd.off;
    double * Z = zbuf + fd.off;
    const int64_t pm = pd.m;
    const int32_t * rp = d.relpos + fd.relpos_ptr;
    const int64_t total = (int64_t)nu * nu, stride = (int64_t)((int)gridDim.y - g_slabs) * kSelinvHeadThreads;
    for (int64_t t = (int64_t)((int)blockIdx.y - g_slabs) * kSelinvHeadThreads + tid; t < total; t += stride) {
      const int j = (int)(t / nu), i = (int)(t - (int64_t)j * nu);
      const int pi = 3 * rp[i / 3] + i % 3, pj = 3 * rp[j / 3] + j % 3;
      Z[(ns + i) + (int64_t)(ns + j) * m] = Zp[pi + pj * pm];
    }
    return;
  }
  const int i0 = NB * (int)blockIdx.y;
  if (i0 >= nu) {return;}
  const int nsp = (ns + NB - 1) & ~(NB - 1);
  double * L = d.fronts + fd.off + ns;                   // L21[i][k] = L[i + k m]
  const double * W = d.winv + fd.woff;                   // (L11^-T)[c][k] = W[k + c nsp] for k >= c; nothing to rely on left of the diagonal
  const int c0 = NB * wave;
  const bool live = c0 < ns;
  v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
  if (live) {
    // D[c][i] = sum_{k >= c} W[c][k] L21[i][k]  (= G[i][c])
    acc = selinv_product(
      [&](int c, int k) {const bool ok = c0 + c < ns && k >= c0 + c && k < ns; const double v = W[ok ? k + (int64_t)(c0 + c) * nsp : 0]; return ok ? v : 0.0;},
      [&](int k, int i) {const bool ok = i0 + i < nu && k < ns; const double v = L[ok ? (i0 + i) + (int64_t)k * m : 0]; return ok ? v : 0.0;},
      c0, ns, lane);
  }
  __syncthreads();                                       // every column block of the slab has read L21 before G goes over it
  if (live) {
    const int i = i0 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + (lane >> 4) + 4 * r;
      if (i < nu && c < ns) {L[i + (int64_t)c * m] = acc[r];}
    }
  }
}

// a wave per tile (16 struct rows x 16 pivot columns) of Z21 = -Z22 G
__global__ __launch_bounds__(256) void k_selinv_z21(SpaDev d, int first_front, double * zbuf)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nib = (nu + NB - 1) / NB, ncb = (ns + NB - 1) / NB;
  const int t = 4 * (int)blockIdx.y + wave;
  if (t >= nib * ncb) {return;}
  const int cb = t / nib, i0 = NB * (t - cb * nib), c0 = NB * cb;
  const double * G = d.fronts + fd.off + ns;
  double * Z = zbuf + fd.off;
  // D[c][i] = -sum_k G[k][c] Z22[k][i]
  const v4d acc = selinv_product(
    [&](int c, int k) {const bool ok = c0 + c < ns && k < nu; const double v = G[ok ? k + (int64_t)(c0 + c) * m : 0]; return ok ? -v : 0.0;},
    [&](int k, int i) {const bool ok = i0 + i < nu && k < nu; const double v = Z[ok ? (ns + i0 + i) + (int64_t)(ns + k) * m : 0]; return ok ? v : 0.0;},
    0, nu, lane);
  const int i = i0 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = c0 + (lane >> 4) + 4 * r;
    if (i < nu && c < ns) {
      Z[(ns + i) + (int64_t)c * m] = acc[r];
      Z[c + (int64_t)(ns + i) * m] = acc[r];
    }
  }
}

// a wave per tile of the lower triangle of Z11 = W W^T - G^T Z21 (tile row A >= tile column B)
__global__ __launch_bounds__(256) void k_selinv_z11(SpaDev d, int first_front, double * zbuf)
{
  const FrontDesc fd = d.desc[first_front + blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncb = (ns + NB - 1) / NB;
  const int t = 4 * (int)blockIdx.y + wave;
  if (t >= ncb * (ncb + 1) / 2) {return;}
  int A = 0;
  while ((A + 1) * (A + 2) / 2 <= t) {++A;}              // (at most kPotrfMaxNs / NB rounds)
  const int B = t - A * (A + 1) / 2;
  const int a0 = NB * A, b0 = NB * B;
  const int nsp = (ns + NB - 1) & ~(NB - 1);
  const double * W = d.winv + fd.woff;
  const double * G = d.fronts + fd.off + ns;
  double * Z = zbuf + fd.off;
  // D[b][a] = sum_{j >= a, b} W[b][j] W[a][j]  (a0 >= b0: the sum starts at a0 at the earliest)
  v4d acc = selinv_product(
    [&](int b, int j) {const bool ok = b0 + b < ns && j >= b0 + b && j < ns; const double v = W[ok ? j + (int64_t)(b0 + b) * nsp : 0]; return ok ? v : 0.0;},
    [&](int j, int a) {const bool ok = a0 + a < ns && j >= a0 + a && j < ns; const double v = W[ok ? j + (int64_t)(a0 + a) * nsp : 0]; return ok ? v : 0.0;},
    a0, ns, lane);
  // ... - sum_k Z21[k][b] G[k][a]
  acc += selinv_product(
    [&](int b, int k) {const bool ok = b0 + b < ns && k < nu; const double v = Z[ok ? (ns + k) + (int64_t)(b0 + b) * m : 0]; return ok ? -v : 0.0;},
    [&](int k, int a) {const bool ok = a0 + a < ns && k < nu; const double v = G[ok ? k + (int64_t)(a0 + a) * m : 0]; return ok ? v : 0.0;},
    0, nu, lane);
  const int a = a0 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + (lane >> 4) + 4 * r;
    if (a < ns && b <= a) {
      Z[a + (int64_t)b * m] = acc[r];
      Z[b + (int64_t)a * m] = acc[r];
    }
  }
}

void spa_launch_selinv_level(const SpaDev & d, int32_t first_front, int32_t n, int32_t max_m, int32_t max_ns, double * zbuf, void * stream)
{
  if (n <= 0) {return;}
  hipStream_t s = (hipStream_t)stream;
  const int max_nu = max_m - 3;        // a front has at least one pivot node; an upper bound is enough for the grids
  const int ncb = (max_ns + NB - 1) / NB;
  if (max_nu > 0) {
    const int nib = (max_nu + NB - 1) / NB;
    // gather workgroups per front: a narrow level spreads its few large Z22 over the chip, a wide one has workgroups enough
    const int gather = std::max(1, std::min(nib * nib / 2, 256 / n));
    hipLaunchKernelGGL(k_selinv_head, dim3(n, nib + gather), dim3(kSelinvHeadThreads), 0, s, d, first_front, zbuf, nib);
    hipLaunchKernelGGL(k_selinv_z21, dim3(n, (nib * ncb + 3) / 4), dim3(256), 0, s, d, first_front, zbuf);
  }
  hipLaunchKernelGGL(k_selinv_z11, dim3(n, (ncb * (ncb + 1) / 2 + 3) / 4), dim3(256), 0, s, d, first_front, zbuf);
}

// Self-cleaning fronts after a selected inverse: G (where L21 was) is zeroed here, as k_backward3 zeroes L21 behind a solve
__global__ __launch_bounds__(256) void k_selinv_clean(SpaDev d)
{
  const FrontDesc fd = d.desc[blockIdx.x];
  const int m = fd.m, ns = fd.ns, nu = m - ns;
  double * G = d.fronts + fd.off + ns;
  const int total = nu * ns;
  for (int t = (int)blockIdx.y * 256 + (int)threadIdx.x; t < total; t += (int)gridDim.y * 256) {
    const int c = t / nu, i = t - c * nu;
    G[i + (int64_t)c * m] = 0.0;
  }
}
void spa_launch_selinv_clean(const SpaDev & d, void * stream)
{
  if (d.n_fronts <= 0) {return;}
  hipLaunchKernelGGL(k_selinv_clean, dim3(d.n_fronts, 4), dim3(256), 0, (hipStream_t)stream, d);
}

// The blocks of the inverse on H's own pattern, unscaled: cov[slot] = s_i Z_ij s_j.  A block of the lower triangle (elimination
// order) is read where slot_dest puts it, a block of the upper one is the transpose of its mirror slot (found in row j of the
// pattern).  s_i s_j is formed first, so that the array is bit-wise symmetric like Z.
__global__ __launch_bounds__(256) void k_cov_gather(SpaDev d, const int32_t * slot_row, const double * __restrict__ zbuf, const double * __restrict__ scale,
                                                    double * cov)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= d.n_slots * 9) {return;}
  const int slot = t / 9, el = t - slot * 9;
  const int r = el / 3, c = el - r * 3;
  const int i = slot_row[slot], j = d.bsr_col[slot];
  int64_t dest = d.slot_dest[slot];
  double z;
  if (dest >= 0) {
    z = zbuf[dest + r + (int64_t)c * d.slot_ld[slot]];
  } else {
    int lo = d.bsr_row_ptr[j], hi = d.bsr_row_ptr[j + 1] - 1;       // row j holds column i: the pattern is symmetric
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (d.bsr_col[mid] < i) {lo = mid + 1;} else {hi = mid;}
    }
    dest = d.slot_dest[lo];
    z = dest >= 0 ? zbuf[dest + c + (int64_t)r * d.slot_ld[lo]] : 0.0;
  }
  cov[t] = z * (scale[3 * i + r] * scale[3 * j + c]);
}
void spa_launch_cov_gather(const SpaDev & d, const double * zbuf, const double * scale, double * cov, void * stream)
{
  hipLaunchKernelGGL(k_cov_gather, dim3((d.n_slots * 9 + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, d.bsr_col + d.n_slots, zbuf, scale, cov);
}

}  // namespace kh
