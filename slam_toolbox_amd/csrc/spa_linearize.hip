// K5 of the pose-graph SPA solver (hot path B): linearisation and the scalars of a Levenberg-Marquardt step.
//
//   k_edge_lin      K5a  PoseGraph2dErrorTerm residual + analytic 3x3 Jacobian blocks per edge
//                        (solvers/ceres_utils.h:84-100; autodiff in the reference)
//   k_gather_H/g    K5b  J^T J / J^T r reduced into the BSR normal matrix and gradient.  Gather form:
//                        one thread per output element walks its (precomputed) contribution list in
//                        a fixed order -> no atomics, bit-reproducible H and g.
//   k_assemble      K6a  scaled + damped H scattered into the multifrontal front storage (the fronts are factorised by
//                        spa_potrf.hip + spa_update.hip, or by spa_factor_front.hip)
//   k_step_fused, k_gather_Hg_norms, k_reduce_partials, k_grad_norm_partials   the step evaluation of an iteration
//   k_sum, k_jacobi_scale, k_grad_norms, k_lin_check                             small vector kernels
//
// Launchers: spa_launch_linearize, _jacobi_scale, _assemble, _lin_check, _grad_norms, _step_and_linearize, _step_scalars and
// spa_step_partials_size, called by spa_compute.cpp (the covariance pass of spa_covariance.cpp assembles through it too);
// spa_launch_edge_lin_all for the constraint audit (spa_audit.hip).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "spa_device.hpp"

#pragma clang fp contract(fast)

namespace kh
{

constexpr double kPiD = 3.14159265358979323846;
constexpr double kTwoPiD = 2.0 * kPiD;

// ceres_utils.h:27-32
__device__ __forceinline__ double d_normalize_angle(double a) {return a - kTwoPiD * floor((a + kPiD) / kTwoPiD);}

// per-workgroup reduction of N values per thread (256 threads, tree in LDS, fixed order: bit-reproducible) into out[0 .. N)
template <int N>
__device__ __forceinline__ void block_reduce_store(double (&v)[N], int max_mask, double * out)      // bit q of max_mask: entry q is a maximum
{
  __shared__ double red[N][256];
#pragma unroll
  for (int q = 0; q < N; ++q) {red[q][threadIdx.x] = v[q];}
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const double a = red[q][threadIdx.x], b = red[q][threadIdx.x + w];
        red[q][threadIdx.x] = ((max_mask >> q) & 1) ? fmax(a, b) : a + b;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < N) {out[threadIdx.x] = red[threadIdx.x][0];}
}

// device half of k_edge_lin: returns rho(s) of the edge (0 for the threads behind the last edge).
// [e_lo, e_hi) = the edge block this GPU linearises (all edges on one GPU); edges outside it get a zero
// record, so the gather kernels below produce this rank's PARTIAL H and g, summed across ranks by the
// caller's all-reduce.
template <bool kJac>
__device__ __forceinline__ double edge_lin(const SpaDev & d, const double * __restrict__ x, int e, int e_lo, int e_hi)
{
  if (e >= d.n_edges) {return 0.0;}
  if (kJac && (e < e_lo || e >= e_hi)) {
    double * out = d.edge_lin + 21 * (size_t)e;
#pragma unroll
    for (int q = 0; q < 21; ++q) {out[q] = 0.0;}
    return 0.0;
  }
  const int a = d.edge_a[e], b = d.edge_b[e];
  const double xa = x[3 * a], ya = x[3 * a + 1], ta = x[3 * a + 2];
  const double xb = x[3 * b], yb = x[3 * b + 1], tb = x[3 * b + 2];
  const double c = cos(ta), s = sin(ta);
  const double dx = xb - xa, dy = yb - ya;
  const double * z = d.edge_z + 3 * e;
  const double * U = d.edge_u + 9 * e;
  const double r0 = c * dx + s * dy - z[0];
  const double r1 = -s * dx + c * dy - z[1];
  const double r2 = d_normalize_angle((tb - ta) - z[2]);
  // f = U r (U upper triangular)
  double f0 = U[0] * r0 + U[1] * r1 + U[2] * r2;
  double f1 = U[4] * r1 + U[5] * r2;
  double f2 = U[8] * r2;
  const double sq = f0 * f0 + f1 * f1 + f2 * f2;
  // Robust loss, as Ceres' ResidualBlock::Evaluate + Corrector apply it: cost 0.5 rho(s); both losses the
  // plugin offers have rho'' <= 0, for which the corrector degenerates to scaling the residual and the
  // Jacobian rows by sqrt(rho'(s)).
  double rho0 = sq, w = 1.0;
  if (d.loss_kind == 1) {            // ceres::HuberLoss: s <= b -> (s, 1); else (2 a sqrt(s) - b, a / sqrt(s))
    if (sq > d.loss_b) {
      const double r = sqrt(sq);
      rho0 = 2.0 * d.loss_a * r - d.loss_b;
      w = sqrt(fmax(2.2250738585072014e-308, d.loss_a / r));
    }
  } else if (d.loss_kind == 2) {     // ceres::CauchyLoss: b log(1 + s/b), 1 / (1 + s/b)
    const double sum = 1.0 + sq * (1.0 / d.loss_b);
    rho0 = d.loss_b * log(sum);
    w = sqrt(fmax(2.2250738585072014e-308, 1.0 / sum));
  }
  d.edge_cost[e] = rho0;
  if (!kJac) {return rho0;}
  double * out = d.edge_lin + 21 * (size_t)e;
  f0 *= w; f1 *= w; f2 *= w;
  out[0] = f0; out[1] = f1; out[2] = f2;
  // raw Jacobians (rows = residual, cols = xa, ya, ta | xb, yb, tb)
  const double ja[9] = {-c, -s, -s * dx + c * dy, s, -c, -c * dx - s * dy, 0.0, 0.0, -1.0};
  const double jb[9] = {c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
  for (int col = 0; col < 3; ++col) {
    out[3 + 0 + col] = w * (U[0] * ja[col] + U[1] * ja[3 + col] + U[2] * ja[6 + col]);
    out[3 + 3 + col] = w * (U[4] * ja[3 + col] + U[5] * ja[6 + col]);
    out[3 + 6 + col] = w * (U[8] * ja[6 + col]);
    out[12 + 0 + col] = w * (U[0] * jb[col] + U[1] * jb[3 + col] + U[2] * jb[6 + col]);
    out[12 + 3 + col] = w * (U[4] * jb[3 + col] + U[5] * jb[6 + col]);
    out[12 + 6 + col] = w * (U[8] * jb[6 + col]);
  }
  return rho0;
}

// cost_partial: per-workgroup sums of rho (the step evaluation's form; nullptr: none).  A sharded linearisation (edges outside
// [e_lo, e_hi) get a zero record) does not produce them: the cost is evaluated over all edges by the <false> instance.
template <bool kJac>
__global__ __launch_bounds__(256) void k_edge_lin(SpaDev d, const double * __restrict__ x, int e_lo, int e_hi, double * cost_partial)
{
  double p[1] = {edge_lin<kJac>(d, x, blockIdx.x * blockDim.x + threadIdx.x, e_lo, e_hi)};
  if (cost_partial) {block_reduce_store<1>(p, 0, cost_partial + blockIdx.x);}
}

__device__ __forceinline__ void gather_H(const SpaDev & d, int t)
{
  if (t >= d.n_slots * 9) {return;}
  const int slot = t / 9, el = t - slot * 9;
  const int row = el / 3, col = el - row * 3;
  double acc = 0.0;
  for (int k = d.slot_contrib_ptr[slot]; k < d.slot_contrib_ptr[slot + 1]; ++k) {
    const int code = d.slot_contrib[k];
    const int e = code >> 2, kind = code & 3;
    const double * lin = d.edge_lin + 21 * (size_t)e;
    const double * L = lin + ((kind == 0 || kind == 2) ? 3 : 12);   // left factor (transposed): Ja or Jb
    const double * R = lin + ((kind == 0 || kind == 3) ? 3 : 12);   // right factor
    acc += L[row] * R[col] + L[3 + row] * R[3 + col] + L[6 + row] * R[6 + col];
  }
  d.H[t] = acc;
}
__global__ __launch_bounds__(256) void k_gather_H(SpaDev d) {gather_H(d, blockIdx.x * blockDim.x + threadIdx.x);}

__global__ __launch_bounds__(256) void k_gather_g(SpaDev d)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d.n_free * 3) {return;}
  const int i = t / 3, comp = t - i * 3;
  double acc = 0.0;
  for (int k = d.node_contrib_ptr[i]; k < d.node_contrib_ptr[i + 1]; ++k) {
    const int code = d.node_contrib[k];
    const int e = code >> 1, role = code & 1;
    const double * lin = d.edge_lin + 21 * (size_t)e;
    const double * J = lin + (role ? 12 : 3);
    acc += J[comp] * lin[0] + J[3 + comp] * lin[1] + J[6 + comp] * lin[2];
  }
  d.g[t] = acc;
}

// deterministic single-workgroup sum: out = factor * sum(in[0..n))
__global__ __launch_bounds__(1024) void k_sum(const double * __restrict__ in, int n, double factor, double * out)
{
  __shared__ double s[1024];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {acc += in[i];}
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {s[threadIdx.x] += s[threadIdx.x + w];}
    __syncthreads();
  }
  if (threadIdx.x == 0) {out[0] = factor * s[0];}
}

void spa_launch_linearize(const SpaDev & d, const double * x, double * cost_out, int e_lo, int e_hi, void * stream)
{
  hipStream_t s = (hipStream_t)stream;
  if (d.n_edges > 0) {
    if (e_lo > 0 || e_hi < d.n_edges) {
      // sharded: the cost is still evaluated over all edges on every rank (E threads, microseconds)
      hipLaunchKernelGGL(k_edge_lin<false>, dim3((d.n_edges + 255) / 256), dim3(256), 0, s, d, x, 0, d.n_edges, (double *)nullptr);
    }
    hipLaunchKernelGGL(k_edge_lin<true>, dim3((d.n_edges + 255) / 256), dim3(256), 0, s, d, x, e_lo, e_hi, (double *)nullptr);
    hipLaunchKernelGGL(k_gather_H, dim3((d.n_slots * 9 + 255) / 256), dim3(256), 0, s, d);
    hipLaunchKernelGGL(k_gather_g, dim3((d.n_free * 3 + 255) / 256), dim3(256), 0, s, d);
  }
  hipLaunchKernelGGL(k_sum, dim3(1), dim3(1024), 0, s, d.edge_cost, d.n_edges, 0.5, cost_out);
}

// the linearisation alone, over all edges (the constraint audit's first launch; the caller has checked n_edges > 0)
void spa_launch_edge_lin_all(const SpaDev & d, const double * x, void * stream)
{
  hipLaunchKernelGGL(k_edge_lin<true>, dim3((d.n_edges + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, x, 0, d.n_edges, (double *)nullptr);
}

// ---------------------------------------------------------------------------------------------
// small vector kernels
__global__ void k_jacobi_scale(SpaDev d, double * scale)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d.n_free * 3) {return;}
  const int i = t / 3, c = t - i * 3;
  const double hii = d.H[(size_t)d.bsr_diag_slot[i] * 9 + c * 3 + c];
  scale[t] = 1.0 / (1.0 + sqrt(hii));      // trust_region_minimizer.cc: jacobian_scaling = 1 / (1 + sqrt(colnorm^2))
}
void spa_launch_jacobi_scale(const SpaDev & d, double * scale_out, void * stream)
{
  hipLaunchKernelGGL(k_jacobi_scale, dim3((d.n_free * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, scale_out);
}

// The head of a factorisation in ONE launch (round 6; three launches before): the scaled + damped H into the fronts, the LM
// diagonal itself where a new one is due (compute_diag: clamp(diag(S H S)) to [lo, hi], levenberg_marquardt_strategy.cc -- the entry
// that needs it is the entry that computes it, and it is kept in `diagonal` for the iterations that reuse it), and behind the blocks
// of the matrix the right-hand side rhs (elimination order) <- scale * g and the fail word <- 0.
__global__ __launch_bounds__(256) void k_assemble(SpaDev d, const int32_t * slot_row, const double * scale, double * diagonal, double inv_radius,
                                                  int compute_diag, double lo, double hi, double * rhs, int32_t * fail_flag, int nb_matrix)
{
  if ((int)blockIdx.x >= nb_matrix) {
    const int t = ((int)blockIdx.x - nb_matrix) * 256 + (int)threadIdx.x;
    if (t == 0 && fail_flag) {*fail_flag = 0;}
    if (t >= d.n_free * 3) {return;}
    const int i = t / 3, c = t - i * 3;
    rhs[3 * d.elim_of_free[i] + c] = scale[t] * d.g[t];
    return;
  }
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= d.n_slots * 9) {return;}
  const int slot = t / 9, el = t - slot * 9;
  const int64_t dest = d.slot_dest[slot];
  if (dest < 0) {return;}
  const int r = el / 3, c = el - r * 3;
  const int i = slot_row[slot], j = d.bsr_col[slot];
  // self-cleaning fronts: nothing is written that no kernel of the factorisation reads (and zeroes) -- the entries of a diagonal
  // block above the diagonal would outlive a change of the fronts' layout
  if (d.scatter && i == j && r < c) {return;}
  double v = scale[3 * i + r] * d.H[t] * scale[3 * j + c];
  if (i == j && r == c) {
    double dg;
    if (compute_diag) {
      dg = v < lo ? lo : v;
      dg = dg > hi ? hi : dg;
      diagonal[3 * i + r] = dg;
    } else {
      dg = diagonal[3 * i + r];
    }
    v += dg * inv_radius;
  }
  d.fronts[dest + r + (int64_t)c * d.slot_ld[slot]] = v;
}

// slot_row is stored right behind bsr_col by the host (bsr_col + n_slots)
void spa_launch_assemble(const SpaDev & d, const double * scale, double * diagonal, double inv_radius, bool compute_diag, double min_diag, double max_diag,
                         double * rhs, int32_t * fail_flag, void * stream)
{
  hipStream_t s = (hipStream_t)stream;
  // (the fronts have been zeroed by the caller, or clean themselves)
  const int nbm = (d.n_slots * 9 + 255) / 256, nbr = (d.n_free * 3 + 255) / 256;
  hipLaunchKernelGGL(k_assemble, dim3(nbm + nbr), dim3(256), 0, s, d, d.bsr_col + d.n_slots, scale, diagonal, inv_radius, compute_diag ? 1 : 0, min_diag,
                     max_diag, rhs, fail_flag, nbm);
}

// kh_spa_set_debug bit 0 (debugging aid): the linear system of this iteration, (Hs + D / radius) step + gs = 0 in the scaled
// variables, evaluated with the BSR matrix -- independent of the fronts.  out[0] = |residual|^2, out[1] = |gs|^2.
__global__ __launch_bounds__(1024) void k_lin_check(SpaDev d, const double * scale, const double * diagonal, double inv_radius,
                                                     const double * step, double * out2)
{
  __shared__ double s0[1024];
  __shared__ double s1[1024];
  double a0 = 0.0, a1 = 0.0;
  const int n3 = d.n_free * 3;
  for (int t = threadIdx.x; t < n3; t += 1024) {
    const int i = t / 3, r = t - i * 3;
    double acc = 0.0;
    for (int k = d.bsr_row_ptr[i]; k < d.bsr_row_ptr[i + 1]; ++k) {
      const int j = d.bsr_col[k];
      const double * blk = d.H + (size_t)k * 9 + r * 3;
      acc += blk[0] * scale[3 * j] * step[3 * j] + blk[1] * scale[3 * j + 1] * step[3 * j + 1] + blk[2] * scale[3 * j + 2] * step[3 * j + 2];
    }
    const double gs = scale[t] * d.g[t];
    const double res = scale[t] * acc + diagonal[t] * inv_radius * step[t] + gs;
    a0 += res * res; a1 += gs * gs;
  }
  s0[threadIdx.x] = a0; s1[threadIdx.x] = a1;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {s0[threadIdx.x] += s0[threadIdx.x + w]; s1[threadIdx.x] += s1[threadIdx.x + w];}
    __syncthreads();
  }
  if (threadIdx.x == 0) {out2[0] = s0[0]; out2[1] = s1[0];}
}
void spa_launch_lin_check(const SpaDev & d, const double * scale, const double * diagonal, double inv_radius, const double * step, double * out2,
                          void * stream)
{
  hipLaunchKernelGGL(k_lin_check, dim3(1), dim3(1024), 0, (hipStream_t)stream, d, scale, diagonal, inv_radius, step, out2);
}

__global__ __launch_bounds__(1024) void k_grad_norms(SpaDev d, const double * x, double * out2)
{
  __shared__ double smax[1024];
  __shared__ double ssum[1024];
  double mx = 0.0, sm = 0.0;
  for (int f = threadIdx.x; f < d.n_free; f += 1024) {
    const int n = d.node_of_free[f];
    const double px = x[3 * n], py = x[3 * n + 1], pt = x[3 * n + 2];
    // x - Plus(x, -g)  (projected gradient step, trust_region_minimizer.cc)
    const double ex = px - (px - d.g[3 * f]), ey = py - (py - d.g[3 * f + 1]);
    const double et = pt - d_normalize_angle(pt - d.g[3 * f + 2]);
    mx = fmax(mx, fmax(fabs(ex), fmax(fabs(ey), fabs(et))));
    sm += px * px + py * py + pt * pt;
  }
  smax[threadIdx.x] = mx; ssum[threadIdx.x] = sm;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]);
      ssum[threadIdx.x] += ssum[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {out2[0] = smax[0]; out2[1] = ssum[0];}
}
void spa_launch_grad_norms(const SpaDev & d, const double * x, double * out2, void * stream)
{
  hipLaunchKernelGGL(k_grad_norms, dim3(1), dim3(1024), 0, (hipStream_t)stream, d, x, out2);
}

// ---------------------------------------------------------------------------------------------
// The step evaluation of an LM iteration in five launches (single GPU): fourteen small launches -- six of them one-workgroup
// sums over 30 000 values, 8-10 us each -- were 0.15 ms of every iteration.  Every kernel leaves per-workgroup partial
// sums (tree reduction in LDS, fixed order: bit-reproducible), and one last workgroup adds the partials up.
//   k_step_fused   step = -y, delta = step * scale, cand = Plus(x, delta), model-cost terms, step norms  (thread = free node)
//   k_edge_lin<true>  candidate cost + linearisation, cost partials
//   k_gather_Hg_norms  normal equations at the candidate, gradient-norm partials (sharded: k_gather_H, k_gather_g, then
//                      k_grad_norm_partials behind the all-reduce)
//   k_reduce_partials
// four lanes per free node: its row of H holds ~7 blocks, each a dependent (column -> step of the column) pair of loads; with one
// thread per node the kernel was 40 workgroups walking them one after the other (20 us for 10 000 nodes)
constexpr int kStepLanes = 4;
__global__ __launch_bounds__(256) void k_step_fused(SpaDev d, const double * __restrict__ scale, const double * __restrict__ rhs,
                                                    const double * __restrict__ x, double * step, double * delta, double * cand, double * partial)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int i = t / kStepLanes, sub = t % kStepLanes;
  double p[5] = {0.0, 0.0, 0.0, 0.0, 0.0};        // step.gs, step^T Hs step, non-finite marker, |x - cand|^2, |cand|^2
  const bool live = i < d.n_free;
  double acc[3] = {0.0, 0.0, 0.0};
  if (live) {
    for (int k = d.bsr_row_ptr[i] + sub; k < d.bsr_row_ptr[i + 1]; k += kStepLanes) {
      const int j = d.bsr_col[k];
      const int ej = d.elim_of_free[j];
      const double * blk = d.H + (size_t)k * 9;
      double sj[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {sj[c] = scale[3 * j + c] * -rhs[3 * ej + c];}
#pragma unroll
      for (int r = 0; r < 3; ++r) {acc[r] += blk[3 * r] * sj[0] + blk[3 * r + 1] * sj[1] + blk[3 * r + 2] * sj[2];}
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    acc[r] += __shfl_xor(acc[r], 1);
    acc[r] += __shfl_xor(acc[r], 2);
  }
  if (live && sub == 0) {
    const int e = d.elim_of_free[i];
    double st[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {st[c] = -rhs[3 * e + c];}                 // levenberg_marquardt_strategy.cc: step *= -1
    double dl[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double sc = scale[3 * i + r];
      step[3 * i + r] = st[r];
      dl[r] = st[r] * sc;                                                  // trust_region_minimizer.cc: delta = step .* jacobian_scaling
      delta[3 * i + r] = dl[r];
      p[0] += st[r] * sc * d.g[3 * i + r];
      p[1] += st[r] * (acc[r] * sc);
      p[2] += (st[r] - st[r] == 0.0) ? 0.0 : 1.0;
    }
    const int n = d.node_of_free[i];
    const double px = x[3 * n], py = x[3 * n + 1], pt = x[3 * n + 2];
    const double nx = px + dl[0], ny = py + dl[1];
    const double nt = d_normalize_angle(pt + dl[2]);                       // AngleLocalParameterization, ceres_utils.h:38-55
    const double ex = px - nx, ey = py - ny, et = pt - nt;
    p[3] = ex * ex + ey * ey + et * et;
    p[4] = nx * nx + ny * ny + nt * nt;
    cand[3 * n] = nx; cand[3 * n + 1] = ny; cand[3 * n + 2] = nt;
  }
  block_reduce_store<5>(p, 0, partial + 5 * blockIdx.x);
}

// The normal equations at the candidate in ONE launch: the first nbg workgroups gather the gradient (and leave the projected-
// gradient norm partials), the others the blocks of H -- two launches in round 5, the shorter one (10 us) a boundary and a ramp
// of its own on the critical stream.
__global__ __launch_bounds__(256) void k_gather_Hg_norms(SpaDev d, const double * __restrict__ x, double * partial, int nbg)
{
  if ((int)blockIdx.x >= nbg) {gather_H(d, ((int)blockIdx.x - nbg) * 256 + (int)threadIdx.x); return;}
  const int t = blockIdx.x * 256 + threadIdx.x;
  double p[2] = {0.0, 0.0};                       // max |x - Plus(x, -g)|, |x_free|^2
  if (t < d.n_free * 3) {
    const int i = t / 3, comp = t - i * 3;
    double acc = 0.0;
    for (int k = d.node_contrib_ptr[i]; k < d.node_contrib_ptr[i + 1]; ++k) {
      const int code = d.node_contrib[k];
      const int e = code >> 1, role = code & 1;
      const double * lin = d.edge_lin + 21 * (size_t)e;
      const double * J = lin + (role ? 12 : 3);
      acc += J[comp] * lin[0] + J[3 + comp] * lin[1] + J[6 + comp] * lin[2];
    }
    d.g[t] = acc;
    const double v = x[3 * d.node_of_free[i] + comp];
    const double moved = comp == 2 ? d_normalize_angle(v - acc) : v - acc;
    p[0] = fabs(v - moved);
    p[1] = v * v;
  }
  block_reduce_store<2>(p, 1, partial + 2 * blockIdx.x);
}

// out[3..7] <- step partials, out[8] <- 0.5 * cost partials, out[9], out[10] <- gradient norm partials.  With h_out (host-coherent
// memory): the same eight numbers and the factorisation's fail word (h_out[11]) go straight to the host, then the flag h_flag <- seq
// (system-scope release): the LM loop reads its iteration's scalars without two copy nodes and a stream drain (30 us of every
// iteration).
__global__ __launch_bounds__(256) void k_reduce_partials(const double * ps, int ns, const double * pe, int ne, const double * pg, int ng, double * out,
                                                         double * h_out, int32_t * h_flag, const int32_t * fail_flag, int32_t seq)
{
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < ns; b += 256) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {v[q] += ps[5 * b + q];}
  }
  for (int b = threadIdx.x; b < ne; b += 256) {v[5] += pe[b];}
  for (int b = threadIdx.x; b < ng; b += 256) {v[6] = fmax(v[6], pg[2 * b]); v[7] += pg[2 * b + 1];}
  __shared__ double res[8];
  block_reduce_store<8>(v, 1 << 6, res);
  __syncthreads();
  if (threadIdx.x < 5) {out[3 + threadIdx.x] = res[threadIdx.x];}
  if (threadIdx.x == 5) {out[8] = 0.5 * res[5];}
  if (threadIdx.x == 6) {out[9] = res[6];}
  if (threadIdx.x == 7) {out[10] = res[7];}
  if (h_out && threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {h_out[3 + q] = res[q];}
    h_out[8] = 0.5 * res[5]; h_out[9] = res[6]; h_out[10] = res[7];
    h_out[11] = (double)*fail_flag;
    __threadfence_system();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(h_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

int64_t spa_step_partials_size(const SpaDev & d)
{
  return 5 * (int64_t)((kStepLanes * d.n_free + 255) / 256) + (d.n_edges + 255) / 256 + 2 * (int64_t)((3 * d.n_free + 255) / 256) + 16;
}

// projected-gradient norm partials on their own (sharded runs: g is only complete after the all-reduce); the same
// arithmetic and the same partial layout as k_gather_Hg_norms
__global__ __launch_bounds__(256) void k_grad_norm_partials(SpaDev d, const double * __restrict__ x, double * partial)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  double p[2] = {0.0, 0.0};
  if (t < d.n_free * 3) {
    const int i = t / 3, comp = t - i * 3;
    const double acc = d.g[t];
    const double v = x[3 * d.node_of_free[i] + comp];
    const double moved = comp == 2 ? d_normalize_angle(v - acc) : v - acc;
    p[0] = fabs(v - moved);
    p[1] = v * v;
  }
  block_reduce_store<2>(p, 1, partial + 2 * blockIdx.x);
}

// first half: everything up to H and g of this rank's edge block [e_lo, e_hi); a sharded caller sums H || g over the ranks
// before the second half
void spa_launch_step_and_linearize(const SpaDev & cur, const SpaDev & alt, const double * scale, const double * rhs, const double * x, double * step,
                                   double * delta, double * cand, double * partial, int e_lo, int e_hi, void * stream)
{
  hipStream_t s = (hipStream_t)stream;
  const int nbs = (kStepLanes * cur.n_free + 255) / 256, nbe = (cur.n_edges + 255) / 256, nbg = (3 * cur.n_free + 255) / 256;
  double * ps = partial, * pe = ps + 5 * (size_t)nbs, * pg = pe + nbe;
  const bool sharded = e_lo > 0 || e_hi < alt.n_edges;
  hipLaunchKernelGGL(k_step_fused, dim3(nbs), dim3(256), 0, s, cur, scale, rhs, x, step, delta, cand, ps);
  if (alt.n_edges > 0) {
    // sharded: the cost is still evaluated over all edges on every rank (E threads, microseconds)
    if (sharded) {
      hipLaunchKernelGGL(k_edge_lin<false>, dim3(nbe), dim3(256), 0, s, alt, cand, 0, alt.n_edges, pe);
      hipLaunchKernelGGL(k_edge_lin<true>, dim3(nbe), dim3(256), 0, s, alt, cand, e_lo, e_hi, (double *)nullptr);
    } else {
      hipLaunchKernelGGL(k_edge_lin<true>, dim3(nbe), dim3(256), 0, s, alt, cand, e_lo, e_hi, pe);
    }
  }
  const int nbh = alt.n_edges > 0 ? (alt.n_slots * 9 + 255) / 256 : 0;
  if (sharded) {
    if (nbh > 0) {hipLaunchKernelGGL(k_gather_H, dim3(nbh), dim3(256), 0, s, alt);}
    hipLaunchKernelGGL(k_gather_g, dim3(nbg), dim3(256), 0, s, alt);
  } else {
    hipLaunchKernelGGL(k_gather_Hg_norms, dim3(nbg + nbh), dim3(256), 0, s, alt, cand, pg, nbg);
  }
}

// second half: scal[3..10] from the partial sums (sharded: the gradient norms from the summed g first)
void spa_launch_step_scalars(const SpaDev & alt, const double * cand, double * partial, bool sharded, double * scal, void * stream, double * h_out,
                             int32_t * h_flag, const int32_t * fail_flag, int32_t seq)
{
  hipStream_t s = (hipStream_t)stream;
  const int nbs = (kStepLanes * alt.n_free + 255) / 256, nbe = (alt.n_edges + 255) / 256, nbg = (3 * alt.n_free + 255) / 256;
  double * ps = partial, * pe = ps + 5 * (size_t)nbs, * pg = pe + nbe;
  if (sharded) {hipLaunchKernelGGL(k_grad_norm_partials, dim3(nbg), dim3(256), 0, s, alt, cand, pg);}
  hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, s, ps, nbs, pe, alt.n_edges > 0 ? nbe : 0, pg, nbg, scal, h_out, h_flag, fail_flag, seq);
}

}  // namespace kh
