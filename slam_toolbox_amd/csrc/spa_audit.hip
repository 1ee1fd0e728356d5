// Constraint audit of the SPA solver (hot path B): k_edge_audit, the leave-one-out test of every constraint against the resident
// covariances.  Launcher: spa_launch_edge_audit, called by spa_covariance.cpp; the linearisation in front of it is
// spa_linearize.hip's (spa_launch_edge_lin_all).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "spa_device.hpp"

#pragma clang fp contract(fast)

namespace kh
{

// ---------------------------------------------------------------------------------------------
// Constraint audit: the leave-one-out test of every constraint already in the graph, one thread per
// constraint.  lin = the audit's OWN linearisation of all edges (k_edge_lin<true> over [0, n_edges) into a buffer of the audit: a
// sharded solver's edge_lin holds zeros outside its shard), cov = the resident blocks of Sigma on H's pattern.  With r (3) the
// whitened, loss-weighted residual and A = [Ja Jb] (3 x 6):
//   H_e = A Sigma(ab, ab) A^T = Ja Saa Ja^T + Jb Sbb Jb^T + C + C^T, C = Ja Sab Jb^T      (a gauge end: no Jacobian, zero blocks)
//   M = I - H_e, lower Cholesky in the order 0, 1, 2 with pivots d0, d1, d2 (the values under the square roots)
// The factorisation stops at the first pivot that is not > min_redundancy (a NaN is not): the edge is unverifiable, chi2_loo = -1,
// and min_pivot = the smallest pivot formed so far (the failing one included; what would follow a pivot at rounding level is
// noise).  Otherwise chi2_loo = r^T x with L y = r, L^T x = y (x = M^-1 r is the leave-one-out residual itself).  Only the upper
// triangle of H_e is formed, so M is symmetric whatever the marginals' last bits are.  The (a, b) slot is found by scanning row
// free_of_node[a] of the pattern: no analysis state of the audit's own.  Everything stays in registers (27 + 21 doubles gathered,
// about 0.4 KB per edge); an edge's arithmetic does not depend on which other edges there are.
// out[4 e ..] = chi2, redundancy, min_pivot, chi2_loo; flag[e] = verifiable.
__device__ __forceinline__ void audit_quad(const double * __restrict__ JL, const double * __restrict__ S, const double * __restrict__ JR, double (&C)[9])
{
  double T[9];                     // T = JL S
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {T[3 * i + j] = (JL[3 * i] * S[j] + JL[3 * i + 1] * S[3 + j]) + JL[3 * i + 2] * S[6 + j];}
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {    // C = T JR^T
#pragma unroll
    for (int j = 0; j < 3; ++j) {C[3 * i + j] = (T[3 * i] * JR[3 * j] + T[3 * i + 1] * JR[3 * j + 1]) + T[3 * i + 2] * JR[3 * j + 2];}
  }
}

__global__ __launch_bounds__(256) void k_edge_audit(SpaDev d, const double * __restrict__ lin, const double * __restrict__ cov, double min_redundancy,
                                                    double * __restrict__ out, int32_t * __restrict__ flag)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= d.n_edges) {return;}
  const int fa = d.free_of_node[d.edge_a[e]], fb = d.free_of_node[d.edge_b[e]];
  const double * l = lin + 21 * (size_t)e;
  const double r0 = l[0], r1 = l[1], r2 = l[2];
  double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0;     // upper triangle of H_e
  bool on_pattern = true;
  double J[9], K[9], S[9], C[9];
  if (fa >= 0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) {J[q] = l[3 + q]; S[q] = cov[9 * (int64_t)d.bsr_diag_slot[fa] + q];}
    audit_quad(J, S, J, C);
    h00 += C[0]; h01 += C[1]; h02 += C[2]; h11 += C[4]; h12 += C[5]; h22 += C[8];
  }
  if (fb >= 0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) {K[q] = l[12 + q]; S[q] = cov[9 * (int64_t)d.bsr_diag_slot[fb] + q];}
    audit_quad(K, S, K, C);
    h00 += C[0]; h01 += C[1]; h02 += C[2]; h11 += C[4]; h12 += C[5]; h22 += C[8];
  }
  if (fa >= 0 && fb >= 0) {
    int slot = -1;
    for (int k = d.bsr_row_ptr[fa]; k < d.bsr_row_ptr[fa + 1]; ++k) {
      if (d.bsr_col[k] == fb) {slot = k; break;}
    }
    on_pattern = slot >= 0;
    if (on_pattern) {
#pragma unroll
      for (int q = 0; q < 9; ++q) {S[q] = cov[9 * (int64_t)slot + q];}
      audit_quad(J, S, K, C);
      h00 += C[0] + C[0]; h01 += C[1] + C[3]; h02 += C[2] + C[6]; h11 += C[4] + C[4]; h12 += C[5] + C[7]; h22 += C[8] + C[8];
    }
  }
  const double m00 = 1.0 - h00, m11 = 1.0 - h11, m22 = 1.0 - h22, m10 = -h01, m20 = -h02, m21 = -h12;
  const double nan = __builtin_nan("");
  double min_pivot = on_pattern ? m00 : nan, loo = -1.0;
  int ok = 0;
  if (min_pivot > min_redundancy) {
    const double l00 = sqrt(m00), l10 = m10 / l00, l20 = m20 / l00;
    const double d1 = m11 - l10 * l10;
    min_pivot = (d1 < min_pivot || d1 != d1) ? d1 : min_pivot;
    if (d1 > min_redundancy) {
      const double l11 = sqrt(d1), l21 = (m21 - l20 * l10) / l11;
      const double d2 = (m22 - l20 * l20) - l21 * l21;
      min_pivot = (d2 < min_pivot || d2 != d2) ? d2 : min_pivot;
      if (d2 > min_redundancy) {
        const double l22 = sqrt(d2);
        const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = ((r2 - l20 * y0) - l21 * y1) / l22;
        const double x2 = y2 / l22, x1 = (y1 - l21 * x2) / l11, x0 = ((y0 - l10 * x1) - l20 * x2) / l00;
        loo = (r0 * x0 + r1 * x1) + r2 * x2;
        ok = 1;
      }
    }
  }
  out[4 * (size_t)e] = (r0 * r0 + r1 * r1) + r2 * r2;
  out[4 * (size_t)e + 1] = (m00 + m11) + m22;
  out[4 * (size_t)e + 2] = min_pivot;
  out[4 * (size_t)e + 3] = loo;
  flag[e] = ok;
}
// x: the poses the resident covariances were computed at; audit.edge_lin / audit.edge_cost: buffers of the audit's own
void spa_launch_edge_audit(const SpaDev & audit, const double * x, const double * cov, double min_redundancy, double * out, int32_t * flag, void * stream)
{
  if (audit.n_edges <= 0) {return;}
  const dim3 grid((audit.n_edges + 255) / 256);
  spa_launch_edge_lin_all(audit, x, stream);
  hipLaunchKernelGGL(k_edge_audit, grid, dim3(256), 0, (hipStream_t)stream, audit, audit.edge_lin, cov, min_redundancy, out, flag);
}

}  // namespace kh
