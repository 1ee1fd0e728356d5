// Device code shared by the kernel files of the pose-graph SPA solver (hot path B), one file per concern:
//   spa_linearize.hip     K5: residuals, Jacobians, the normal equations, the scalars of an LM step
//   spa_factor_front.hip  K6, any-size route: one workgroup per front (k_extend_add, k_factor, k_backward)
//   spa_potrf.hip         K6, level pipeline: the pivot blocks (k_potrf; its 16 x 16 diagonal block: spa_diag_block.hpp)
//   spa_update.hip        K6, level pipeline: k_trsm, k_syrk, k_front_update, k_backward3 and the self-cleaning helpers
//   spa_selinv.hip        selected inverse of the factor, the marginal blocks on H's pattern
//   spa_cov_columns.hip   block columns of the inverse, relative and difference covariances
//   spa_audit.hip         the constraint audit
// Only what more than one of them needs lives here.  No kernel is shared between two files: each file launches its own (the
// launchers are declared in spa_internal.hpp, the one helper the files call among themselves at the end of this header).
//
// Numerics are FP64 with FMA contraction allowed (the parity bar of the solver is 1e-9 against the CPU restatement, not bit
// equality).  The build passes -ffp-contract=off, so the pragma below is what allows it: it holds from here to the end of every
// file that includes this header, and every kernel file repeats it behind its includes so that the rule is visible where the
// arithmetic is.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "spa_internal.hpp"

#pragma clang fp contract(fast)

namespace kh
{

constexpr int NB = 16;                     // panel width of every blocked kernel = side of a matrix-core tile
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int kPotrfMaxNs = 128;           // pivots of a front of the level pipeline (the symbolic analysis splits larger supernodes)

// ---- children's update matrices, read in place (no extend-add pass) ----
// child number s of a front: the first three sit in the front's own descriptor, further ones (rare: a separator above
// several disconnected pieces) come from the child list
__device__ __forceinline__ ChildInfo child_info(const SpaDev & d, const FrontDesc & fd, int s)
{
  if (s == 0) {return fd.ch[0];}
  if (s == 1) {return fd.ch[1];}
  if (s == 2) {return fd.ch[2];}
  const FrontDesc & c = d.desc[d.child_list[fd.child_ptr + s]];
  ChildInfo ci;
  ci.off = c.off; ci.m = c.m; ci.ns = c.ns; ci.rows_ptr = c.rows_ptr; ci.pad = 0;
  return ci;
}

// round 6 (Symbolic::scatter_mode): children read in place come first in the child list
__device__ __forceinline__ int front_nkids(const SpaDev & d, const FrontDesc & fd)
{
  return d.gather ? fd.child_end - fd.child_ptr : (d.scatter ? (fd.flags >> 8) : 0);
}
// buffer B of a front, or nullptr when no child adds into it
__device__ __forceinline__ const double * front_b(const SpaDev & d, const FrontDesc & fd)
{
  return (d.scatter && (fd.flags & 4)) ? d.fronts_b + fd.off : nullptr;
}

// entry (i, j), i >= j (scalar positions in the parent front), of one child's update matrix, 0 where the child has none
__device__ __forceinline__ double gather_entry(const double * __restrict__ fronts, const ChildInfo & c, const int32_t * __restrict__ inv, int i, int j)
{
  const int in = i / 3, jn = j / 3;
  const int a = inv[in], b = inv[jn];
  const bool ok = a >= 0 && b >= 0;
  const int64_t at = ok ? (int64_t)(c.ns + 3 * a + (i - 3 * in)) + (int64_t)(c.ns + 3 * b + (j - 3 * jn)) * c.m : 0;
  const double v = fronts[c.off + at];
  return ok ? v : 0.0;
}

// ---- a 16 x 16 tile of a product with operands straight from memory (selected inverse, covariance columns) ----
// Operand and result places of v_mfma_f64_16x16x4: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register r of lane l
// is D[(l >> 4) + 4 r][l & 15].
// a(i, k), b(k, j): entries of the 16 x K and K x 16 operands (0 outside the matrices); [k_lo, k_hi), k_lo a multiple of 4
template <class FA, class FB>
__device__ __forceinline__ v4d selinv_product(FA a, FB b, int k_lo, int k_hi, int lane)
{
  const int lr = lane & 15, lk = lane >> 4;
  v4d acc = v4d{0.0, 0.0, 0.0, 0.0}, other = v4d{0.0, 0.0, 0.0, 0.0};     // two chains of dependent matrix-core operations, as k_potrf's ll_accumulate
  int k = k_lo;
  for (; k + 4 < k_hi; k += 8) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a(lr, k + lk), b(k + lk, lr), acc, 0, 0, 0);
    other = __builtin_amdgcn_mfma_f64_16x16x4f64(a(lr, k + 4 + lk), b(k + 4 + lk, lr), other, 0, 0, 0);
  }
  if (k < k_hi) {acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a(lr, k + lk), b(k + lk, lr), acc, 0, 0, 0);}
  return acc + other;
}

// spa_linearize.hip, for spa_audit.hip: k_edge_lin<true> over ALL edges of `d` at x, into d.edge_lin / d.edge_cost
void spa_launch_edge_lin_all(const SpaDev & d, const double * x, void * stream);

}  // namespace kh
