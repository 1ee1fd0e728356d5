// The round-3 form of k_potrf's 16 x 16 diagonal block: the pivot chain in the registers of lanes 0..15.  The solver no longer
// runs it (round 6 put the block on the matrix cores, csrc/spa_diag_block.hpp); it is kept here as the baseline that
// tools/diag_probe.hip times and checks the matrix-core form against.
#pragma once
#include "../slam_toolbox_amd/csrc/spa_diag_block.hpp"

#pragma clang fp contract(fast)

namespace kh
{

// lane n of every row of 16 lanes, to all lanes of that row: two v_mov_b32_dpp row_newbcast (full-rate VALU; a v_readlane
// pair goes through SGPRs and stalls on the VALU->SGPR->VALU hazards: 30 of them per pivot were most of a pivot's 230 ns)
template <int N>
__device__ __forceinline__ double row_bcast_c(double v)
{
  const long long b = __double_as_longlong(v);
  int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x150 + N, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x150 + N, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double row_bcast(double v, int n)      // n is a constant after unrolling
{
  switch (n) {
    case 0: return row_bcast_c<0>(v); case 1: return row_bcast_c<1>(v); case 2: return row_bcast_c<2>(v); case 3: return row_bcast_c<3>(v);
    case 4: return row_bcast_c<4>(v); case 5: return row_bcast_c<5>(v); case 6: return row_bcast_c<6>(v); case 7: return row_bcast_c<7>(v);
    case 8: return row_bcast_c<8>(v); case 9: return row_bcast_c<9>(v); case 10: return row_bcast_c<10>(v); case 11: return row_bcast_c<11>(v);
    case 12: return row_bcast_c<12>(v); case 13: return row_bcast_c<13>(v); case 14: return row_bcast_c<14>(v); default: return row_bcast_c<15>(v);
  }
}

// 16 x 16 Cholesky in the registers of lanes 0..15 (lane = row) with the identity riding along: xr = row `lane` of the
// identity on entry, row `lane` of L^-T on return (x L^T = e, right-looking: the L[c][j] a pivot broadcasts for the
// trailing update of the block are exactly the factors the rows of the identity need).
__device__ __forceinline__ bool diag_chain_inv(double (&row)[NB], double (&xr)[NB], int lane, double & rdiag)
{
  bool bad = false;
  rdiag = 1.0;
  const int l16 = lane & 15;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    double djj = row_bcast(row[j], j);
    if (!(djj > 0.0)) {bad = true; djj = 1.0;}
    double r = __builtin_amdgcn_rsq(djj);
    const double h = 0.5 * djj;
    r = r * (1.5 - h * r * r);
    r = r * (1.5 - h * r * r);
    row[j] = (l16 == j) ? djj * r : row[j] * r;
    if (l16 == j) {rdiag = r;}
    xr[j] *= r;
#pragma unroll
    for (int c = j + 1; c < NB; ++c) {
      const double lcj = row_bcast(row[j], c);          // L[c][j]
      row[c] -= row[j] * lcj;
      xr[c] -= xr[j] * lcj;
    }
  }
  return bad;
}

// Diagonal block `blk` of the LDS matrix (row stride LD): L over its lower part, the strictly upper part of L^-T over its
// strictly upper part, all of L^-T to xd (16 x XDS), the reciprocal pivots (= diagonal of L^-T) to rdv
__device__ __forceinline__ bool potrf_diag(double * blk, int LD, int lane, double * xd, double * rdv)
{
  double row[NB], xr[NB];
  const int l16 = lane & 15;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    row[c] = (lane < NB && c <= lane) ? blk[lane * LD + c] : ((lane >= NB && c == l16) ? 1.0 : 0.0);
    xr[c] = c == l16 ? 1.0 : 0.0;
  }
  double rdiag;
  const bool bad = diag_chain_inv(row, xr, lane, rdiag);
  if (lane < NB) {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      blk[lane * LD + c] = (c <= lane) ? row[c] : xr[c];
      xd[lane * XDS + c] = xr[c];
    }
    rdv[lane] = rdiag;
  }
  return bad && lane < NB;
}

}  // namespace kh
