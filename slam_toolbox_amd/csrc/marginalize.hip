// Marginalizing node removal on the device: one launch composes the constraints of a ROUND of leaving nodes through them into
// constraints among their neighbours (the rule is restated in numpy in tests/marginalize_rule.py, and the
// arithmetic below follows it operation by operation -- the library is built with -ffp-contract=off).
//
// One wave per node, one lane per neighbour entry (at most 64).  A lane fuses its entry's parallel constraints, the wave agrees on
// the hub (largest determinant of the information, ties to the lowest id) by a butterfly of cross-lane moves, the hub's lane hands
// its oriented constraint to the others through v_readlane (a double as two 32-bit halves), and every other lane composes
// inverse(v -> hub) (+) (v -> its neighbour), fuses the result into the existing hub-neighbour constraint where the host listed
// one, and stores 9 doubles at the slot the host fixed (prefix over d - 1, rank among the non-hub lanes).  All 3 x 3 float64
// arithmetic is in registers: no LDS, no atomics.  The closed neighbourhoods of a round's nodes are disjoint, so no two lanes of
// the launch touch the same constraint.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "marginalize.hpp"

namespace kh
{
namespace
{

struct M3 {double a[9];};            // row-major 3 x 3
struct V3 {double a[3];};

__device__ __forceinline__ double normalize_angle(double th)      // ceres_utils.h:27-32: [-pi, pi)
{
  const double pi = 3.14159265358979323846;
  return th - 2.0 * pi * floor((th + pi) / (2.0 * pi));
}

__device__ __forceinline__ M3 mm(const M3 & A, const M3 & B)
{
  M3 C;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {C.a[3 * i + j] = A.a[3 * i] * B.a[j] + A.a[3 * i + 1] * B.a[3 + j] + A.a[3 * i + 2] * B.a[6 + j];}
  }
  return C;
}

__device__ __forceinline__ V3 mv(const M3 & A, const V3 & x)
{
  V3 y;
#pragma unroll
  for (int i = 0; i < 3; ++i) {y.a[i] = A.a[3 * i] * x.a[0] + A.a[3 * i + 1] * x.a[1] + A.a[3 * i + 2] * x.a[2];}
  return y;
}

__device__ __forceinline__ M3 transpose(const M3 & A)
{
  M3 T;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {T.a[3 * i + j] = A.a[3 * j + i];}
  }
  return T;
}

// the symmetric matrix that has M's upper triangle
__device__ __forceinline__ M3 mirror(M3 M) {M.a[3] = M.a[1]; M.a[6] = M.a[2]; M.a[7] = M.a[5]; return M;}

__device__ __forceinline__ M3 congruence(const M3 & J, const M3 & S) {return mirror(mm(mm(J, S), transpose(J)));}

__device__ __forceinline__ double det3(const M3 & m)
{
  return m.a[0] * (m.a[4] * m.a[8] - m.a[5] * m.a[5]) - m.a[1] * (m.a[1] * m.a[8] - m.a[5] * m.a[2]) + m.a[2] * (m.a[1] * m.a[5] - m.a[4] * m.a[2]);
}

// inverse of a symmetric 3 x 3 by the cofactors of its upper triangle
__device__ __forceinline__ M3 inv3(const M3 & m)
{
  const double c00 = m.a[4] * m.a[8] - m.a[5] * m.a[5];
  const double c01 = m.a[2] * m.a[5] - m.a[1] * m.a[8];
  const double c02 = m.a[1] * m.a[5] - m.a[2] * m.a[4];
  const double c11 = m.a[0] * m.a[8] - m.a[2] * m.a[2];
  const double c12 = m.a[1] * m.a[2] - m.a[0] * m.a[5];
  const double c22 = m.a[0] * m.a[4] - m.a[1] * m.a[1];
  const double r = 1.0 / (m.a[0] * c00 + m.a[1] * c01 + m.a[2] * c02);
  M3 o;
  o.a[0] = c00 * r; o.a[1] = c01 * r; o.a[2] = c02 * r;
  o.a[3] = c01 * r; o.a[4] = c11 * r; o.a[5] = c12 * r;
  o.a[6] = c02 * r; o.a[7] = c12 * r; o.a[8] = c22 * r;
  return o;
}

// (z, Sigma) of b in a's frame -> of a in b's frame
__device__ __forceinline__ void inverse(V3 & z, M3 & S)
{
  const double c = cos(z.a[2]), s = sin(z.a[2]);
  const double x = z.a[0], y = z.a[1];
  M3 J;
  J.a[0] = -c; J.a[1] = -s; J.a[2] = s * x - c * y;
  J.a[3] = s; J.a[4] = -c; J.a[5] = c * x + s * y;
  J.a[6] = 0.0; J.a[7] = 0.0; J.a[8] = -1.0;
  z.a[0] = -(c * x + s * y); z.a[1] = -(c * y - s * x); z.a[2] = -z.a[2];
  S = congruence(J, S);
}

// (z1, S1) (+) (z2, S2), the first term's covariance weighted w
__device__ __forceinline__ void compose(const V3 & z1, const M3 & S1, const V3 & z2, const M3 & S2, double w, V3 & z, M3 & S)
{
  const double c = cos(z1.a[2]), s = sin(z1.a[2]);
  const double x = z2.a[0], y = z2.a[1];
  z.a[0] = z1.a[0] + (c * x - s * y); z.a[1] = z1.a[1] + (s * x + c * y); z.a[2] = normalize_angle(z1.a[2] + z2.a[2]);
  M3 J1, J2;
  J1.a[0] = 1.0; J1.a[1] = 0.0; J1.a[2] = -(s * x) - c * y;
  J1.a[3] = 0.0; J1.a[4] = 1.0; J1.a[5] = c * x - s * y;
  J1.a[6] = 0.0; J1.a[7] = 0.0; J1.a[8] = 1.0;
  J2.a[0] = c; J2.a[1] = -s; J2.a[2] = 0.0;
  J2.a[3] = s; J2.a[4] = c; J2.a[5] = 0.0;
  J2.a[6] = 0.0; J2.a[7] = 0.0; J2.a[8] = 1.0;
  const M3 A = congruence(J1, S1), B = congruence(J2, S2);
#pragma unroll
  for (int k = 0; k < 9; ++k) {S.a[k] = w * A.a[k] + B.a[k];}
  S = mirror(S);
}

// the same constraint (z, Omega) stored the other way round
__device__ __forceinline__ void flip(V3 & z, M3 & O)
{
  M3 S = inv3(O);
  inverse(z, S);
  O = inv3(S);
}

// (z2, O2) fused onto (z1, O1), both on the same ordered pair
__device__ __forceinline__ void fuse(V3 & z1, M3 & O1, const V3 & z2, const M3 & O2)
{
  M3 O;
#pragma unroll
  for (int k = 0; k < 9; ++k) {O.a[k] = O1.a[k] + O2.a[k];}
  O = mirror(O);
  V3 d;
  d.a[0] = z2.a[0] - z1.a[0]; d.a[1] = z2.a[1] - z1.a[1]; d.a[2] = normalize_angle(z2.a[2] - z1.a[2]);
  const V3 v = mv(O2, d);
  const V3 r = mv(inv3(O), v);
  z1.a[0] = z1.a[0] + r.a[0]; z1.a[1] = z1.a[1] + r.a[1]; z1.a[2] = z1.a[2] + r.a[2];
  O1 = O;
}

__device__ __forceinline__ void load9(const double * __restrict__ p, V3 & z, M3 & O)
{
  z.a[0] = p[0]; z.a[1] = p[1]; z.a[2] = p[2];
  O.a[0] = p[3]; O.a[1] = p[4]; O.a[2] = p[5]; O.a[4] = p[6]; O.a[5] = p[7]; O.a[8] = p[8];
  O = mirror(O);
}

// a double of lane `src` (wave-uniform) to every lane, as two 32-bit halves
__device__ __forceinline__ double read_lane_f64(double v, int src)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double shfl_xor_f64(double v, int mask)
{
  const int lo = __shfl_xor(__double2loint(v), mask, 64);
  const int hi = __shfl_xor(__double2hiint(v), mask, 64);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(256) void k_marginalize_round(MargDev g)
{
  const int lane = threadIdx.x & 63;
  const int node = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (node >= g.n_nodes) {return;}                             // (the whole wave)
  const int e0 = g.ent_ptr[node];
  const int d = g.ent_ptr[node + 1] - e0;                      // 2 .. 64 (the host refuses anything else)
  const bool active = lane < d;
  V3 z = {{0.0, 0.0, 0.0}};
  M3 O = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
  int dir = 0, id = INT_MAX;
  double det = -__builtin_huge_val();
  if (active) {
    // 1. the entry: its first constraint with the later parallel ones fused onto it, in constraint order
    const int k0 = g.con_ptr[e0 + lane], k1 = g.con_ptr[e0 + lane + 1];
    load9(g.con_d + 9ll * k0, z, O);
    dir = g.con_dir[k0];
    for (int k = k0 + 1; k < k1; ++k) {
      V3 z2; M3 O2;
      load9(g.con_d + 9ll * k, z2, O2);
      if (g.con_dir[k] != dir) {flip(z2, O2);}
      fuse(z, O, z2, O2);
    }
    id = g.ent_id[e0 + lane];
    det = det3(O);
  }
  // 2. the hub: largest determinant, ties to the lowest id (ids are distinct among the active lanes)
  double best = det; int best_id = id, best_lane = lane;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const double o_det = shfl_xor_f64(best, m);
    const int o_id = __shfl_xor(best_id, m, 64), o_lane = __shfl_xor(best_lane, m, 64);
    if (o_det > best || (o_det == best && (o_id < best_id || (o_id == best_id && o_lane < best_lane)))) {best = o_det; best_id = o_id; best_lane = o_lane;}
  }
  const int h = __builtin_amdgcn_readfirstlane(best_lane);
  // 3. oriented node -> neighbour, as a covariance
  M3 S = inv3(O);
  if (dir != 0) {inverse(z, S);}
  // the hub's lane hands over its constraint; every lane inverts it for itself (the same arithmetic, the same bits)
  V3 zh; M3 Sh;
#pragma unroll
  for (int k = 0; k < 3; ++k) {zh.a[k] = read_lane_f64(z.a[k], h);}
  Sh.a[0] = read_lane_f64(S.a[0], h); Sh.a[1] = read_lane_f64(S.a[1], h); Sh.a[2] = read_lane_f64(S.a[2], h);
  Sh.a[4] = read_lane_f64(S.a[4], h); Sh.a[5] = read_lane_f64(S.a[5], h); Sh.a[8] = read_lane_f64(S.a[8], h);
  Sh = mirror(Sh);
  inverse(zh, Sh);
  if (!active || lane == h) {return;}
  // 4. hub -> neighbour, the hub's term weighted d - 1
  V3 zn; M3 Sn;
  compose(zh, Sh, z, S, static_cast<double>(d - 1), zn, Sn);
  M3 On = inv3(Sn);
  // 5. an existing constraint between the hub and the neighbour takes the new one in and keeps its direction
  const int lo = lane < h ? lane : h, hi = lane < h ? h : lane;
  int found = -1;
  for (int p = g.pair_ptr[node]; p < g.pair_ptr[node + 1]; ++p) {
    const int w = g.pair_ent[p];
    if ((w & 0xff) == lo && ((w >> 8) & 0xff) == hi) {
      found = p;
      const bool from_hub = ((w >> 16) & 1) == 0 ? lo == h : hi == h;
      if (!from_hub) {flip(zn, On);}
      V3 ze; M3 Oe;
      load9(g.pair_d + 9ll * p, ze, Oe);
      fuse(ze, Oe, zn, On);
      zn = ze; On = Oe;
      break;
    }
  }
  const int slot = g.out_ptr[node] + (lane < h ? lane : lane - 1);
  double * o = g.out_d + 9ll * slot;
  o[0] = zn.a[0]; o[1] = zn.a[1]; o[2] = zn.a[2];
  o[3] = On.a[0]; o[4] = On.a[1]; o[5] = On.a[2]; o[6] = On.a[4]; o[7] = On.a[5]; o[8] = On.a[8];
  g.out_i[2 * slot] = h; g.out_i[2 * slot + 1] = found;
}

}  // namespace

void marginalize_launch_round(const MargDev & d, void * stream)
{
  if (d.n_nodes <= 0) {return;}
  hipLaunchKernelGGL(k_marginalize_round, dim3((d.n_nodes + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), d);
}

}  // namespace kh
