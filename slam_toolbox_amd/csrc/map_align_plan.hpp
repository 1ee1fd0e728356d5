// The host rules of kh_map_raycast's default and of kh_map_align without a device: the reading of a beam that
// found nothing, the choice of the probes, the corrections and their order, the candidates' sensor poses, the ranking.  Needs no HIP
// header: tests/map_align_plan_check.cpp drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "map_localize_plan.hpp"

namespace kh
{
// The reading of a beam that found nothing.  A reading EQUAL to range_threshold is a valid point for LocalizedRangeScan::Update (the
// inclusive InRange(minimum_range, range_threshold)) and would paint a wall where the map ended; the next double above it is dropped
// from the point readings and, below maximum_range, still clears the beam in AddScan.  Where no such reading exists: NaN.
inline double ray_no_return(double range_threshold, double maximum_range)
{
  const double above = std::nextafter(range_threshold, std::numeric_limits<double>::infinity());
  return above < maximum_range ? above : std::numeric_limits<double>::quiet_NaN();
}

// ---- corrections: tests/merge_rule.py's arithmetic (cos and sin of an angle each called on its own) ----
struct AlignRigid
{
  double x = 0.0, y = 0.0, yaw = 0.0, c = 1.0, s = 0.0;
  AlignRigid() = default;
  AlignRigid(double x_, double y_, double yaw_) : x(x_), y(y_), yaw(yaw_)
  {
    double (* volatile own_cos)(double) = std::cos;      // (not merged into one sincos call)
    double (* volatile own_sin)(double) = std::sin;
    c = own_cos(yaw_); s = own_sin(yaw_);
  }
  void pose(const double in[3], double out[3]) const
  {
    out[0] = (c * in[0] - s * in[1]) + x;
    out[1] = (s * in[0] + c * in[1]) + y;
    out[2] = mapper::normalize_angle(in[2] + yaw);
  }
};
inline AlignRigid align_compose(const AlignRigid & a, const AlignRigid & b)
{
  return AlignRigid(a.x + (a.c * b.x - a.s * b.y), a.y + (a.s * b.x + a.c * b.y), mapper::normalize_angle(a.yaw + b.yaw));
}
inline AlignRigid align_inverse(const AlignRigid & a)
{
  const AlignRigid r(0.0, 0.0, mapper::normalize_angle(-a.yaw));
  return AlignRigid(-(r.c * a.x - r.s * a.y), -(r.s * a.x + r.c * a.y), r.yaw);
}
// C = P . inverse(Q): the probe, at robot pose Q in the moving map, stands at P in the target's
inline void align_correction(const double p[3], const double q[3], double out[3])
{
  const AlignRigid c = align_compose(AlignRigid(p[0], p[1], p[2]), align_inverse(AlignRigid(q[0], q[1], q[2])));
  out[0] = c.x; out[1] = c.y; out[2] = c.yaw;
}

// ---- the probes: the n_probes seeds with the most HIT beams, ties to the lower seed index, none without a HIT ----
inline std::vector<int32_t> align_pick_probes(const std::vector<int32_t> & hits, int32_t n_probes)
{
  std::vector<int32_t> order;
  for (size_t k = 0; k < hits.size(); ++k) {
    if (hits[k] > 0) {order.push_back(static_cast<int32_t>(k));}
  }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {return hits[static_cast<size_t>(a)] > hits[static_cast<size_t>(b)];});
  if (order.size() > static_cast<size_t>(n_probes > 0 ? n_probes : 0)) {order.resize(static_cast<size_t>(n_probes > 0 ? n_probes : 0));}
  return order;
}

// ---- the candidates: `initial`, then the probes in pick order, each one's hypotheses in rank order ----
inline kh_map_align_cand align_candidate(const double correction[3], int32_t probe_seed, int32_t hypothesis, double fine_response)
{
  kh_map_align_cand c;
  std::memset(&c, 0, sizeof(c));
  std::copy(correction, correction + 3, c.correction);
  c.probe_seed = probe_seed; c.hypothesis = hypothesis; c.fine_response = fine_response;
  return c;
}

// known >= min_known first, then score descending, agree descending, index ascending (kh_merge_align's ranking)
inline bool align_before(const kh_map_align_cand & a, const kh_map_align_cand & b)
{
  if (a.enough != b.enough) {return a.enough > b.enough;}
  if (a.fit.score != b.fit.score) {return a.fit.score > b.fit.score;}
  if (a.fit.agree != b.fit.agree) {return a.fit.agree > b.fit.agree;}
  return a.index < b.index;
}
// the summed counters of every candidate (kFitCounters each) -> fit, index, enough; then the ranking
inline void align_rank(std::vector<kh_map_align_cand> & cands, const std::vector<uint64_t> & sums, uint64_t min_known)
{
  for (size_t k = 0; k < cands.size(); ++k) {
    cands[k].fit = fit_derive(&sums[k * kFitCounters]);
    cands[k].index = static_cast<int32_t>(k);
    cands[k].enough = cands[k].fit.known >= min_known ? 1 : 0;
  }
  std::sort(cands.begin(), cands.end(), align_before);
}

// what kh_map_align takes of its parameters before a device is looked for
inline bool align_params_ok(const kh_map_align_params & p)
{
  return std::isfinite(p.probe_spacing) && p.probe_spacing > 0 && p.n_probes >= 1 && p.top_k >= 1 && p.max_unknown >= -1 &&
         std::isfinite(p.initial[0]) && std::isfinite(p.initial[1]) && std::isfinite(p.initial[2]) && relocalize_params_ok(p.relocalize);
}
}  // namespace kh
