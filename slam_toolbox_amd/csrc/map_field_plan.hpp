// The host rules of kh_map_field_*  without a device: the argument checks, the radius in cells and the limits,
// the cost table, the derived score, the refinement's candidate order, tie rule and state machine.  Needs no HIP header:
// tests/map_field_plan_check.cpp drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "map_localize_plan.hpp"     // fit_pose_ok: what kh_map_fit refuses of a pose

namespace kh
{
constexpr int32_t kMaxFieldRadius = 1024;             // cells: R, Rt and T
constexpr int64_t kMaxFieldSide = 32768;              // cells of a side: d2 < 2^31, a row of column distances fits 64 KiB of LDS
constexpr int64_t kMaxFieldCells = 1ll << 28;
constexpr int64_t kMaxUncappedSide = 4096;            // cells of a side when R == 0
constexpr uint16_t kFieldNoColumn = 0xFFFFu;          // k_field_columns: no obstacle in this column (within R)
constexpr int32_t kMaxRefineHalvings = 32, kMaxRefineRounds = 4096;
constexpr int32_t kRefineCandidates = 27, kRefineCentre = 13;
// the counters of the field and of a scored pose, in the order the kernels keep them
enum : int32_t {kFieldObstacles = 0, kFieldFar = 1, kFieldMaxD2 = 2, kFieldCounters = 3};
enum : int32_t {kScoreKept = 0, kScoreHit = 1, kScoreInside = 2, kScoreNear = 3, kScoreSum = 4, kScoreCounters = 5};

// ceil(metres * scale) cells, or -1 where metres is not finite or < 0 or the radius lies above kMaxFieldRadius
inline int32_t field_radius(double metres, double scale)
{
  if (!std::isfinite(metres) || metres < 0.0) {return -1;}
  const double cells = std::ceil(metres * scale);
  return cells <= static_cast<double>(kMaxFieldRadius) ? static_cast<int32_t>(cells) : -1;
}

// what kh_map_field_create takes of a well-formed view and its parameters before a device is looked for
enum : int32_t {kFieldOk = 0, kFieldBadDistance = 1, kFieldBadObstacles = 2, kFieldSideTooLong = 3, kFieldTooManyCells = 4, kFieldUncappedTooLong = 5};
inline int32_t field_check(int32_t width, int32_t height, double scale, const kh_map_field_params & p, int32_t * radius)
{
  const int32_t r = field_radius(p.max_distance, scale);
  if (r < 0) {return kFieldBadDistance;}
  if (p.obstacles < KH_FIELD_OBSTACLE_OCCUPIED || p.obstacles > KH_FIELD_OBSTACLE_NOT_FREE) {return kFieldBadObstacles;}
  if (width > kMaxFieldSide || height > kMaxFieldSide) {return kFieldSideTooLong;}
  if (static_cast<int64_t>(width) * height > kMaxFieldCells) {return kFieldTooManyCells;}
  if (r == 0 && (width > kMaxUncappedSide || height > kMaxUncappedSide)) {return kFieldUncappedTooLong;}
  *radius = r;
  return kFieldOk;
}

// the row stride of the field's own arrays (cells, column distances, values, costs): whole groups of four cells
inline int32_t field_stride(int32_t width) {return (width + 3) & ~3;}

// ---- costmap values ----
// what is taken of the parameters whatever the scale
inline bool inflation_params_ok(const kh_inflation_params & p)
{
  return std::isfinite(p.inscribed_radius) && p.inscribed_radius >= 0.0 && std::isfinite(p.inflation_radius) && std::isfinite(p.cost_scaling_factor) &&
         p.cost_scaling_factor >= 0.0 && p.inscribed_radius <= p.inflation_radius && p.track_unknown >= 0 && p.track_unknown <= 1 &&
         p.inflate_unknown >= 0 && p.inflate_unknown <= 1;
}
// Rt, or -1 where the parameters or the scale are refused or Rt lies above kMaxFieldRadius
inline int32_t inflation_radius_cells(const kh_inflation_params & p, double scale)
{
  if (!inflation_params_ok(p) || !std::isfinite(scale) || !(scale > 0.0)) {return -1;}
  return field_radius(p.inflation_radius, scale);
}
// entry d2 of the table
inline uint8_t inflation_cost(const kh_inflation_params & p, double scale, uint32_t d2)
{
  if (d2 == 0u) {return 254;}
  const double m = std::sqrt(static_cast<double>(d2)) / scale;
  if (m <= p.inscribed_radius) {return 253;}
  if (m <= p.inflation_radius) {return static_cast<uint8_t>(252.0 * std::exp(-p.cost_scaling_factor * (m - p.inscribed_radius)));}
  return 0;
}
inline std::vector<uint8_t> inflation_table(const kh_inflation_params & p, double scale, int32_t rt)
{
  std::vector<uint8_t> table(static_cast<size_t>(rt) * static_cast<size_t>(rt) + 1);
  for (size_t d2 = 0; d2 < table.size(); ++d2) {table[d2] = inflation_cost(p, scale, static_cast<uint32_t>(d2));}
  return table;
}

// ---- the endpoint score ----
// T, or -1 where refused: truncate_cells outside 0 .. kMaxFieldRadius, or both it and the field's R zero
inline int32_t score_truncation(int32_t truncate_cells, int32_t radius)
{
  if (truncate_cells < 0 || truncate_cells > kMaxFieldRadius) {return -1;}
  const int32_t t = truncate_cells > 0 ? truncate_cells : radius;
  return t > 0 ? t : -1;
}
// the five sums of a pose -> kh_field_score
inline kh_field_score score_derive(const uint64_t c[kScoreCounters], int32_t t)
{
  kh_field_score s;
  s.n_kept = static_cast<int32_t>(c[kScoreKept]); s.n_hit = static_cast<int32_t>(c[kScoreHit]);
  s.n_inside = static_cast<int32_t>(c[kScoreInside]); s.n_near = static_cast<int32_t>(c[kScoreNear]);
  const uint64_t t2 = static_cast<uint64_t>(t) * static_cast<uint64_t>(t);
  s.sum_d2 = c[kScoreSum];
  s.cost = s.sum_d2 + (c[kScoreHit] - c[kScoreNear]) * t2;
  s.score = s.n_hit > 0 ? 1.0 - static_cast<double>(s.cost) / (static_cast<double>(s.n_hit) * static_cast<double>(t2)) : 0.0;
  return s;
}

// ---- the refinement ----
inline bool refine_params_ok(const kh_field_refine_params & p)
{
  return std::isfinite(p.step_xy) && p.step_xy > 0.0 && std::isfinite(p.step_heading) && p.step_heading >= 0.0 && p.n_halvings >= 0 &&
         p.n_halvings <= kMaxRefineHalvings && p.max_rounds >= 1 && p.max_rounds <= kMaxRefineRounds && p.truncate_cells >= 0 &&
         p.truncate_cells <= kMaxFieldRadius;
}
// candidate c of a start at `pose` with steps (s, s, a)
inline void refine_candidate(const double pose[3], double s, double a, int32_t c, double out[3])
{
  out[0] = pose[0] + static_cast<double>(c % 3 - 1) * s;
  out[1] = pose[1] + static_cast<double>(c / 3 % 3 - 1) * s;
  out[2] = pose[2] + static_cast<double>(c / 9 - 1) * a;
}
// the candidate of least cost: the centre if it is among the least, else the smallest c
inline int32_t refine_pick(const uint64_t cost[kRefineCandidates])
{
  int32_t best = kRefineCentre;
  for (int32_t c = kRefineCandidates - 1; c >= 0; --c) {
    if (cost[c] < cost[best] || (cost[c] == cost[best] && best != kRefineCentre)) {best = c;}
  }
  return best;
}
// One start.  begin() takes the score where it stands; then, while running(): candidates() writes the 27 poses of the next round, or
// ends the start (LEFT_LATTICE) where one of them is refused; advance() takes their costs.
struct RefineStart
{
  double pose[3], s, a;
  uint64_t cost_start = 0, cost = 0;
  int32_t n_hit = 0, rounds = 0, halvings = 0, status = -1;         // -1: still running
  void begin(const double p[3], const kh_field_refine_params & q, uint64_t cost_here, int32_t hits)
  {
    pose[0] = p[0]; pose[1] = p[1]; pose[2] = p[2]; s = q.step_xy; a = q.step_heading;
    cost_start = cost = cost_here; n_hit = hits; rounds = 0; halvings = 0;
    status = q.max_rounds < 1 ? KH_REFINE_MAX_ROUNDS : -1;
  }
  bool running() const {return status < 0;}
  bool candidates(double ax, double ay, double scale, double out[3 * kRefineCandidates])
  {
    for (int32_t c = 0; c < kRefineCandidates; ++c) {
      refine_candidate(pose, s, a, c, out + 3 * c);
      if (!fit_pose_ok(out + 3 * c, ax, ay, scale)) {status = KH_REFINE_LEFT_LATTICE; return false;}
    }
    return true;
  }
  void advance(const uint64_t costs[kRefineCandidates], const kh_field_refine_params & q)
  {
    const int32_t best = refine_pick(costs);
    ++rounds;
    cost = costs[best];
    if (best == kRefineCentre) {
      if (halvings == q.n_halvings) {status = KH_REFINE_CONVERGED; return;}
      s *= 0.5; a *= 0.5; ++halvings;
    } else {
      double next[3];
      refine_candidate(pose, s, a, best, next);
      pose[0] = next[0]; pose[1] = next[1]; pose[2] = next[2];
    }
    if (rounds >= q.max_rounds) {status = KH_REFINE_MAX_ROUNDS;}
  }
  kh_field_refined result() const
  {
    kh_field_refined r;
    r.pose[0] = pose[0]; r.pose[1] = pose[1]; r.pose[2] = pose[2];
    r.cost_start = cost_start; r.cost = cost; r.n_hit = n_hit; r.rounds = rounds; r.halvings = halvings; r.status = status;
    return r;
  }
};
}  // namespace kh
