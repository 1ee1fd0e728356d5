// The host rules of the distance field (slam_toolbox_amd/csrc/map_field_plan.hpp) without a device: reads one case per line on
// stdin, prints one result per line.  tests/test_map_field_plan.py makes the cases and holds the expectations.
//
//   radius metres scale                                 -> R, or -1
//   field width height scale max_distance obstacles     -> "0 R stride", or the refusal 1 .. 5
//   table inscribed inflation factor track inflate scale -> "-1", or n and the n entries
//   truncation truncate_cells R                         -> T, or -1
//   derive kept hit inside near sum T                   -> cost and the score
//   refine_args step_xy step_heading n_halvings max_rounds truncate_cells -> 0 / 1
//   candidates x y h s a                                -> the 27 candidates, 3 doubles each
//   pick (27 costs)                                     -> the index
//   machine x y h step_xy step_heading n_halvings max_rounds tx ty th scale
//                                                       -> pose cost_start cost n_hit rounds halvings status of one start driven with
//                                                          the scripted cost floor(64 |x - tx| + .5) + floor(64 |y - ty| + .5) +
//                                                          floor(1024 |h - th| + .5) on the lattice of anchor (0, 0) and `scale`
//
// Doubles are read with strtod and printed with %a, so they pass bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../slam_toolbox_amd/csrc/map_field_plan.hpp"

using namespace kh;

namespace
{
double real(std::istringstream & in) {std::string t; in >> t; return std::strtod(t.c_str(), nullptr);}
long long whole(std::istringstream & in) {long long v = 0; in >> v; return v;}
uint64_t scripted(const double p[3], const double target[3])
{
  return static_cast<uint64_t>(std::floor(64.0 * std::fabs(p[0] - target[0]) + 0.5) + std::floor(64.0 * std::fabs(p[1] - target[1]) + 0.5) +
         std::floor(1024.0 * std::fabs(p[2] - target[2]) + 0.5));
}
}  // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "radius") {
      const double metres = real(in), scale = real(in);
      std::printf("%d\n", field_radius(metres, scale));
    } else if (what == "field") {
      const int32_t width = (int32_t)whole(in), height = (int32_t)whole(in);
      const double scale = real(in);
      kh_map_field_params p;
      std::memset(&p, 0, sizeof(p));
      p.max_distance = real(in); p.obstacles = (int32_t)whole(in);
      int32_t radius = -7;
      const int32_t rc = field_check(width, height, scale, p, &radius);
      if (rc) {std::printf("%d\n", rc);} else {std::printf("0 %d %d\n", radius, field_stride(width));}
    } else if (what == "table") {
      kh_inflation_params p;
      std::memset(&p, 0, sizeof(p));
      p.inscribed_radius = real(in); p.inflation_radius = real(in); p.cost_scaling_factor = real(in);
      p.track_unknown = (int32_t)whole(in); p.inflate_unknown = (int32_t)whole(in);
      const double scale = real(in);
      const int32_t rt = inflation_radius_cells(p, scale);
      if (rt < 0) {std::printf("-1\n"); continue;}
      const std::vector<uint8_t> t = inflation_table(p, scale, rt);
      std::printf("%zu", t.size());
      for (uint8_t v : t) {std::printf(" %u", (unsigned)v);}
      std::printf("\n");
    } else if (what == "truncation") {
      const int32_t t = (int32_t)whole(in), r = (int32_t)whole(in);
      std::printf("%d\n", score_truncation(t, r));
    } else if (what == "derive") {
      uint64_t c[kScoreCounters];
      for (uint64_t & v : c) {unsigned long long t = 0; in >> t; v = t;}
      const kh_field_score s = score_derive(c, (int32_t)whole(in));
      std::printf("%llu %a %d %d %d %d %llu\n", (unsigned long long)s.cost, s.score, s.n_kept, s.n_hit, s.n_inside, s.n_near, (unsigned long long)s.sum_d2);
    } else if (what == "refine_args") {
      kh_field_refine_params p;
      std::memset(&p, 0, sizeof(p));
      p.step_xy = real(in); p.step_heading = real(in);
      p.n_halvings = (int32_t)whole(in); p.max_rounds = (int32_t)whole(in); p.truncate_cells = (int32_t)whole(in);
      std::printf("%d\n", refine_params_ok(p) ? 1 : 0);
    } else if (what == "candidates") {
      double pose[3];
      for (double & v : pose) {v = real(in);}
      const double s = real(in), a = real(in);
      for (int32_t c = 0; c < kRefineCandidates; ++c) {
        double out[3];
        refine_candidate(pose, s, a, c, out);
        std::printf("%s%a %a %a", c ? " " : "", out[0], out[1], out[2]);
      }
      std::printf("\n");
    } else if (what == "pick") {
      uint64_t cost[kRefineCandidates];
      for (uint64_t & v : cost) {unsigned long long t = 0; in >> t; v = t;}
      std::printf("%d\n", refine_pick(cost));
    } else if (what == "machine") {
      double pose[3], target[3];
      for (double & v : pose) {v = real(in);}
      kh_field_refine_params p;
      std::memset(&p, 0, sizeof(p));
      p.step_xy = real(in); p.step_heading = real(in);
      p.n_halvings = (int32_t)whole(in); p.max_rounds = (int32_t)whole(in);
      for (double & v : target) {v = real(in);}
      const double scale = real(in);
      RefineStart start;
      start.begin(pose, p, scripted(pose, target), 5);
      double cands[3 * kRefineCandidates];
      while (start.running() && start.candidates(0.0, 0.0, scale, cands)) {
        uint64_t costs[kRefineCandidates];
        for (int32_t c = 0; c < kRefineCandidates; ++c) {costs[c] = scripted(cands + 3 * c, target);}
        start.advance(costs, p);
      }
      const kh_field_refined r = start.result();
      std::printf("%a %a %a %llu %llu %d %d %d %d\n", r.pose[0], r.pose[1], r.pose[2], (unsigned long long)r.cost_start, (unsigned long long)r.cost, r.n_hit,
        r.rounds, r.halvings, r.status);
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
