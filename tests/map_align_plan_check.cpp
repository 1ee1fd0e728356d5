// The host rules of the ray cast and of the map alignment (slam_toolbox_amd/csrc/map_align_plan.hpp, RayWalk of occupancy_device.hpp)
// without a device: reads one case per line on stdin, prints one result per line.  tests/test_map_align_plan.py makes the cases and
// holds the expectations.
//
//   walk x0 y0 x1 y1                      -> the cells RayWalk visits outward from (x0, y0): "x,y x,y ..."
//   noreturn range_threshold max_range    -> the default reading of a beam without a hit
//   probes n_probes hits...               -> the picked seed indices
//   correction px py ph qx qy qh          -> P . inverse(Q)
//   pose cx cy ch sx sy sh                -> C . S
//   rank min_known n (6 counters) * n     -> per ranked candidate "index:enough:score"
//   args probe_spacing n_probes top_k max_unknown ix iy ih seed_spacing n_headings   -> 0 / 1
//
// Doubles are read with strtod and printed with %a, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../slam_toolbox_amd/csrc/map_align_plan.hpp"

using namespace kh;

namespace
{
double real(std::istringstream & in) {std::string t; in >> t; return std::strtod(t.c_str(), nullptr);}
long long whole(std::istringstream & in) {long long v = 0; in >> v; return v;}
}  // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "walk") {
      const int32_t x0 = (int32_t)whole(in), y0 = (int32_t)whole(in), x1 = (int32_t)whole(in), y1 = (int32_t)whole(in);
      RayWalk walk(x0, y0, x1, y1);
      const int32_t length = walk.length();
      for (int32_t s = 0; s <= length; ++s, walk.next()) {std::printf("%s%d,%d", s ? " " : "", walk.x(), walk.y());}
      std::printf("\n");
    } else if (what == "noreturn") {
      const double threshold = real(in), max_range = real(in);
      std::printf("%a\n", ray_no_return(threshold, max_range));
    } else if (what == "probes") {
      const int32_t n_probes = (int32_t)whole(in);
      std::vector<int32_t> hits;
      long long v;
      while (in >> v) {hits.push_back((int32_t)v);}
      for (int32_t k : align_pick_probes(hits, n_probes)) {std::printf("%d ", k);}
      std::printf("\n");
    } else if (what == "correction") {
      double p[3], q[3], c[3];
      for (double & v : p) {v = real(in);}
      for (double & v : q) {v = real(in);}
      align_correction(p, q, c);
      std::printf("%a %a %a\n", c[0], c[1], c[2]);
    } else if (what == "pose") {
      double c[3], s[3], out[3];
      for (double & v : c) {v = real(in);}
      for (double & v : s) {v = real(in);}
      AlignRigid(c[0], c[1], c[2]).pose(s, out);
      std::printf("%a %a %a\n", out[0], out[1], out[2]);
    } else if (what == "rank") {
      unsigned long long min_known = 0;
      in >> min_known;
      const size_t n = (size_t)whole(in);
      std::vector<uint64_t> sums(n * kFitCounters);
      for (uint64_t & v : sums) {unsigned long long t = 0; in >> t; v = t;}
      const double zero[3] = {0.0, 0.0, 0.0};
      std::vector<kh_map_align_cand> cands(n, align_candidate(zero, -1, -1, 0.0));
      align_rank(cands, sums, min_known);
      for (const kh_map_align_cand & c : cands) {std::printf("%d:%d:%a ", c.index, c.enough, c.fit.score);}
      std::printf("\n");
    } else if (what == "args") {
      kh_map_align_params p;
      std::memset(&p, 0, sizeof(p));                     // (zeros are valid relocalization parameters but for the spacing)
      p.probe_spacing = real(in);
      p.n_probes = (int32_t)whole(in); p.top_k = (int32_t)whole(in); p.max_unknown = (int32_t)whole(in); p.pad = 0; p.min_known = 0;
      for (double & v : p.initial) {v = real(in);}
      p.relocalize.seed_spacing = real(in); p.relocalize.n_headings = (int32_t)whole(in);
      std::printf("%d\n", align_params_ok(p) ? 1 : 0);
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
