// The host rules of the region analysis (slam_toolbox_amd/csrc/map_regions_plan.hpp) without a device: reads one case per line on
// stdin, prints one result per line.  tests/test_map_regions_plan.py makes the cases and holds the expectations.
//
//   check min_clearance scale connectivity min_r max_r min_f max_f -> "0 Rc", or the refusal 1 .. 5
//   reach R Rc                                                    -> 0 / 1
//   grid width height                                             -> tiles_x tiles_y seam_threads units
//   cell sum n                                                    -> the centroid cell's coordinate
//   record anchor o sum n a scale                                 -> the centroid's and the anchor's coordinate, two doubles
//
// Doubles are read with strtod and printed with %a, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../slam_toolbox_amd/csrc/map_regions_plan.hpp"

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
    if (what == "check") {
      kh_map_regions_params p;
      std::memset(&p, 0, sizeof(p));
      p.min_clearance = real(in);
      const double scale = real(in);
      p.connectivity = (int32_t)whole(in); p.min_region_cells = (int32_t)whole(in); p.max_regions = (int32_t)whole(in);
      p.min_frontier_cells = (int32_t)whole(in); p.max_frontiers = (int32_t)whole(in);
      int32_t rc = -7;
      const int32_t bad = regions_check(p, scale, &rc);
      if (bad) {std::printf("%d\n", bad);} else {std::printf("0 %d\n", rc);}
    } else if (what == "reach") {
      const int32_t r = (int32_t)whole(in), rc = (int32_t)whole(in);
      std::printf("%d\n", regions_reach_ok(r, rc) ? 1 : 0);
    } else if (what == "grid") {
      const int32_t width = (int32_t)whole(in), height = (int32_t)whole(in);
      const RegionGrid g = region_grid(width, height);
      std::printf("%d %d %lld %lld\n", g.tiles_x, g.tiles_y, (long long)g.seam_threads, (long long)g.units);
    } else if (what == "cell") {
      unsigned long long sum = 0, n = 0;
      in >> sum >> n;
      std::printf("%llu\n", (unsigned long long)centroid_cell(sum, n));
    } else if (what == "record") {
      const double anchor = real(in);
      const int32_t o = (int32_t)whole(in);
      unsigned long long sum = 0;
      in >> sum;
      const uint32_t n = (uint32_t)whole(in);
      const int32_t a = (int32_t)whole(in);
      const double scale = real(in);
      std::printf("%a %a\n", region_centroid(anchor, o, sum, n, scale), region_cell_world(anchor, o, a, scale));
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
