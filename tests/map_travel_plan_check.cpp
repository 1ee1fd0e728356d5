// The host rules of the travel costs (slam_toolbox_amd/csrc/map_travel_plan.hpp) without a device: reads one case per line on stdin,
// prints one result per line.  tests/test_map_travel_plan.py makes the cases and holds the expectations.
//
//   check min_clearance scale inscribed inflation factor track inflate connectivity cut neutral weight snap -> "0 Rc Rt", or the refusal 1 .. 8
//   field connectivity neutral weight Rc Rt R width height  -> 0, or the refusal 1 .. 3
//   qmax neutral weight                                     -> q_max
//   overflow width height connectivity q_max                -> 0 / 1
//   grid width height                                       -> tiles_x tiles_y tiles
//   flag tx ty tiles_x tiles_y conn8 lowered                -> the mask of the flagged neighbours
//   step n                                                  -> di dj L
//   paths n max_cells                                       -> 0 / 1
//   snap snap_cells                                         -> 0 / 1
//
// Doubles are read with strtod, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../slam_toolbox_amd/csrc/map_travel_plan.hpp"

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
      kh_map_travel_params p;
      std::memset(&p, 0, sizeof(p));
      p.min_clearance = real(in);
      const double scale = real(in);
      p.inflation.inscribed_radius = real(in); p.inflation.inflation_radius = real(in); p.inflation.cost_scaling_factor = real(in);
      p.inflation.track_unknown = (int32_t)whole(in); p.inflation.inflate_unknown = (int32_t)whole(in);
      p.connectivity = (int32_t)whole(in); p.cut_corners = (int32_t)whole(in); p.neutral_cost = (int32_t)whole(in); p.cost_weight = (int32_t)whole(in);
      p.goal_snap_cells = (int32_t)whole(in);
      int32_t rc = -7, rt = -7;
      const int32_t bad = travel_check(p, scale, &rc, &rt);
      if (bad) {std::printf("%d\n", bad);} else {std::printf("0 %d %d\n", rc, rt);}
    } else if (what == "field") {
      kh_map_travel_params p;
      std::memset(&p, 0, sizeof(p));
      p.connectivity = (int32_t)whole(in); p.neutral_cost = (int32_t)whole(in); p.cost_weight = (int32_t)whole(in);
      const int32_t rc = (int32_t)whole(in), rt = (int32_t)whole(in), r = (int32_t)whole(in);
      const long long width = whole(in), height = whole(in);
      std::printf("%d\n", travel_field_check(p, rc, rt, r, width, height));
    } else if (what == "qmax") {
      const int32_t neutral = (int32_t)whole(in), weight = (int32_t)whole(in);
      std::printf("%u\n", travel_q_max(neutral, weight));
    } else if (what == "overflow") {
      const long long width = whole(in), height = whole(in);
      const int32_t connectivity = (int32_t)whole(in);
      const uint32_t qmax = (uint32_t)whole(in);
      std::printf("%d\n", travel_overflows(width, height, connectivity, qmax) ? 1 : 0);
    } else if (what == "grid") {
      const int32_t width = (int32_t)whole(in), height = (int32_t)whole(in);
      const TravelGrid g = travel_grid(width, height);
      std::printf("%d %d %lld\n", g.tiles_x, g.tiles_y, (long long)g.tiles);
    } else if (what == "flag") {
      const int32_t tx = (int32_t)whole(in), ty = (int32_t)whole(in), tiles_x = (int32_t)whole(in), tiles_y = (int32_t)whole(in), conn8 = (int32_t)whole(in);
      const uint32_t lowered = (uint32_t)whole(in);
      std::printf("%u\n", travel_flagged(tx, ty, tiles_x, tiles_y, conn8 != 0, lowered));
    } else if (what == "step") {
      const int32_t n = (int32_t)whole(in);
      std::printf("%d %d %u\n", travel_di(n), travel_dj(n), travel_length(n));
    } else if (what == "paths") {
      const int32_t n = (int32_t)whole(in), max_cells = (int32_t)whole(in);
      std::printf("%d\n", travel_path_buffer_ok(n, max_cells) ? 1 : 0);
    } else if (what == "snap") {
      std::printf("%d\n", travel_snap_ok((int32_t)whole(in)) ? 1 : 0);
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
