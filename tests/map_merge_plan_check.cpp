// The host rules of the map merge (slam_toolbox_amd/csrc/map_merge_plan.hpp) without a device: reads one case per line on stdin,
// prints one result per line.  tests/test_map_merge_plan.py makes the cases and holds the expectations.
//
//   offsets n scale_t                                   -> the n sample offsets of one axis
//   footprint scale_m scale_t                           -> the default footprint
//   inverse cx cy cyaw                                  -> inverse(C) as x y yaw cos sin
//   window tox toy tw th tax tay tscale max may mscale i0 j0 i1 j1 cx cy cyaw grow
//                                                       -> "0 ox oy width height width_step", or the refusal 1 / 2 / 3
//   agreement (6 counters)                              -> overlap and the agreement
//   args cx cy cyaw footprint conflict grow             -> 0 / 1
//
// Doubles are read with strtod and printed with %a, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../slam_toolbox_amd/csrc/map_merge_plan.hpp"

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
    if (what == "offsets") {
      const int32_t n = (int32_t)whole(in);
      const double scale = real(in);
      double d[kMaxMergeFootprint];
      merge_sample_offsets(n, scale, d);
      for (int32_t k = 0; k < n; ++k) {std::printf("%s%a", k ? " " : "", d[k]);}
      std::printf("\n");
    } else if (what == "footprint") {
      const double scale_m = real(in), scale_t = real(in);
      std::printf("%d\n", merge_default_footprint(scale_m, scale_t));
    } else if (what == "inverse") {
      const double x = real(in), y = real(in), yaw = real(in);
      const AlignRigid inv = align_inverse(AlignRigid(x, y, yaw));
      std::printf("%a %a %a %a %a\n", inv.x, inv.y, inv.yaw, inv.c, inv.s);
    } else if (what == "window") {
      kh_map_view target, moving;
      std::memset(&target, 0, sizeof(target)); std::memset(&moving, 0, sizeof(moving));
      target.ox = (int32_t)whole(in); target.oy = (int32_t)whole(in); target.width = (int32_t)whole(in); target.height = (int32_t)whole(in);
      target.anchor[0] = real(in); target.anchor[1] = real(in); target.scale = real(in);
      moving.anchor[0] = real(in); moving.anchor[1] = real(in); moving.scale = real(in);
      int32_t box[4];
      for (int32_t & v : box) {v = (int32_t)whole(in);}
      double c[3];
      for (double & v : c) {v = real(in);}
      const int32_t grow = (int32_t)whole(in);
      MergeWindow w;
      const int32_t rc = merge_window(target, moving, box, c, grow, &w);
      if (rc) {std::printf("%d\n", rc);} else {std::printf("0 %d %d %d %d %d\n", w.ox, w.oy, w.width, w.height, w.ws);}
    } else if (what == "agreement") {
      uint64_t c[kMergeCounters];
      for (uint64_t & v : c) {unsigned long long t = 0; in >> t; v = t;}
      std::printf("%llu %a\n", (unsigned long long)merge_overlap(c), merge_agreement(c));
    } else if (what == "args") {
      kh_map_merge_params p;
      std::memset(&p, 0, sizeof(p));
      for (double & v : p.correction) {v = real(in);}
      p.footprint = (int32_t)whole(in); p.conflict = (int32_t)whole(in); p.grow = (int32_t)whole(in);
      std::printf("%d\n", merge_params_ok(p) ? 1 : 0);
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
