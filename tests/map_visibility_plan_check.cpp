// The host rules of the visibility analysis (slam_toolbox_amd/csrc/map_visibility_plan.hpp) without a device: reads one case per line
// on stdin, prints one result per line.  tests/test_map_visibility_plan.py makes the cases and holds the expectations.
//
//   create nulls width height width_step ox oy anchor_x anchor_y scale n_beams min_angle ang_res min_range max_range range_threshold
//          max_unknown w_unknown w_free w_occupied            -> "0 reach", or the refusal 1 .. 6   (nulls: bit 0 view, 1 laser, 2 params, 3 out)
//   call nulls n k min_gain select n_beams scale bad_pose value -> "0", or the refusal 1 .. 6 (and the pose's index for 3); pose bad_pose's x is `value`
//   reach range_threshold scale                               -> reach
//   bitmap reach                                              -> side words bytes lds_bytes
//   mask width height                                         -> words
//   same field                                                -> 0 / 1: a view against itself with `field` changed (none: unchanged)
//
// Doubles are read with strtod, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../slam_toolbox_amd/csrc/map_visibility_plan.hpp"

using namespace kh;

namespace
{
double real(std::istringstream & in) {std::string t; in >> t; return std::strtod(t.c_str(), nullptr);}
long long whole(std::istringstream & in) {long long v = 0; in >> v; return v;}
}  // namespace

int main()
{
  std::string line;
  static const uint8_t some_cells[4] = {0, 0, 0, 0};           // never read: a view's cells only need an address here
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "create") {
      const int nulls = (int)whole(in);
      kh_map_view v;
      std::memset(&v, 0, sizeof(v));
      v.device_cells = some_cells;
      v.width = (int32_t)whole(in); v.height = (int32_t)whole(in); v.width_step = (int32_t)whole(in); v.ox = (int32_t)whole(in); v.oy = (int32_t)whole(in);
      v.anchor[0] = real(in); v.anchor[1] = real(in); v.scale = real(in);
      kh_laser l;
      std::memset(&l, 0, sizeof(l));
      l.n_beams = (int32_t)whole(in); l.minimum_angle = real(in); l.angular_resolution = real(in); l.minimum_range = real(in); l.maximum_range = real(in);
      l.range_threshold = real(in);
      kh_visibility_params p;
      p.max_unknown = (int32_t)whole(in); p.w_unknown = (int32_t)whole(in); p.w_free = (int32_t)whole(in); p.w_occupied = (int32_t)whole(in);
      int32_t reach = -7;
      void * out = &reach;
      const int32_t bad = vis_create_check((nulls & 1) ? nullptr : &v, (nulls & 2) ? nullptr : &l, (nulls & 4) ? nullptr : &p, (nulls & 8) ? nullptr : out, &reach);
      if (bad) {std::printf("%d\n", bad);} else {std::printf("0 %d\n", reach);}
    } else if (what == "call") {
      const int nulls = (int)whole(in);
      const int32_t n = (int32_t)whole(in), k = (int32_t)whole(in);
      const uint32_t min_gain = (uint32_t)whole(in);
      const bool select = whole(in) != 0;
      const int32_t n_beams = (int32_t)whole(in);
      const double scale = real(in);
      const long long bad_at = whole(in);
      const double value = real(in);
      std::vector<double> poses(3 * (size_t)(n > 0 ? n : 1), 0.5);
      if (bad_at >= 0 && bad_at < n) {poses[3 * (size_t)bad_at] = value;}
      int32_t bad_pose = -1;
      const int32_t bad = vis_call_check((nulls & 1) != 0, n, (nulls & 2) ? nullptr : poses.data(), 0.0, 0.0, scale, n_beams, select, k, min_gain, &bad_pose);
      if (bad == kVisCallPose) {std::printf("%d %d\n", bad, bad_pose);} else {std::printf("%d\n", bad);}
    } else if (what == "reach") {
      const double range_threshold = real(in), scale = real(in);
      std::printf("%d\n", vis_reach(range_threshold, scale));
    } else if (what == "bitmap") {
      const int32_t reach = (int32_t)whole(in);
      std::printf("%d %d %d %d\n", vis_side(reach), vis_bitmap_words(reach), vis_bitmap_bytes(reach), vis_lds_bytes(reach));
    } else if (what == "mask") {
      const int32_t width = (int32_t)whole(in), height = (int32_t)whole(in);
      std::printf("%lld\n", (long long)vis_mask_words(width, height));
    } else if (what == "same") {
      std::string field;
      in >> field;
      kh_map_view a;
      std::memset(&a, 0, sizeof(a));
      a.device_cells = some_cells; a.width = 60; a.height = 50; a.width_step = 64; a.ox = -3; a.oy = 4; a.anchor[0] = 0.5; a.anchor[1] = -0.25; a.scale = 4.0;
      kh_map_view b = a;
      if (field == "cells") {b.device_cells = some_cells + 1;} else if (field == "step") {b.width_step = 72;} else if (field == "width") {b.width = 59;}
      else if (field == "height") {b.height = 51;} else if (field == "ox") {b.ox = -2;} else if (field == "oy") {b.oy = 5;}
      else if (field == "anchor_x") {b.anchor[0] = 0.75;} else if (field == "anchor_y") {b.anchor[1] = 0.0;} else if (field == "scale") {b.scale = 8.0;}
      else if (field == "device") {b.device = 1;}
      std::printf("%d\n", vis_same_window(a, b) ? 1 : 0);
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
