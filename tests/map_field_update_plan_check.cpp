// The host rules of kh_map_field_update (slam_toolbox_amd/csrc/map_field_update_plan.hpp) without a device: reads one case per line
// on stdin, prints one result per line.  tests/test_map_field_update_plan.py makes the cases and holds the expectations.
//
//   clip ox oy width height [x y w h]            -> "x0 y0 x1 y1" in window columns / rows, "none" for an empty clip (no rect: NULL)
//   regions width height R x0 y0 x1 y1           -> values, columns, reads, staged: four rectangles "x0 y0 x1 y1" / "none"
//   box x0 y0 x1 y1                              -> k_field_changed's inclusive box as a rectangle
//   bands R rows forced                          -> band height and band count
//   lattice ax ay scale device bx by scale2 device2 -> 0 same, 1 anchor x, 2 anchor y, 3 scale, 4 device
//   window width height R                        -> field_check's code for a new window
//   kind same_window has_columns R failed_before -> 0 region, 1 relayout, 2 no columns, 3 uncapped, 4 after a failure
//
// Doubles are read with strtod, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../slam_toolbox_amd/csrc/map_field_update_plan.hpp"

using namespace kh;

namespace
{
double real(std::istringstream & in) {std::string t; in >> t; return std::strtod(t.c_str(), nullptr);}
long long whole(std::istringstream & in) {long long v = 0; in >> v; return v;}
std::string text(const Rect & r)
{
  if (r.empty()) {return "none";}
  return std::to_string(r.x0) + " " + std::to_string(r.y0) + " " + std::to_string(r.x1) + " " + std::to_string(r.y1);
}
}  // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "clip") {
      const int32_t ox = (int32_t)whole(in), oy = (int32_t)whole(in), width = (int32_t)whole(in), height = (int32_t)whole(in);
      int32_t rect[4];
      int32_t n = 0;
      for (long long v; n < 4 && (in >> v); ++n) {rect[n] = (int32_t)v;}
      std::printf("%s\n", text(update_clip(n == 4 ? rect : nullptr, ox, oy, width, height)).c_str());
    } else if (what == "regions") {
      const int32_t width = (int32_t)whole(in), height = (int32_t)whole(in), radius = (int32_t)whole(in);
      Rect c;
      c.x0 = whole(in); c.y0 = whole(in); c.x1 = whole(in); c.y1 = whole(in);
      const UpdateRegions u = update_regions(c, radius, width, height);
      std::printf("%s, %s, %s, %s\n", text(u.values).c_str(), text(u.columns).c_str(), text(u.reads).c_str(), text(u.staged).c_str());
    } else if (what == "box") {
      int32_t w[4];
      for (int32_t & v : w) {v = (int32_t)whole(in);}
      std::printf("%s\n", text(changed_box(w)).c_str());
    } else if (what == "bands") {
      const int32_t radius = (int32_t)whole(in);
      const int64_t rows = whole(in);
      const int32_t forced = (int32_t)whole(in);
      const int32_t band = band_rows(radius, rows, forced);
      std::printf("%d %lld\n", band, (long long)band_count(rows, band));
    } else if (what == "lattice") {
      double a[2], b[2];
      a[0] = real(in); a[1] = real(in);
      const double scale = real(in);
      const int32_t device = (int32_t)whole(in);
      b[0] = real(in); b[1] = real(in);
      const double scale2 = real(in);
      const int32_t device2 = (int32_t)whole(in);
      std::printf("%d\n", lattice_check(a, scale, device, b, scale2, device2));
    } else if (what == "window") {
      const int32_t width = (int32_t)whole(in), height = (int32_t)whole(in), radius = (int32_t)whole(in);
      std::printf("%d\n", update_window_check(width, height, radius));
    } else if (what == "kind") {
      const bool same = whole(in) != 0, has = whole(in) != 0;
      const int32_t radius = (int32_t)whole(in);
      const bool failed = whole(in) != 0;
      std::printf("%d\n", update_kind(same, has, radius, failed));
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
