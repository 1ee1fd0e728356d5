// The host rules of the footprint analysis (slam_toolbox_amd/csrc/map_footprint_plan.hpp) without a device: reads one case per line on
// stdin, prints one result per line.  tests/test_map_footprint_plan.py makes the cases and holds the expectations.
//
//   create nulls scale n vx vy ..          -> "0 reach", or the refusal 1 .. 5   (nulls: bit 0 field, 1 vertices, 2 out)
//   convex n vx vy ..                      -> 0 / 1
//   reach scale n vx vy ..                 -> ceil(r_max * scale) + 1, as %.17g
//   check nulls n bad_at value             -> "0", or the refusal 1 .. 3 (and the pose's index for 3); word bad_at of the poses is `value`
//   layer n_headings max_status reach      -> "0", or the refusal 1 .. 3
//   cells scale ax ay x y theta n vx vy .. -> "L", or "own_x own_y x0 y0 x1 y1 .."
//   offsets scale h H n vx vy ..           -> "x0 y0 x1 y1 .."
//   spans n x y ..                         -> "y0 lo hi lo hi ..", or "none"
//   table scale reach H n vx vy ..         -> "rows words..", or "none"
//   triangles                              -> for every triangle (a, b, c) of cells of the 7 x 7 box, a-major: its covered cells as a
//                                             49-bit mask (bit 7 y + x), in hex
//
// Doubles are read with strtod, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../slam_toolbox_amd/csrc/map_footprint_plan.hpp"

using namespace kh;

namespace
{
double real(std::istringstream & in) {std::string t; in >> t; return std::strtod(t.c_str(), nullptr);}
long long whole(std::istringstream & in) {long long v = 0; in >> v; return v;}
std::vector<double> vertices(std::istringstream & in, int32_t * n)
{
  *n = (int32_t)whole(in);
  std::vector<double> v(2 * (size_t)(*n > 0 ? *n : 0) + 2, 0.0);
  for (int32_t k = 0; k < 2 * *n; ++k) {v[(size_t)k] = real(in);}
  return v;
}
}  // namespace

int main()
{
  std::string line;
  static const int some_field = 0;                            // never read: a field only needs an address here
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "create") {
      const int nulls = (int)whole(in);
      const double scale = real(in);
      int32_t n = 0;
      const std::vector<double> v = vertices(in, &n);
      int32_t reach = -7;
      const int32_t bad = foot_create_check((nulls & 1) ? nullptr : &some_field, n, (nulls & 2) ? nullptr : v.data(), (nulls & 4) ? nullptr : &reach, scale, &reach);
      if (bad) {std::printf("%d\n", bad);} else {std::printf("0 %d\n", reach);}
    } else if (what == "convex") {
      int32_t n = 0;
      const std::vector<double> v = vertices(in, &n);
      std::printf("%d\n", foot_convex(n, v.data()) ? 1 : 0);
    } else if (what == "reach") {
      const double scale = real(in);
      int32_t n = 0;
      const std::vector<double> v = vertices(in, &n);
      std::printf("%.17g\n", foot_reach(n, v.data(), scale));
    } else if (what == "check") {
      const int nulls = (int)whole(in);
      const int32_t n = (int32_t)whole(in);
      const long long bad_at = whole(in);
      const double value = real(in);
      std::vector<double> poses(3 * (size_t)(n > 0 && n <= kFootMaxPoses ? n : 1), 0.5);
      if (bad_at >= 0 && (size_t)bad_at < poses.size()) {poses[(size_t)bad_at] = value;}
      int32_t bad_pose = -1;
      const int32_t bad = foot_check_check(n, (nulls & 1) ? nullptr : poses.data(), (nulls & 2) ? nullptr : &bad_pose, &bad_pose);
      if (bad == kFootCallPose) {std::printf("%d %d\n", bad, bad_pose);} else {std::printf("%d\n", bad);}
    } else if (what == "layer") {
      const int32_t h = (int32_t)whole(in), max_status = (int32_t)whole(in), reach = (int32_t)whole(in);
      std::printf("%d\n", foot_layer_check(h, max_status, reach));
    } else if (what == "cells") {
      const double scale = real(in), ax = real(in), ay = real(in);
      const double pose[3] = {real(in), real(in), real(in)};
      int32_t n = 0;
      const std::vector<double> v = vertices(in, &n);
      int32_t cells[2 * kFootMaxVertices], own[2];
      if (!foot_pose_cells(n, v.data(), pose, ax, ay, scale, cells, own)) {
        std::printf("L\n");
      } else {
        std::printf("%d %d", own[0], own[1]);
        for (int32_t k = 0; k < 2 * n; ++k) {std::printf(" %d", cells[k]);}
        std::printf("\n");
      }
    } else if (what == "offsets") {
      const double scale = real(in);
      const int32_t h = (int32_t)whole(in), n_headings = (int32_t)whole(in);
      int32_t n = 0;
      const std::vector<double> v = vertices(in, &n);
      int32_t cells[2 * kFootMaxVertices];
      foot_heading_offsets(n, v.data(), h, n_headings, scale, cells);
      for (int32_t k = 0; k < 2 * n; ++k) {std::printf(k ? " %d" : "%d", cells[k]);}
      std::printf("\n");
    } else if (what == "spans") {
      const int32_t n = (int32_t)whole(in);
      std::vector<int32_t> v(2 * (size_t)n);
      for (int32_t & c : v) {c = (int32_t)whole(in);}
      FootSpans s;
      if (!foot_spans(v.data(), n, &s)) {
        std::printf("none\n");
      } else {
        std::printf("%d", s.y0);
        for (size_t r = 0; r < s.lo.size(); ++r) {std::printf(" %d %d", s.lo[r], s.hi[r]);}
        std::printf("\n");
      }
    } else if (what == "table") {
      const double scale = real(in);
      const int32_t reach = (int32_t)whole(in), n_headings = (int32_t)whole(in);
      int32_t n = 0;
      const std::vector<double> v = vertices(in, &n);
      std::vector<int32_t> table;
      int32_t rows = 0;
      if (!foot_layer_table(n, v.data(), n_headings, scale, reach, &table, &rows)) {
        std::printf("none\n");
      } else {
        std::printf("%d", rows);
        for (const int32_t w : table) {std::printf(" %d", w);}
        std::printf("\n");
      }
    } else if (what == "triangles") {
      FootSpans s;
      for (int32_t a = 0; a < 49; ++a) {
        for (int32_t b = 0; b < 49; ++b) {
          for (int32_t c = 0; c < 49; ++c) {
            const int32_t v[6] = {a % 7, a / 7, b % 7, b / 7, c % 7, c / 7};
            unsigned long long mask = 0ull;
            if (foot_spans(v, 3, &s)) {
              for (size_t r = 0; r < s.lo.size(); ++r) {
                for (int32_t x = s.lo[r]; x <= s.hi[r]; ++x) {mask |= 1ull << (7 * (s.y0 + (int32_t)r) + x);}
              }
            }
            std::printf("%llx ", mask);
          }
        }
      }
      std::printf("\n");
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
