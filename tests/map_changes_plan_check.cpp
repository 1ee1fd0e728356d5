// The host rules of the map change layer (slam_toolbox_amd/csrc/map_changes_plan.hpp) without a device: reads one case per line on
// stdin, prints one result per line.  tests/test_map_changes_plan.py makes the cases and holds the expectations.
//
//   bound bound n_scans n_beams                         -> taken (0 / 1) and the bound afterwards (unchanged when refused)
//   decay bound shift                                   -> shift_ok and the shifted bound (unchanged when refused)
//   args nulls n_beams range_threshold min_range max_range min_angle ang_res n_scans tolerance (x y heading) * max(n_scans, 0)
//                                                       -> 0 / 1; nulls: bit 0 laser, bit 1 ranges, bit 2 poses are NULL
//   walk range_threshold min_range max_range scale ax ay n_scans (x y heading) * n_scans
//                                                       -> 0 fine, 1 the laser, 2 a pose
//   diffargs threshold cap has_cells has_out            -> 0 / 1
//
// Doubles are read with strtod, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../slam_toolbox_amd/csrc/map_changes_plan.hpp"

using namespace kh;

namespace
{
double real(std::istringstream & in) {std::string t; in >> t; return std::strtod(t.c_str(), nullptr);}
long long whole(std::istringstream & in) {long long v = 0; in >> v; return v;}
std::vector<double> poses(std::istringstream & in, long long n)
{
  std::vector<double> p(static_cast<size_t>(n > 0 ? 3 * n : 0));
  for (double & v : p) {v = real(in);}
  if (p.empty()) {p.push_back(0.0);}                  // (a pointer that is not NULL)
  return p;
}
}  // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "bound") {
      unsigned long long bound = 0;
      in >> bound;
      const int32_t n_scans = (int32_t)whole(in), n_beams = (int32_t)whole(in);
      uint64_t after = bound;
      const bool taken = changes_bound_after(bound, n_scans, n_beams, &after);
      std::printf("%d %llu\n", taken ? 1 : 0, (unsigned long long)after);
    } else if (what == "decay") {
      unsigned long long bound = 0;
      in >> bound;
      const int32_t shift = (int32_t)whole(in);
      const bool ok = changes_shift_ok(shift);
      std::printf("%d %llu\n", ok ? 1 : 0, (unsigned long long)(ok ? changes_bound_decayed(bound, shift) : bound));
    } else if (what == "args") {
      const long long nulls = whole(in);
      kh_laser laser;
      laser.n_beams = (int32_t)whole(in);
      laser.range_threshold = real(in); laser.minimum_range = real(in); laser.maximum_range = real(in);
      laser.minimum_angle = real(in); laser.angular_resolution = real(in);
      laser.offset_x = 0.0; laser.offset_y = 0.0; laser.offset_heading = 0.0;
      const int32_t n_scans = (int32_t)whole(in), tolerance = (int32_t)whole(in);
      const std::vector<double> p = poses(in, n_scans);
      const double ranges[1] = {1.0};
      std::printf("%d\n", changes_observe_args_ok((nulls & 1) ? nullptr : &laser, n_scans, (nulls & 2) ? nullptr : ranges,
        (nulls & 4) ? nullptr : p.data(), tolerance) ? 1 : 0);
    } else if (what == "walk") {
      kh_laser laser;
      laser.n_beams = 1;
      laser.range_threshold = real(in); laser.minimum_range = real(in); laser.maximum_range = real(in);
      laser.minimum_angle = 0.0; laser.angular_resolution = 0.0; laser.offset_x = 0.0; laser.offset_y = 0.0; laser.offset_heading = 0.0;
      const double scale = real(in), ax = real(in), ay = real(in);
      const int32_t n_scans = (int32_t)whole(in);
      const std::vector<double> p = poses(in, n_scans);
      std::printf("%d\n", changes_observe_walk(laser, n_scans, p.data(), ax, ay, scale).failed);
    } else if (what == "diffargs") {
      const double threshold = real(in);
      const int32_t cap = (int32_t)whole(in);
      const bool has_cells = whole(in) != 0, has_out = whole(in) != 0;
      int32_t cells[3];
      std::printf("%d\n", changes_diff_args_ok(threshold, has_cells ? cells : nullptr, cap, has_out ? &line : nullptr) ? 1 : 0);
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
