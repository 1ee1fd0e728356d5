// The host rules of the map localizer (slam_toolbox_amd/csrc/map_localize_plan.hpp) without a device: reads one case per line on
// stdin, prints one result per line.  tests/test_map_localize_plan.py makes the cases and holds the expectations.
//
//   pitch seed_spacing scale                           -> pitch in cells, 0 = refused
//   blocks ox oy width height pitch                    -> bx0 by0 nx ny
//   compact ox oy width height pitch ax ay scale region cx cy radius  n (local) * n
//                                                      -> i j x y per seed, separated by blanks ("none": no seed); n = nx * ny
//   answer min_fit_score merge_distance merge_heading  n (index fine coarse x y heading known score) * n
//                                                      -> rank order | kept | rejected duplicates   (hypothesis indices)
//   predict (last odometric) (last corrected) (odometric)   -> x y heading of the predicted pose
//   fitok range_threshold min_range max_range scale ax ay x y heading   -> laser_ok pose_ok
//   inputs range_threshold min_range max_range min_angle angular_resolution scale ax ay  n (x y heading) * n
//                                                      -> failed pose | the refusal in the words of a call that takes a view
//   mergefit range_threshold min_range max_range scale off_x off_y  n_candidates n_scans (sensor x y) * n_candidates * n_scans
//                                                      -> failed candidate | the refusal in the words of kh_merge_fit
//
// Doubles are read with strtod and printed with %a, so they pass bit for bit.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../slam_toolbox_amd/csrc/map_localize_plan.hpp"

using namespace kh;

namespace
{
double real(std::istringstream & in) {std::string t; in >> t; return std::strtod(t.c_str(), nullptr);}
int64_t whole(std::istringstream & in) {long long v = 0; in >> v; return v;}
mapper::Pose pose(std::istringstream & in) {mapper::Pose p; p.x = real(in); p.y = real(in); p.h = real(in); return p;}
}  // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "pitch") {
      const double spacing = real(in), scale = real(in);
      std::printf("%d\n", seed_pitch(spacing, scale));
    } else if (what == "blocks") {
      const int32_t ox = (int32_t)whole(in), oy = (int32_t)whole(in), w = (int32_t)whole(in), h = (int32_t)whole(in), p = (int32_t)whole(in);
      const SeedBlocks b = seed_blocks(ox, oy, w, h, p);
      std::printf("%lld %lld %lld %lld\n", (long long)b.bx0, (long long)b.by0, (long long)b.nx, (long long)b.ny);
    } else if (what == "compact") {
      const int32_t ox = (int32_t)whole(in), oy = (int32_t)whole(in), w = (int32_t)whole(in), h = (int32_t)whole(in), p = (int32_t)whole(in);
      const double ax = real(in), ay = real(in), scale = real(in);
      const bool region = whole(in) != 0;
      double center[2];
      center[0] = real(in); center[1] = real(in);
      const double radius = real(in);
      std::vector<int32_t> local(static_cast<size_t>(whole(in)));
      for (int32_t & v : local) {v = (int32_t)whole(in);}
      const SeedBlocks b = seed_blocks(ox, oy, w, h, p);
      if (static_cast<int64_t>(local.size()) != b.count()) {std::printf("error: %lld blocks\n", (long long)b.count()); continue;}
      const std::vector<Seed> seeds = compact_seeds(b, p, local.data(), ax, ay, scale, region ? center : nullptr, radius);
      if (seeds.empty()) {std::printf("none");}
      for (size_t k = 0; k < seeds.size(); ++k) {std::printf("%s%d %d %a %a", k ? " " : "", seeds[k].i, seeds[k].j, seeds[k].x, seeds[k].y);}
      std::printf("\n");
    } else if (what == "answer") {
      const double min_fit = real(in), merge_d = real(in), merge_h = real(in);
      std::vector<Ranked> h(static_cast<size_t>(whole(in)));
      for (Ranked & r : h) {
        r.index = (int32_t)whole(in); r.fine_response = real(in); r.coarse_response = real(in);
        r.fine_mean[0] = real(in); r.fine_mean[1] = real(in); r.fine_mean[2] = real(in);
        r.known = (uint64_t)whole(in); r.score = real(in);
      }
      rank_hypotheses(h);
      int32_t rejected = 0, duplicates = 0;
      const std::vector<int32_t> kept = suppress_hypotheses(h, min_fit, merge_d, merge_h, &rejected, &duplicates);
      for (size_t k = 0; k < h.size(); ++k) {std::printf("%s%d", k ? " " : "", h[k].index);}
      std::printf(" |");
      for (int32_t k : kept) {std::printf(" %d", h[k].index);}
      std::printf(" | %d %d\n", rejected, duplicates);
    } else if (what == "predict") {
      const mapper::Pose a = pose(in), b = pose(in), c = pose(in);
      const mapper::Pose r = predict_pose(a, b, c);
      std::printf("%a %a %a\n", r.x, r.y, r.h);
    } else if (what == "fitok") {
      const double rt = real(in), lo = real(in), hi = real(in), scale = real(in), ax = real(in), ay = real(in);
      double p[3];
      p[0] = real(in); p[1] = real(in); p[2] = real(in);
      std::printf("%d %d\n", fit_laser_ok(rt, lo, hi, scale) ? 1 : 0, fit_pose_ok(p, ax, ay, scale) ? 1 : 0);
    } else if (what == "inputs") {
      const double rt = real(in), lo = real(in), hi = real(in), a0 = real(in), da = real(in), scale = real(in), ax = real(in), ay = real(in);
      std::vector<double> p(3 * static_cast<size_t>(whole(in)));
      for (double & v : p) {v = real(in);}
      const FitInputs f = fit_inputs_check(rt, lo, hi, a0, da, p.size() / 3, p.data(), ax, ay, scale);
      std::printf("%d %d | %s\n", f.failed, f.pose, f.failed ? fit_inputs_text(f, "who", kViewLaserWords, kViewPoseWords).c_str() : "");
    } else if (what == "mergefit") {
      const double rt = real(in), lo = real(in), hi = real(in), scale = real(in), ox = real(in), oy = real(in);
      const size_t n_candidates = static_cast<size_t>(whole(in)), n_scans = static_cast<size_t>(whole(in));
      std::vector<double> xy(2 * n_candidates * n_scans);
      for (double & v : xy) {v = real(in);}
      const FitInputs f = merge_fit_check(rt, lo, hi, n_candidates, n_scans, xy.data(), ox, oy, scale);
      std::printf("%d %d | %s\n", f.failed, f.pose, f.failed ? fit_inputs_text(f, "kh_merge_fit", kMergeLaserWords, kMergePoseWords).c_str() : "");
    } else {
      std::printf("error: unknown case %s\n", what.c_str());
    }
  }
  return 0;
}
