// The host rules of the map localizer (kh_map_seeds, kh_map_fit, kh_map_localizer_*) without a device: the
// pitch of the seed lattice, the blocks that cover a window, the compaction of the per-block answers, the walk-length guard of the
// fit, the ranking and the suppression of an answer, the odometric prediction.  Needs no HIP header: tests/map_localize_plan_check.cpp
// drives it on the CPU.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "live_map_plan.hpp"     // floor_div
#include "mapper_pose.hpp"       // Pose, transform_pose, normalize_angle, kTolerance
#include "occupancy_device.hpp"  // round_half_away, the order of the six counters

namespace kh
{
constexpr int32_t kMaxSeedPitch = 4096;              // cells: the key of k_map_seeds holds a block's local index in 32 bits with room to spare
constexpr int64_t kMaxFitWalk = 1ll << 20;           // cells one beam of k_map_fit may walk
constexpr double kMaxFitCell = 1073741824.0;         // |lattice index| of a sensor cell of k_map_fit (2^30): index +- walk stays an int32

// pitch = max(1, (int)round_half_away(seed_spacing * scale)) | 1 cells; 0 = refused (spacing not finite or <= 0, pitch above kMaxSeedPitch)
inline int32_t seed_pitch(double seed_spacing, double scale)
{
  if (!std::isfinite(seed_spacing) || !(seed_spacing > 0.0) || !std::isfinite(scale) || !(scale > 0.0)) {return 0;}
  const double cells = round_half_away(seed_spacing * scale);
  if (!(cells <= static_cast<double>(kMaxSeedPitch))) {return 0;}
  const int32_t pitch = std::max(1, static_cast<int32_t>(cells)) | 1;
  return pitch > kMaxSeedPitch ? 0 : pitch;
}

// the blocks of side `pitch` that hold a cell of the window [ox, ox + width) x [oy, oy + height): block indices are floor quotients of
// the lattice index, so a block stays where it is when the window grows
struct SeedBlocks
{
  int64_t bx0 = 0, by0 = 0;      // first block column / row
  int64_t nx = 0, ny = 0;        // block columns / rows
  int64_t count() const {return nx * ny;}
};
inline SeedBlocks seed_blocks(int32_t ox, int32_t oy, int32_t width, int32_t height, int32_t pitch)
{
  SeedBlocks b;
  if (width <= 0 || height <= 0 || pitch <= 0) {return b;}
  b.bx0 = floor_div(ox, pitch); b.by0 = floor_div(oy, pitch);
  b.nx = floor_div(static_cast<int64_t>(ox) + width - 1, pitch) - b.bx0 + 1;
  b.ny = floor_div(static_cast<int64_t>(oy) + height - 1, pitch) - b.by0 + 1;
  return b;
}

// One seed: its lattice cell and its world point anchor + lattice / scale (the integer sum o + i is the lattice index itself)
struct Seed {int32_t i, j; double x, y;};

// k_map_seeds answers per block, row-major over the blocks, the local index (row * pitch + column inside the block) of its seed or
// -1.  The seeds in ascending (by, bx); with radius > 0 only those with (dx * dx) + (dy * dy) < radius * radius + KT_TOLERANCE.
inline std::vector<Seed> compact_seeds(const SeedBlocks & b, int32_t pitch, const int32_t * local, double ax, double ay, double scale,
  const double * center_xy, double radius)
{
  std::vector<Seed> seeds;
  for (int64_t by = 0; by < b.ny; ++by) {
    for (int64_t bx = 0; bx < b.nx; ++bx) {
      const int32_t loc = local[by * b.nx + bx];
      if (loc < 0) {continue;}
      Seed s;
      s.i = static_cast<int32_t>((b.bx0 + bx) * pitch + loc % pitch);
      s.j = static_cast<int32_t>((b.by0 + by) * pitch + loc / pitch);
      s.x = ax + static_cast<double>(s.i) / scale;
      s.y = ay + static_cast<double>(s.j) / scale;
      if (center_xy && radius > 0) {
        const double dx = s.x - center_xy[0], dy = s.y - center_xy[1];
        if (!((dx * dx) + (dy * dy) < radius * radius + mapper::kTolerance)) {continue;}
      }
      seeds.push_back(s);
    }
  }
  return seeds;
}

// Can every beam of a scan at sensor position (sx, sy) be walked in at most kMaxFitWalk cells, with every cell index an int32?  A kept
// beam ends within range_threshold of the sensor (AddScan clips it there), give or take a rounding on either end.
inline bool fit_laser_ok(double range_threshold, double min_range, double max_range, double scale)
{
  return std::isfinite(range_threshold) && range_threshold > 0.0 && !std::isnan(min_range) && !std::isnan(max_range) &&
         range_threshold * scale + 2.0 <= static_cast<double>(kMaxFitWalk);
}
inline bool fit_pose_ok(const double pose[3], double ax, double ay, double scale)
{
  if (!std::isfinite(pose[0]) || !std::isfinite(pose[1]) || !std::isfinite(pose[2])) {return false;}
  const double cx = (pose[0] - ax) * scale, cy = (pose[1] - ay) * scale;
  return std::fabs(cx) <= kMaxFitCell && std::fabs(cy) <= kMaxFitCell;
}

// The laser and pose check of every call that walks beams on a map view: the laser (fit_laser_ok, and angles that are numbers), then
// pose 0 .. n_poses - 1 of `poses` (3 doubles each; fit_pose_ok).  Which input failed and, for a pose, which one.
enum : int32_t {kFitInputsOk = 0, kFitInputsLaser = 1, kFitInputsPose = 2};
struct FitInputs {int32_t failed; int32_t pose;};
inline FitInputs fit_inputs_check(double range_threshold, double min_range, double max_range, double min_angle, double angular_resolution,
  size_t n_poses, const double * poses, double ax, double ay, double scale)
{
  if (!fit_laser_ok(range_threshold, min_range, max_range, scale) || !std::isfinite(min_angle) || !std::isfinite(angular_resolution)) {
    return FitInputs{kFitInputsLaser, -1};
  }
  for (size_t k = 0; k < n_poses; ++k) {
    if (!fit_pose_ok(poses + 3 * k, ax, ay, scale)) {return FitInputs{kFitInputsPose, static_cast<int32_t>(k)};}
  }
  return FitInputs{kFitInputsOk, -1};
}
// ... and the refusal as the caller's message: "`who`: `laser_words`", or "`who`: `pose_words`" with the pose's index in the place of
// its '#', if it has one.  The words of the calls that take a view (a handle speaks of its own map in words of its own):
constexpr const char * kViewLaserWords = "the laser's range_threshold * scale must stay below 2^20 cells, its other fields must be numbers";
constexpr const char * kViewPoseWords = "pose # is not finite or lies more than 2^30 cells from the anchor";
inline std::string fit_inputs_text(const FitInputs & f, const char * who, const char * laser_words, const char * pose_words)
{
  std::string words = f.failed == kFitInputsLaser ? laser_words : pose_words;
  const size_t at = f.failed == kFitInputsPose ? words.find('#') : std::string::npos;
  if (at != std::string::npos) {words.replace(at, 1, std::to_string(f.pose));}
  return std::string(who) + ": " + words;
}

// The same check for the fit of a session merge (kh_merge_fit, kh_merge_align): the moving submap's laser
// (fit_laser_ok), then the sensor position of every scan under every candidate -- sensors_xy holds n_candidates * n_scans pairs
// (x, y), candidate-major, as k_occ_fit_merged reads them -- by fit_pose_ok's arithmetic with the reference grid's offset as the
// origin.  A refused position is reported with its CANDIDATE's index in FitInputs::pose.
inline FitInputs merge_fit_check(double range_threshold, double min_range, double max_range, size_t n_candidates, size_t n_scans,
  const double * sensors_xy, double off_x, double off_y, double scale)
{
  if (!fit_laser_ok(range_threshold, min_range, max_range, scale)) {return FitInputs{kFitInputsLaser, -1};}
  for (size_t k = 0; k < n_candidates; ++k) {
    for (size_t i = 0; i < n_scans; ++i) {
      const double * xy = sensors_xy + 2 * (k * n_scans + i);
      const double at[3] = {xy[0], xy[1], 0.0};
      if (!fit_pose_ok(at, off_x, off_y, scale)) {return FitInputs{kFitInputsPose, static_cast<int32_t>(k)};}
    }
  }
  return FitInputs{kFitInputsOk, -1};
}
constexpr const char * kMergeLaserWords =
  "the moving submap's range_threshold * scale must stay below 2^20 cells, its minimum and maximum range must be numbers";
constexpr const char * kMergePoseWords = "correction # puts a scan's sensor more than 2^30 cells from the offset of the reference grid";

// the six counters -> kh_merge_fit_t
inline kh_merge_fit_t fit_derive(const uint64_t c[kFitCounters])
{
  kh_merge_fit_t f;
  f.pass_unknown = c[kFitPassUnknown]; f.pass_occupied = c[kFitPassOccupied]; f.pass_free = c[kFitPassFree];
  f.hits_unknown = c[kFitHitsUnknown]; f.hits_occupied = c[kFitHitsOccupied]; f.hits_free = c[kFitHitsFree];
  // pass - 2 hits = the visits that are not the end cell of a hit beam (that cell is visited twice: by the line, and as the hit)
  f.agree = f.hits_occupied + (f.pass_free - 2 * f.hits_free);
  f.conflict = (f.pass_occupied - 2 * f.hits_occupied) + f.hits_free;
  f.known = f.agree + f.conflict;
  f.score = f.known == 0 ? 0.0 : static_cast<double>(f.agree) / static_cast<double>(f.known);
  return f;
}

// what kh_map_localizer_relocalize (and kh_map_align, which hands them on) takes of its parameters before a device is looked for
inline bool relocalize_params_ok(const kh_map_relocalize_params & p)
{
  return p.seed_spacing > 0 && std::isfinite(p.seed_spacing) && p.n_headings >= 0 && p.n_headings <= 4096 && p.top_k >= 0 &&
         std::isfinite(p.radius) && std::isfinite(p.center_xy[0]) && std::isfinite(p.center_xy[1]) && !std::isnan(p.minimum_response_coarse) &&
         !std::isnan(p.maximum_variance_coarse) && !std::isnan(p.minimum_response_fine) && !std::isnan(p.min_fit_score) &&
         !std::isnan(p.merge_distance) && !std::isnan(p.merge_heading);
}

// ---- the answer of a relocalization ----
// what the ranking reads of an accepted hypothesis
struct Ranked
{
  int32_t index;
  double fine_response, coarse_response;
  double fine_mean[3];
  uint64_t known;
  double score;
};

// fine response descending, coarse response descending, index ascending
inline void rank_hypotheses(std::vector<Ranked> & h)
{
  std::sort(h.begin(), h.end(), [](const Ranked & a, const Ranked & b) {
      if (a.fine_response != b.fine_response) {return a.fine_response > b.fine_response;}
      if (a.coarse_response != b.coarse_response) {return a.coarse_response > b.coarse_response;}
      return a.index < b.index;
    });
}

// In rank order: a hypothesis with known > 0 and score < min_fit_score is dropped; then one is dropped as a duplicate when a KEPT one
// has (dx * dx) + (dy * dy) < merge_distance^2 and |NormalizeAngle(dh)| < merge_heading on the fine means (greedy: a dropped one
// suppresses nothing).  merge_distance <= 0: no suppression.  -> positions in `h` of the kept ones, in order.
inline std::vector<int32_t> suppress_hypotheses(const std::vector<Ranked> & h, double min_fit_score, double merge_distance, double merge_heading,
  int32_t * n_rejected_fit, int32_t * n_duplicates)
{
  std::vector<int32_t> kept;
  int32_t rejected = 0, duplicates = 0;
  for (size_t k = 0; k < h.size(); ++k) {
    if (h[k].known > 0 && h[k].score < min_fit_score) {++rejected; continue;}
    bool duplicate = false;
    if (merge_distance > 0) {
      for (int32_t q : kept) {
        const double dx = h[k].fine_mean[0] - h[q].fine_mean[0], dy = h[k].fine_mean[1] - h[q].fine_mean[1];
        const double dh = mapper::normalize_angle(h[k].fine_mean[2] - h[q].fine_mean[2]);
        if ((dx * dx) + (dy * dy) < merge_distance * merge_distance && std::fabs(dh) < merge_heading) {duplicate = true; break;}
      }
    }
    if (duplicate) {++duplicates; continue;}
    kept.push_back(static_cast<int32_t>(k));
  }
  if (n_rejected_fit) {*n_rejected_fit = rejected;}
  if (n_duplicates) {*n_duplicates = duplicates;}
  return kept;
}

// hypothesis i = seed i / n_headings at heading -pi + (i % n_headings) * (2 pi / n_headings)
inline double heading_of(size_t i, int32_t n_headings)
{
  return -mapper::kPi + static_cast<double>(i % static_cast<size_t>(n_headings)) * (mapper::k2Pi / static_cast<double>(n_headings));
}

// section 7d's default: ceil(2 pi / (2 * coarse_search_angle_offset)) headings
inline int32_t default_headings(double coarse_search_angle_offset)
{
  const double window = 2.0 * coarse_search_angle_offset;
  const double turns = window > 0 ? std::ceil(mapper::k2Pi / window) : 1.0;
  return (turns >= 1.0 && turns <= 4096.0) ? static_cast<int32_t>(turns) : 1;
}

// Mapper::Process' prediction (Mapper.cpp:2699-2703): Transform(last odometric, last corrected).TransformPose(odometric)
inline mapper::Pose predict_pose(const mapper::Pose & last_odometric, const mapper::Pose & last_corrected, const mapper::Pose & odometric)
{
  return mapper::transform_pose(last_odometric, last_corrected, odometric);
}
}  // namespace kh
