// The map localizer (kh_map_localizer_*): global relocalization and pose tracking of one laser in a map that is
// nothing but a kh_map_view -- section 7d's hypotheses (seeds x headings, TryCloseLoop's coarse match, gate and fine match,
// Mapper.cpp:1515-1549) with kh_map_seeds in the place of the seed vertices and kh_matcher_match_map_batch in the place of the chain
// matches, kh_map_fit as the health signal, and Mapper::Process' odometric prediction (Mapper.cpp:2699-2703) for the step from scan
// to scan.  The rules that need no device are in map_localize_plan.hpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "map_localizer_private.hpp"

using namespace kh;
using namespace kh::mapper;

namespace
{
// what the two matches of one hypothesis answered
struct Result {double cm[3], cc[9], cr, fm[3], fc[9], fr; int32_t passed;};

bool finite3(const double * v) {return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);}

// n MatchScans of the same readings at n sensor poses against the map, in batches of max_batch; the readings are placed with
// kh_scan_points (n_beams libm sincos per pose, on the worker pool)
int match_poses(kh_map_localizer * loc, kh_matcher * matcher, const double * ranges, size_t n, const double * poses, bool penalize, bool refine,
  double * means, double * covs, double * responses)
{
  const size_t nb = static_cast<size_t>(loc->laser.n), piece = static_cast<size_t>(loc->max_batch);
  std::vector<double> points;
  std::vector<kh_scan> q;
  std::vector<int32_t> status;
  for (size_t at = 0; at < n; at += piece) {
    const size_t np = std::min(piece, n - at);
    points.resize(2 * nb * np); q.resize(np); status.assign(np, KH_OK);
    scan_points_at(ranges, 0, loc->laser.n, loc->laser.min_angle, loc->laser.ang_res, np, poses + 3 * at, points.data(), nullptr);
    for (size_t j = 0; j < np; ++j) {
      q[j].n = loc->laser.n; q[j].ranges = ranges; q[j].points_xy = &points[2 * nb * j]; q[j].device_points_xy = nullptr;
      std::copy(poses + 3 * (at + j), poses + 3 * (at + j) + 3, q[j].sensor_pose);
    }
    int rc = kh_matcher_match_map_batch(matcher, static_cast<int32_t>(np), q.data(), &loc->view, penalize ? 1 : 0, refine ? 1 : 0, means + 3 * at,
        covs + 9 * at, responses + at, status.data());
    for (size_t j = 0; j < np && rc == KH_OK; ++j) {rc = status[j];}
    if (rc) {return rc;}
  }
  return KH_OK;
}

// kh_map_fit of the readings at n sensor poses on the localizer's own work buffers
int fit_poses(kh_map_localizer * loc, const double * ranges, size_t n, const double * poses, kh_merge_fit_t * out, double * kernel_ms)
{
  std::vector<uint64_t> counts(n * kFitCounters);
  const int rc = localizer_fit_counts(loc, ranges, n, poses, counts.data(), kernel_ms);
  if (rc) {return rc;}
  for (size_t k = 0; k < n; ++k) {out[k] = fit_derive(&counts[k * kFitCounters]);}
  return KH_OK;
}
}  // namespace

namespace kh
{
int localizer_fit_counts(kh_map_localizer * loc, const double * ranges, size_t n, const double * poses, uint64_t * counts, double * kernel_ms)
{
  double unused_ms = 0.0;
  if (!kernel_ms) {kernel_ms = &unused_ms;}
  *kernel_ms = 0.0;
  if (n == 0) {return KH_OK;}
  // (the angles of a localizer's laser are judged nowhere, here neither: 0 stands for them)
  const FitInputs inputs = fit_inputs_check(loc->laser.range_threshold, loc->laser.min_range, loc->laser.max_range, 0.0, 0.0, n, poses,
      loc->view.anchor[0], loc->view.anchor[1], loc->view.scale);
  if (inputs.failed) {
    set_error(fit_inputs_text(inputs, "map localizer", "the laser's range_threshold * scale must stay below 2^20 cells of this map",
      "a matched pose is not finite or lies more than 2^30 cells from the map's anchor"));
    return KH_ERR_INVALID_ARG;
  }
  const size_t nb = static_cast<size_t>(loc->laser.n);
  std::vector<double> points(2 * nb * n), sensor_xy(2 * n);
  scan_points_at(ranges, 0, loc->laser.n, loc->laser.min_angle, loc->laser.ang_res, n, poses, points.data(), sensor_xy.data());
  const int rc = map_fit_counts(loc->work, loc->view, loc->laser.n, ranges, static_cast<int32_t>(n), points.data(), sensor_xy.data(),
      loc->laser.range_threshold, loc->laser.min_range, loc->laser.max_range, counts, kernel_ms);
  if (rc) {return rc;}
  loc->stats.poses_fitted += static_cast<int64_t>(n);
  loc->stats.fit_kernel_ms += *kernel_ms;
  return KH_OK;
}
}  // namespace kh

namespace
{

// (1) where to try
int relocalize_seeds(kh_map_localizer * loc, const kh_map_relocalize_params * params, std::vector<Seed> & seeds, kh_map_relocalize_summary * summary)
{
  const int32_t pitch = seed_pitch(params->seed_spacing, loc->view.scale);
  if (pitch == 0) {
    set_error("kh_map_localizer_relocalize: seed_spacing is more than " + std::to_string(kMaxSeedPitch) + " cells of this map");
    return KH_ERR_INVALID_ARG;
  }
  const SeedBlocks blocks = seed_blocks(loc->view.ox, loc->view.oy, loc->view.width, loc->view.height, pitch);
  std::vector<int32_t> local(static_cast<size_t>(blocks.count()));
  const int rc = map_seed_blocks(loc->work, loc->view, pitch, blocks.bx0, blocks.by0, blocks.nx, blocks.ny, local.data(), &summary->seed_kernel_ms);
  if (rc) {return rc;}
  loc->stats.seed_kernel_ms += summary->seed_kernel_ms;
  seeds = compact_seeds(blocks, pitch, local.data(), loc->view.anchor[0], loc->view.anchor[1], loc->view.scale,
      params->radius > 0 ? params->center_xy : nullptr, params->radius);
  return KH_OK;
}

// (2) the two matches of every hypothesis: all coarse matches, the gate, then the fine matches of those that passed
int relocalize_matches(kh_map_localizer * loc, const double * ranges, const kh_map_relocalize_params * params, int32_t n_headings,
  const std::vector<Seed> & seeds, std::vector<Result> & results, kh_map_relocalize_summary * summary)
{
  const size_t n = results.size();
  std::vector<double> poses(3 * n), means(3 * n), covs(9 * n), responses(n);
  for (size_t i = 0; i < n; ++i) {
    const Seed & seed = seeds[i / static_cast<size_t>(n_headings)];
    Pose robot; robot.x = seed.x; robot.y = seed.y; robot.h = heading_of(i, n_headings);
    put_pose(sensor_at(loc->laser, robot), &poses[3 * i]);
  }
  const auto t_coarse = std::chrono::steady_clock::now();
  int rc = match_poses(loc, loc->loop, ranges, n, poses.data(), false, false, means.data(), covs.data(), responses.data());
  summary->coarse_ms = ms_since(t_coarse);
  if (rc) {return rc;}
  std::vector<size_t> passed;
  for (size_t i = 0; i < n; ++i) {
    Result & r = results[i];
    std::memset(&r, 0, sizeof(r));
    std::copy(&means[3 * i], &means[3 * i] + 3, r.cm); std::copy(&covs[9 * i], &covs[9 * i] + 9, r.cc); r.cr = responses[i];
    // Mapper.cpp:1519-1521
    r.passed = (r.cr > params->minimum_response_coarse && r.cc[0] < params->maximum_variance_coarse && r.cc[4] < params->maximum_variance_coarse) ? 1 : 0;
    if (r.passed) {passed.push_back(i);}
  }
  summary->n_passed = static_cast<int32_t>(passed.size());
  const size_t m = passed.size();
  std::vector<double> fine_poses(3 * m), fm(3 * m), fc(9 * m), fr(m);
  for (size_t j = 0; j < m; ++j) {std::copy(results[passed[j]].cm, results[passed[j]].cm + 3, &fine_poses[3 * j]);}    // tmpScan.SetSensorPose(bestPose)
  const auto t_fine = std::chrono::steady_clock::now();
  rc = match_poses(loc, loc->seq, ranges, m, fine_poses.data(), false, true, fm.data(), fc.data(), fr.data());
  summary->fine_ms = ms_since(t_fine);
  if (rc) {return rc;}
  for (size_t j = 0; j < m; ++j) {
    Result & r = results[passed[j]];
    std::copy(&fm[3 * j], &fm[3 * j] + 3, r.fm); std::copy(&fc[9 * j], &fc[9 * j] + 9, r.fc); r.fr = fr[j];
  }
  return KH_OK;
}

// (3) acceptance, ranking, fit, suppression
int relocalize_answer(kh_map_localizer * loc, const double * ranges, const kh_map_relocalize_params * params, int32_t n_headings,
  const std::vector<Seed> & seeds, const std::vector<Result> & results, kh_map_hyp * out, int32_t cap, kh_map_relocalize_summary * summary)
{
  std::vector<Ranked> ranked;
  for (size_t i = 0; i < results.size(); ++i) {
    const Result & r = results[i];
    if (!r.passed || !(r.fr >= params->minimum_response_fine)) {continue;}
    Ranked h;
    h.index = static_cast<int32_t>(i); h.fine_response = r.fr; h.coarse_response = r.cr;
    std::copy(r.fm, r.fm + 3, h.fine_mean);
    h.known = 0; h.score = 0.0;
    ranked.push_back(h);
  }
  summary->n_accepted = static_cast<int32_t>(ranked.size());
  rank_hypotheses(ranked);
  std::vector<double> poses(3 * ranked.size());
  for (size_t k = 0; k < ranked.size(); ++k) {std::copy(ranked[k].fine_mean, ranked[k].fine_mean + 3, &poses[3 * k]);}
  std::vector<kh_merge_fit_t> fits(ranked.size());
  const int rc = fit_poses(loc, ranges, ranked.size(), poses.data(), fits.data(), &summary->fit_kernel_ms);
  if (rc) {return rc;}
  for (size_t k = 0; k < ranked.size(); ++k) {ranked[k].known = fits[k].known; ranked[k].score = fits[k].score;}
  const std::vector<int32_t> kept = suppress_hypotheses(ranked, params->min_fit_score, params->merge_distance, params->merge_heading,
      &summary->n_rejected_fit, &summary->n_duplicates);
  const size_t n_out = std::min(kept.size(), static_cast<size_t>(params->top_k > 0 ? std::min(params->top_k, cap) : cap));
  for (size_t k = 0; k < n_out; ++k) {
    const Ranked & rk = ranked[kept[k]];
    const Result & r = results[rk.index];
    const Seed & seed = seeds[static_cast<size_t>(rk.index) / static_cast<size_t>(n_headings)];
    kh_map_hyp & h = out[k];
    std::memset(&h, 0, sizeof(h));
    h.index = rk.index; h.seed_cell[0] = seed.i; h.seed_cell[1] = seed.j;
    h.heading = heading_of(static_cast<size_t>(rk.index), n_headings);
    std::copy(r.cm, r.cm + 3, h.coarse_mean); std::copy(r.cc, r.cc + 9, h.coarse_cov); h.coarse_response = r.cr;
    std::copy(r.fm, r.fm + 3, h.fine_mean); std::copy(r.fc, r.fc + 9, h.fine_cov); h.fine_response = r.fr;
    put_pose(corrected_at(loc->laser, to_pose(r.fm)), h.robot_pose);
    h.fit = fits[kept[k]];
  }
  summary->n_returned = static_cast<int32_t>(n_out);
  return KH_OK;
}
}  // namespace

extern "C" {

int kh_map_localizer_create(const kh_mapper_params * params, const kh_laser * laser, int32_t device, int32_t max_batch, kh_map_localizer ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (!params || !laser || laser->n_beams <= 0 || max_batch < 1 || device < 0) {return KH_ERR_INVALID_ARG;}
  if (require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  std::unique_ptr<kh_map_localizer> loc(new kh_map_localizer());
  loc->p = *params; loc->device = device; loc->max_batch = max_batch;
  loc->laser = to_laser(*laser);
  std::memset(&loc->stats, 0, sizeof(loc->stats));
  std::memset(&loc->view, 0, sizeof(loc->view));
  auto fail = [&](int rc) {kh_map_localizer_destroy(loc.release()); return rc;};
  int rc = kh_matcher_create(params->correlation_search_space_dimension, params->correlation_search_space_resolution,
      params->correlation_search_space_smear_deviation, laser->range_threshold, device, max_batch, &loc->seq);
  if (rc) {return fail(rc);}
  rc = kh_matcher_create(params->loop_search_space_dimension, params->loop_search_space_resolution, params->loop_search_space_smear_deviation,
      laser->range_threshold, device, max_batch, &loc->loop);
  if (rc) {return fail(rc);}
  rc = kh_matcher_set_params(loc->seq, &params->match); if (rc) {return fail(rc);}
  rc = kh_matcher_set_params(loc->loop, &params->match); if (rc) {return fail(rc);}
  loc->work = map_work_create(device);
  if (!loc->work) {return fail(KH_ERR_HIP);}
  *out = loc.release();
  return KH_OK;
}

void kh_map_localizer_destroy(kh_map_localizer * loc)
{
  if (!loc) {return;}
  if (loc->seq) {kh_matcher_destroy(loc->seq);}
  if (loc->loop) {kh_matcher_destroy(loc->loop);}
  map_work_destroy(loc->work);
  delete loc;
}

int kh_map_localizer_set_map(kh_map_localizer * loc, const kh_map_view * view)
{
  if (!loc || map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (view->device != loc->device) {set_error("the map view lies on another device than the localizer"); return KH_ERR_INVALID_ARG;}
  loc->view = *view;
  loc->has_map = true;
  return KH_OK;
}

void kh_map_relocalize_params_default(const kh_mapper_params * mapper_params, kh_map_relocalize_params * p)
{
  if (!p) {return;}
  kh_mapper_params defaults;
  if (!mapper_params) {kh_mapper_params_default(&defaults); mapper_params = &defaults;}
  std::memset(p, 0, sizeof(*p));
  p->seed_spacing = mapper_params->loop_search_space_dimension / 4;       // a block's diagonal stays inside the coarse half window
  p->n_headings = 0;                                   // = ceil(2 pi / (2 * coarse_search_angle_offset)) of the localizer the call is made on
  p->top_k = 8;
  p->radius = 0.0;                                     // the whole map
  p->minimum_response_coarse = mapper_params->loop_match_minimum_response_coarse;
  p->maximum_variance_coarse = mapper_params->loop_match_maximum_variance_coarse;
  p->minimum_response_fine = mapper_params->loop_match_minimum_response_fine;
  p->min_fit_score = 0.0;
  p->merge_distance = mapper_params->loop_search_space_resolution;
  p->merge_heading = mapper_params->match.coarse_angle_resolution;
}

int kh_map_localizer_relocalize(kh_map_localizer * loc, const double * ranges, const kh_map_relocalize_params * params, kh_map_hyp * out,
  int32_t cap, kh_map_relocalize_summary * summary)
{
  if (!ranges || !params || !summary || cap < 0 || (cap > 0 && !out)) {return KH_ERR_INVALID_ARG;}
  std::memset(summary, 0, sizeof(*summary));
  if (!relocalize_params_ok(*params)) {
    set_error("kh_map_localizer_relocalize: seed_spacing > 0, 0 <= n_headings <= 4096, top_k >= 0, a finite region and no NaN are required");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!loc) {return KH_ERR_INVALID_ARG;}
  if (!loc->has_map) {set_error("kh_map_localizer_relocalize: no map set"); return KH_ERR_NOT_FOUND;}
  const auto t_begin = std::chrono::steady_clock::now();
  const int32_t n_headings = params->n_headings > 0 ? params->n_headings : default_headings(loc->p.match.coarse_search_angle_offset);
  summary->n_headings = n_headings;
  std::vector<Seed> seeds;
  int rc = relocalize_seeds(loc, params, seeds, summary);
  if (rc) {return rc;}
  const size_t n_hyp = seeds.size() * static_cast<size_t>(n_headings);
  if (n_hyp > static_cast<size_t>(0x7fffffff)) {set_error("kh_map_localizer_relocalize: more than 2^31 hypotheses"); return KH_ERR_INVALID_ARG;}
  summary->n_seeds = static_cast<int32_t>(seeds.size()); summary->n_hypotheses = static_cast<int32_t>(n_hyp);
  std::vector<Result> results(n_hyp);
  if (n_hyp > 0) {
    rc = relocalize_matches(loc, ranges, params, n_headings, seeds, results, summary);
    if (rc) {return rc;}
    rc = relocalize_answer(loc, ranges, params, n_headings, seeds, results, out, cap, summary);
    if (rc) {return rc;}
  }
  summary->total_ms = ms_since(t_begin);
  loc->stats.relocalizations += 1; loc->stats.hypotheses += static_cast<int64_t>(n_hyp); loc->stats.relocalize_ms += summary->total_ms;
  return KH_OK;
}

int kh_map_localizer_set_pose(kh_map_localizer * loc, const double robot_pose[3], const double odometric_pose[3])
{
  if (!loc || !robot_pose || !odometric_pose || !finite3(robot_pose) || !finite3(odometric_pose)) {return KH_ERR_INVALID_ARG;}
  loc->robot = to_pose(robot_pose); loc->odometric = to_pose(odometric_pose);
  loc->has_pose = true;
  return KH_OK;
}

int kh_map_localizer_get_pose(const kh_map_localizer * loc, double robot_pose[3], double odometric_pose[3])
{
  if (!loc) {return KH_ERR_INVALID_ARG;}
  if (!loc->has_pose) {set_error("kh_map_localizer_get_pose: no pose set"); return KH_ERR_NOT_FOUND;}
  if (robot_pose) {put_pose(loc->robot, robot_pose);}
  if (odometric_pose) {put_pose(loc->odometric, odometric_pose);}
  return KH_OK;
}

int kh_map_localizer_process(kh_map_localizer * loc, const double * ranges, const double odometric_pose[3], kh_map_track_t * out)
{
  if (!ranges || !odometric_pose || !out || !finite3(odometric_pose)) {return KH_ERR_INVALID_ARG;}
  std::memset(out, 0, sizeof(*out));
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!loc) {return KH_ERR_INVALID_ARG;}
  if (!loc->has_map) {set_error("kh_map_localizer_process: no map set"); return KH_ERR_NOT_FOUND;}
  if (!loc->has_pose) {set_error("kh_map_localizer_process: no pose set"); return KH_ERR_NOT_FOUND;}
  const auto t_begin = std::chrono::steady_clock::now();
  const Pose odometric = to_pose(odometric_pose);
  const Pose predicted = predict_pose(loc->odometric, loc->robot, odometric);
  double start[3];
  put_pose(sensor_at(loc->laser, predicted), start);
  const auto t_match = std::chrono::steady_clock::now();
  int rc = match_poses(loc, loc->seq, ranges, 1, start, true, true, out->sensor_pose, out->covariance, &out->response);
  loc->stats.match_ms += ms_since(t_match);
  if (rc) {return rc;}
  rc = fit_poses(loc, ranges, 1, out->sensor_pose, &out->fit, nullptr);
  if (rc) {return rc;}
  const Pose robot = corrected_at(loc->laser, to_pose(out->sensor_pose));
  put_pose(predicted, out->predicted_pose);
  put_pose(robot, out->robot_pose);
  loc->robot = robot; loc->odometric = odometric;          // always adopted, as Mapper::Process adopts its match
  loc->stats.steps += 1; loc->stats.process_ms += ms_since(t_begin);
  return KH_OK;
}

int kh_map_localizer_stats(const kh_map_localizer * loc, kh_map_localizer_stats_t * out)
{
  if (!loc || !out) {return KH_ERR_INVALID_ARG;}
  *out = loc->stats;
  return KH_OK;
}

}  // extern "C"
