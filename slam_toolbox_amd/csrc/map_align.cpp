// Placing one map in another (kh_map_align): kh_merge_align's scheme with no scan of either map.  The probes
// are scans the MOVING map would produce (kh_map_raycast at its seeds), relocalized in the localizer's map; the candidates are ranked
// by how all the probes fit there.  The rules that need no device are in map_align_plan.hpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "map_align_plan.hpp"
#include "map_localizer_private.hpp"

using namespace kh;
using namespace kh::mapper;

namespace
{
// one probe: its seed, the robot and sensor pose in the moving map, the scan cast there
struct Probe
{
  int32_t seed;
  double robot[3], sensor[3];
  std::vector<double> ranges;
};

// (1) seeds of the moving map, one cast of all of them, the probes
int cast_probes(kh_map_localizer * loc, const kh_map_view & moving, const kh_map_align_params & params, std::vector<Probe> & probes)
{
  const int32_t pitch = seed_pitch(params.probe_spacing, moving.scale);
  if (pitch == 0) {
    set_error("kh_map_align: probe_spacing is more than " + std::to_string(kMaxSeedPitch) + " cells of the moving map");
    return KH_ERR_INVALID_ARG;
  }
  const SeedBlocks blocks = seed_blocks(moving.ox, moving.oy, moving.width, moving.height, pitch);
  std::vector<int32_t> local(static_cast<size_t>(blocks.count()));
  int rc = map_seed_blocks(loc->work, moving, pitch, blocks.bx0, blocks.by0, blocks.nx, blocks.ny, local.data(), nullptr);
  if (rc) {return rc;}
  const std::vector<Seed> seeds = compact_seeds(blocks, pitch, local.data(), moving.anchor[0], moving.anchor[1], moving.scale, nullptr, 0.0);
  if (seeds.empty()) {return KH_OK;}
  if (seeds.size() > static_cast<size_t>(INT32_MAX)) {set_error("kh_map_align: more than 2^31 seeds"); return KH_ERR_INVALID_ARG;}
  const size_t nb = static_cast<size_t>(loc->laser.n);
  std::vector<double> robots(3 * seeds.size()), sensors(3 * seeds.size());
  for (size_t k = 0; k < seeds.size(); ++k) {
    Pose robot; robot.x = seeds[k].x; robot.y = seeds[k].y; robot.h = 0.0;
    put_pose(robot, &robots[3 * k]);
    put_pose(sensor_at(loc->laser, robot), &sensors[3 * k]);
  }
  const kh_laser laser = to_kh_laser(loc->laser);
  if (map_raycast_check(&moving, &laser, static_cast<int32_t>(seeds.size()), sensors.data(), params.max_unknown) != KH_OK) {return KH_ERR_INVALID_ARG;}
  std::vector<kh_ray_t> rays(seeds.size() * nb);
  rc = map_raycast(loc->work, moving, laser, static_cast<int32_t>(seeds.size()), sensors.data(), params.max_unknown,
      ray_no_return(laser.range_threshold, laser.maximum_range), rays.data(), nullptr);
  if (rc) {return rc;}
  std::vector<int32_t> hits(seeds.size(), 0);
  for (size_t k = 0; k < seeds.size(); ++k) {
    for (size_t b = 0; b < nb; ++b) {hits[k] += rays[k * nb + b].code == KH_RAY_HIT ? 1 : 0;}
  }
  for (int32_t k : align_pick_probes(hits, params.n_probes)) {
    Probe p;
    p.seed = k;
    std::copy(&robots[3 * static_cast<size_t>(k)], &robots[3 * static_cast<size_t>(k)] + 3, p.robot);
    std::copy(&sensors[3 * static_cast<size_t>(k)], &sensors[3 * static_cast<size_t>(k)] + 3, p.sensor);
    p.ranges.resize(nb);
    for (size_t b = 0; b < nb; ++b) {p.ranges[b] = rays[static_cast<size_t>(k) * nb + b].range;}
    probes.push_back(std::move(p));
  }
  return KH_OK;
}

// (2) every probe relocalized in the localizer's map: the candidates after `initial`
int relocalize_probes(kh_map_localizer * loc, const kh_map_align_params & params, const std::vector<Probe> & probes, std::vector<kh_map_align_cand> & cands)
{
  kh_map_relocalize_params relocalize = params.relocalize;
  relocalize.top_k = params.top_k;
  std::vector<kh_map_hyp> hyps(static_cast<size_t>(params.top_k));
  for (const Probe & probe : probes) {
    kh_map_relocalize_summary summary;
    const int rc = kh_map_localizer_relocalize(loc, probe.ranges.data(), &relocalize, hyps.data(), params.top_k, &summary);
    if (rc) {return rc;}
    for (int32_t h = 0; h < summary.n_returned; ++h) {
      double correction[3];
      align_correction(hyps[static_cast<size_t>(h)].robot_pose, probe.robot, correction);
      if (!std::isfinite(correction[0]) || !std::isfinite(correction[1]) || !std::isfinite(correction[2])) {
        set_error("kh_map_align: a candidate correction is not finite");
        return KH_ERR_INVALID_ARG;
      }
      cands.push_back(align_candidate(correction, probe.seed, h, hyps[static_cast<size_t>(h)].fine_response));
    }
  }
  return KH_OK;
}

// (3) every candidate fitted with every probe: one k_map_fit launch per probe with all candidates as poses, the counters summed
int fit_candidates(kh_map_localizer * loc, const std::vector<Probe> & probes, const std::vector<kh_map_align_cand> & cands, std::vector<uint64_t> & sums)
{
  const size_t n = cands.size();
  sums.assign(n * kFitCounters, uint64_t{0});
  std::vector<double> poses(3 * n);
  std::vector<uint64_t> counts(n * kFitCounters);
  for (const Probe & probe : probes) {
    for (size_t i = 0; i < n; ++i) {
      const double * c = cands[i].correction;
      AlignRigid(c[0], c[1], c[2]).pose(probe.sensor, &poses[3 * i]);
    }
    const int rc = localizer_fit_counts(loc, probe.ranges.data(), n, poses.data(), counts.data(), nullptr);
    if (rc) {return rc;}
    for (size_t k = 0; k < counts.size(); ++k) {sums[k] += counts[k];}
  }
  return KH_OK;
}
}  // namespace

extern "C" {

void kh_map_align_params_default(const kh_map_localizer * loc, kh_map_align_params * p)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  kh_map_relocalize_params_default(loc ? &loc->p : nullptr, &p->relocalize);
  p->probe_spacing = p->relocalize.seed_spacing;
  p->n_probes = 3; p->top_k = 4; p->max_unknown = 20; p->min_known = 0;
}

int kh_map_align(kh_map_localizer * loc, const kh_map_view * moving, const kh_map_align_params * params, kh_map_align_cand * out, int32_t cap,
  int32_t * n_candidates, double times_ms[4])
{
  if (!params || !n_candidates || cap < 0 || (cap > 0 && !out)) {return KH_ERR_INVALID_ARG;}
  *n_candidates = 0;
  if (times_ms) {std::fill(times_ms, times_ms + 4, 0.0);}
  if (map_view_check(moving) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (!align_params_ok(*params)) {
    set_error("kh_map_align: probe_spacing > 0, n_probes >= 1, top_k >= 1, max_unknown >= -1, a finite initial and valid relocalization "
      "parameters are required");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!loc) {return KH_ERR_INVALID_ARG;}
  if (!loc->has_map) {set_error("kh_map_align: no map set"); return KH_ERR_NOT_FOUND;}
  if (moving->device != loc->device) {set_error("kh_map_align: the moving view lies on another device than the localizer"); return KH_ERR_INVALID_ARG;}
  const auto t_begin = std::chrono::steady_clock::now();
  std::vector<Probe> probes;
  int rc = cast_probes(loc, *moving, *params, probes);
  if (rc) {return rc;}
  const double cast_ms = ms_since(t_begin);
  std::vector<kh_map_align_cand> cands(1, align_candidate(params->initial, -1, -1, 0.0));
  const auto t_relocalize = std::chrono::steady_clock::now();
  rc = relocalize_probes(loc, *params, probes, cands);
  if (rc) {return rc;}
  const double relocalize_ms = ms_since(t_relocalize);
  if (cands.size() > static_cast<size_t>(INT32_MAX)) {set_error("kh_map_align: too many candidates"); return KH_ERR_INVALID_ARG;}
  const auto t_fit = std::chrono::steady_clock::now();
  std::vector<uint64_t> sums;
  rc = fit_candidates(loc, probes, cands, sums);
  if (rc) {return rc;}
  const double fit_ms = ms_since(t_fit);
  align_rank(cands, sums, params->min_known);
  const int32_t n = static_cast<int32_t>(cands.size());
  std::copy(cands.begin(), cands.begin() + std::min(cap, n), out);
  *n_candidates = n;
  if (times_ms) {times_ms[0] = cast_ms; times_ms[1] = relocalize_ms; times_ms[2] = fit_ms; times_ms[3] = ms_since(t_begin);}
  return KH_OK;
}

}  // extern "C"
