// Global relocalization on the mapper front end: TryCloseLoop's test (Mapper.cpp:1515-1549) for one scan
// placed at poses taken from the map -- a seed vertex per cell of a lattice, n_headings headings each -- instead of at its
// odometric pose.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>

#include "graph_internal.hpp"
#include "map_localize_plan.hpp"     // heading_of
#include "mapper_private.hpp"

namespace kh
{
namespace mapper
{
namespace
{
// what the two matches of one hypothesis answered: coarse / fine mean, covariance, response, and whether the coarse gate was passed
struct Result {double cm[3], cc[9], cr, fm[3], fc[9], fr; int32_t passed;};

// (1) where to try: seeds and their bases, as positions in the store's scan list
int relocalize_candidates(kh_mapper * m, const kh_relocalize_params * params, std::chrono::steady_clock::time_point t_begin, int32_t n_headings,
  std::vector<int32_t> & seeds, std::vector<int32_t> & base_begin, std::vector<int32_t> & base_idx, kh_relocalize_summary * summary)
{
  int rc = graph_relocalize_candidates(m->graph, params->seed_spacing, m->p.loop_search_maximum_distance, params->max_base,
      params->radius > 0 ? params->center_xy : nullptr, params->radius, seeds, base_begin, base_idx);
  if (rc) {return rc;}
  summary->kernel_ms = kh_graph_last_relocalize_kernel_ms(m->graph);
  summary->candidates_ms = ms_since(t_begin);
  const size_t n_hyp = seeds.size() * static_cast<size_t>(n_headings);
  if (n_hyp > static_cast<size_t>(0x7fffffff)) {set_error("kh_mapper_relocalize: more than 2^31 hypotheses"); return KH_ERR_INVALID_ARG;}
  summary->n_seeds = static_cast<int32_t>(seeds.size()); summary->n_hypotheses = static_cast<int32_t>(n_hyp);
  for (int32_t v : base_idx) {
    if (v < 0 || v >= static_cast<int32_t>(m->alive.size())) {set_error("kh_mapper_relocalize: base index out of range"); return KH_ERR_HIP;}
  }
  return KH_OK;
}

// (2) the hypotheses in pieces of max_candidates per member; hypothesis i goes to member i % members, each member runs
// kh_loop_closure_batch on its own loop / sequential matcher pair against the scan copies of its own device
int relocalize_batches(kh_mapper * m, const double * ranges, int32_t n_headings, const std::vector<int32_t> & seeds,
  const std::vector<int32_t> & base_begin, const std::vector<int32_t> & base_idx, std::vector<Result> & results, kh_relocalize_summary * summary)
{
  const size_t n_hyp = results.size(), nh = static_cast<size_t>(n_headings);
  const size_t nm = m->member_device.size(), nb = static_cast<size_t>(m->laser.n);
  const size_t piece = static_cast<size_t>(m->max_candidates) * nm;
  std::vector<double> poses, points;
  for (size_t at = 0; at < n_hyp; at += piece) {
    const size_t np = std::min(piece, n_hyp - at);
    // the query scans of the piece: LocalizedRangeScan::Update at the hypothesis' sensor pose (n_beams libm sincos each, on the worker pool)
    const auto t_scans = std::chrono::steady_clock::now();
    poses.resize(3 * np); points.resize(2 * nb * np);
    for (size_t j = 0; j < np; ++j) {
      const size_t i = at + j;
      const MScan & seed = *m->scans[m->alive[seeds[i / nh]]];
      Pose robot; robot.x = seed.corrected.x; robot.y = seed.corrected.y; robot.h = heading_of(i, n_headings);
      put_pose(sensor_at(m->laser, robot), &poses[3 * j]);
    }
    scan_points_at(ranges, 0, m->laser.n, m->laser.min_angle, m->laser.ang_res, np, poses.data(), points.data(), nullptr);
    summary->scans_ms += ms_since(t_scans);
    const auto t_batch = std::chrono::steady_clock::now();
    struct Share
    {
      std::vector<size_t> hyp;                                 // hypotheses of this member, ascending
      std::vector<kh_scan> q, b;
      std::vector<int32_t> begin, passed;
      std::vector<double> cm, cc, cr, fm, fc, fr;
      int rc = KH_OK;
      std::string error;
    };
    std::vector<Share> shares(nm);
    for (size_t j = 0; j < np; ++j) {shares[(at + j) % nm].hyp.push_back(at + j);}
    for (size_t k = 0; k < nm; ++k) {
      Share & sh = shares[k];
      sh.begin.assign(1, 0);
      for (size_t i : sh.hyp) {
        const size_t j = i - at;
        kh_scan q;
        q.n = m->laser.n; q.ranges = ranges; q.points_xy = &points[2 * nb * j]; q.device_points_xy = nullptr;
        std::copy(&poses[3 * j], &poses[3 * j] + 3, q.sensor_pose);
        sh.q.push_back(q);
        const size_t seed = i / nh;
        for (int32_t t = base_begin[seed]; t < base_begin[seed + 1]; ++t) {
          MScan & s = *m->scans[m->alive[base_idx[t]]];
          kh_scan b = as_kh_scan(s);
          b.device_points_xy = resident_points(m, s, m->member_slot[k]);
          sh.b.push_back(b);
        }
        sh.begin.push_back(static_cast<int32_t>(sh.b.size()));
      }
      const size_t n = sh.hyp.size();
      sh.passed.assign(n, 0);
      sh.cm.assign(3 * n, 0.0); sh.cc.assign(9 * n, 0.0); sh.cr.assign(n, 0.0);
      sh.fm.assign(3 * n, 0.0); sh.fc.assign(9 * n, 0.0); sh.fr.assign(n, 0.0);
    }
    auto run = [&](size_t k) {
        Share & sh = shares[k];
        if (sh.hyp.empty()) {return;}
        sh.rc = kh_loop_closure_batch(kh_matcher_group_member(m->loop_group, static_cast<int32_t>(k)),
            kh_matcher_group_member(m->seq_group, static_cast<int32_t>(k)), static_cast<int32_t>(sh.hyp.size()), sh.q.data(), sh.b.data(),
            sh.begin.data(), m->laser.min_angle, m->laser.ang_res, m->p.loop_match_minimum_response_coarse,
            m->p.loop_match_maximum_variance_coarse, 1, sh.cm.data(), sh.cc.data(), sh.cr.data(), sh.passed.data(), sh.fm.data(),
            sh.fc.data(), sh.fr.data());
        if (sh.rc) {sh.error = kh_last_error();}                // the message is thread local: carried to the caller below
      };
    {
      std::vector<std::thread> workers;
      for (size_t k = 1; k < nm; ++k) {
        if (!shares[k].hyp.empty()) {workers.emplace_back(run, k);}
      }
      run(0);
      for (std::thread & w : workers) {w.join();}
    }
    summary->batch_ms += ms_since(t_batch);
    for (size_t k = 0; k < nm; ++k) {
      if (shares[k].rc) {set_error(shares[k].error); return shares[k].rc;}
    }
    for (size_t k = 0; k < nm; ++k) {
      const Share & sh = shares[k];
      for (size_t t = 0; t < sh.hyp.size(); ++t) {
        Result & r = results[sh.hyp[t]];
        std::copy(&sh.cm[3 * t], &sh.cm[3 * t] + 3, r.cm); std::copy(&sh.cc[9 * t], &sh.cc[9 * t] + 9, r.cc); r.cr = sh.cr[t];
        std::copy(&sh.fm[3 * t], &sh.fm[3 * t] + 3, r.fm); std::copy(&sh.fc[9 * t], &sh.fc[9 * t] + 9, r.fc); r.fr = sh.fr[t];
        r.passed = sh.passed[t];
      }
    }
  }
  return KH_OK;
}

// (3) acceptance and ranking
void relocalize_rank(const kh_mapper * m, const kh_relocalize_params * params, int32_t n_headings, const std::vector<int32_t> & seeds,
  const std::vector<Result> & results, kh_relocalize_hyp * out, int32_t cap, kh_relocalize_summary * summary)
{
  std::vector<int32_t> accepted;
  for (size_t i = 0; i < results.size(); ++i) {
    if (!results[i].passed) {continue;}
    summary->n_passed += 1;
    if (results[i].fr >= m->p.loop_match_minimum_response_fine) {accepted.push_back(static_cast<int32_t>(i));}
  }
  summary->n_accepted = static_cast<int32_t>(accepted.size());
  std::sort(accepted.begin(), accepted.end(), [&](int32_t a, int32_t b) {
      const Result & ra = results[a], & rb = results[b];
      if (ra.fr != rb.fr) {return ra.fr > rb.fr;}
      if (ra.cr != rb.cr) {return ra.cr > rb.cr;}
      return a < b;
    });
  const size_t n_out = std::min(accepted.size(), static_cast<size_t>(params->top_k > 0 ? std::min(params->top_k, cap) : cap));
  for (size_t k = 0; k < n_out; ++k) {
    const int32_t i = accepted[k];
    const Result & r = results[i];
    kh_relocalize_hyp & h = out[k];
    std::memset(&h, 0, sizeof(h));
    h.index = i; h.seed_scan = m->alive[seeds[static_cast<size_t>(i) / static_cast<size_t>(n_headings)]];
    h.heading = heading_of(static_cast<size_t>(i), n_headings);
    std::copy(r.cm, r.cm + 3, h.coarse_mean); std::copy(r.cc, r.cc + 9, h.coarse_cov); h.coarse_response = r.cr;
    std::copy(r.fm, r.fm + 3, h.fine_mean); std::copy(r.fc, r.fc + 9, h.fine_cov); h.fine_response = r.fr;
    put_pose(corrected_at(m->laser, to_pose(r.fm)), h.robot_pose);
  }
  summary->n_returned = static_cast<int32_t>(n_out);
}
}  // namespace
}  // namespace mapper
}  // namespace kh

using namespace kh;
using namespace kh::mapper;

extern "C" {

void kh_relocalize_params_default(const kh_mapper_params * mapper_params, kh_relocalize_params * p)
{
  if (!p) {return;}
  kh_mapper_params defaults;
  if (!mapper_params) {kh_mapper_params_default(&defaults); mapper_params = &defaults;}
  std::memset(p, 0, sizeof(*p));
  p->seed_spacing = mapper_params->loop_search_maximum_distance / 2;
  p->n_headings = 0;                                  // = ceil(2 pi / (2 * coarse_search_angle_offset)) of the mapper the call is made on
  p->max_base = 40;                                   // the upper chain length of BASELINE config 3
  p->top_k = 8;
  p->radius = 0.0;                                    // the whole map
}

int kh_mapper_relocalize(kh_mapper * m, const double * ranges, const kh_relocalize_params * params, kh_relocalize_hyp * out, int32_t cap,
  kh_relocalize_summary * summary)
{
  if (!ranges || !params || !summary || cap < 0 || (cap > 0 && !out)) {return KH_ERR_INVALID_ARG;}
  std::memset(summary, 0, sizeof(*summary));
  if (!(params->seed_spacing > 0) || !std::isfinite(params->seed_spacing) || params->n_headings < 0 || params->max_base < 1 || params->top_k < 0 ||
    !std::isfinite(params->radius) || !std::isfinite(params->center_xy[0]) || !std::isfinite(params->center_xy[1]))
  {
    set_error("kh_mapper_relocalize: seed_spacing > 0, n_headings >= 0, max_base >= 1, top_k >= 0 and finite values are required");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (m->failed) {
    set_error("kh_mapper_relocalize: an earlier Process call failed after its scan had entered the graph; the handle is unusable");
    return KH_ERR_SOLVER;
  }
  const auto t_begin = std::chrono::steady_clock::now();
  int32_t n_headings = params->n_headings;
  if (n_headings == 0) {
    const double window = 2.0 * m->p.match.coarse_search_angle_offset;
    const double turns = window > 0 ? std::ceil(k2Pi / window) : 1.0;
    n_headings = (turns >= 1.0 && turns <= 4096.0) ? static_cast<int32_t>(turns) : 1;
  }
  summary->n_headings = n_headings;
  // the graph store is the mapper's own view of itself (rebuilt from the scans whenever an edit outran it): bringing it up to date
  // changes nothing a Process call computes
  if (m->graph_dirty) {const int rc = sync_graph(m); if (rc) {return rc;}}
  if (m->alive.empty()) {summary->total_ms = ms_since(t_begin); return KH_OK;}
  std::vector<int32_t> seeds, base_begin, base_idx;
  int rc = relocalize_candidates(m, params, t_begin, n_headings, seeds, base_begin, base_idx, summary);
  if (rc) {return rc;}
  std::vector<Result> results(static_cast<size_t>(summary->n_hypotheses));
  rc = relocalize_batches(m, ranges, n_headings, seeds, base_begin, base_idx, results, summary);
  if (rc) {return rc;}
  relocalize_rank(m, params, n_headings, seeds, results, out, cap, summary);
  summary->total_ms = ms_since(t_begin);
  return KH_OK;
}

}  // extern "C"
