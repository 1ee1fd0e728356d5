// The mapper's loop search: MapperGraph::TryCloseLoop (lib/karto_sdk/src/Mapper.cpp:1500-1561) and the covariance gate in front of
// it.
//
// TryCloseLoop is where the GPU changes the SHAPE of the computation without changing its result: the reference matches
// one candidate chain after another; here all chains FindPossibleLoopClosure would return for the current poses are
// enumerated in one kernel, coarse-matched in one kh_matcher_match_batch, the ones passing the coarse gate fine-matched
// in a second batch, and the results consumed in the reference's order up to the first accepted closure.  CorrectPoses
// then moves every pose, so what was computed for later chains is discarded and the enumeration resumes behind the
// accepted chain with the new poses (closures are rare, the speculation almost always commits).
#include <algorithm>
#include <cmath>

#include "mapper_private.hpp"
#include "spa_internal.hpp"

namespace kh
{
namespace mapper
{
namespace
{
// ---- the covariance gate of the loop search ----
// Whether the difference covariances can change anything: with covariance_scale = 0 or both chi2 values null every row is zero and
// the jump test sees the matcher's covariance alone, so no column pass runs -- a pass re-analyses the solver's graph, which the
// next Compute() would inherit, and a gate with null parameters must leave the run as it is, bit for bit.
bool gate_needs_covariances(const kh_loop_gate_params & g)
{
  return g.covariance_scale != 0.0 && (g.chi2_position > 0.0 || g.chi2_jump > 0.0);
}

// One refresh: a column pass with the current scan as the query, then D = cov(x_i - x_scan) of every scan alive that the solver
// knows (k_cov_difference).  gated = false: the pass was refused (KH_ERR_SOLVER) or the solver does not know the scan.
int gate_refresh(kh_mapper * m, int32_t scan_id, bool & gated)
{
  gated = false;
  m->gate_d.assign(9 * m->scans.size(), 0.0);
  if (m->adj[scan_id].empty()) {return KH_OK;}           // no constraint yet (the first scan): every D is zero, the refresh stays owed
  const auto t0 = std::chrono::steady_clock::now();
  int rc = kh_spa_compute_covariance_columns(m->solver, 1, &scan_id, nullptr);
  if (rc == KH_ERR_SOLVER) {m->gate_stats.ungated_searches += 1; return KH_OK;}
  if (rc == KH_ERR_NOT_FOUND) {return KH_OK;}            // the solver took none of the scan's constraints: as without constraints
  if (rc) {return rc;}
  std::vector<int32_t> ids;
  for (int32_t id : m->alive) {
    if (spa_covariance_has_node(m->solver, id)) {ids.push_back(id);}
  }
  std::vector<double> d(9 * ids.size());
  rc = kh_spa_get_difference_covariances(m->solver, scan_id, static_cast<int32_t>(ids.size()), ids.data(), d.data());
  if (rc) {return rc;}
  for (size_t k = 0; k < ids.size(); ++k) {std::copy(d.begin() + 9 * k, d.begin() + 9 * k + 9, m->gate_d.begin() + 9 * static_cast<size_t>(ids[k]));}
  m->gate_stats.column_passes += 1;
  m->gate_stats.column_ms += ms_since(t0);
  m->gate_age = 0; m->gate_due = false;
  gated = true;
  return KH_OK;
}

// The rows of one enumeration, in list order: G = covariance_scale D, scaled down where s (Gxx + Gyy) exceeds (max_reach / r)^2 - 1
// (s = chi2_position / r^2), so that no semi-axis sqrt(r^2 + chi2 lambda_max(G)) exceeds max_reach: lambda_max <= the trace.
void gate_prepare_rows(kh_mapper * m)
{
  const kh_loop_gate_params & g = m->gate;
  const double r = m->p.loop_search_maximum_distance;
  const double s = g.chi2_position / (r * r);
  const double limit = std::max(0.0, (g.max_reach / r) * (g.max_reach / r) - 1.0);
  m->gate_rows.assign(9 * m->alive.size(), 0.0);
  for (size_t c = 0; c < m->alive.size(); ++c) {
    const size_t id = static_cast<size_t>(m->alive[c]);
    if (9 * id + 9 > m->gate_d.size()) {continue;}       // appended since the refresh
    double * row = &m->gate_rows[9 * c];
    for (int k = 0; k < 9; ++k) {row[k] = g.covariance_scale * m->gate_d[9 * id + k];}
    const double reach = s * (row[0] + row[4]);
    if (reach > limit) {
      const double f = limit / reach;
      for (int k = 0; k < 9; ++k) {row[k] *= f;}
    }
    const double half = 0.5 * (row[0] - row[4]);
    const double lambda = 0.5 * (row[0] + row[4]) + std::sqrt(half * half + row[1] * row[1]);
    if (lambda > 0.0 && std::isfinite(lambda)) {
      m->gate_stats.max_semi_axis = std::max(m->gate_stats.max_semi_axis, std::sqrt(r * r + g.chi2_position * lambda));
    }
  }
}

// The jump test: e = mean - current sensor pose (angle normalised) against covariance_scale D3(i*) + C_fine, i* the chain's scan
// LinkChainToScan would link to once the scan stands at `mean`.  true: e^T M^-1 e > chi2_jump, or M is not positive definite.
bool gate_jump_rejects(kh_mapper * m, const MScan & scan, const std::vector<int32_t> & chain, const double mean[3], const double cov[9])
{
  const Pose sp = scan.sensor_pose();
  const double e[3] = {mean[0] - sp.x, mean[1] - sp.y, normalize_angle(mean[2] - sp.h)};
  MScan moved;
  moved.ranges = scan.ranges;
  moved.corrected = corrected_at(m->laser, to_pose(mean));
  update_scan(moved, m->laser);
  double xy[2];
  reference_xy(m, moved, xy);
  const int32_t closest = closest_scan_to(m, chain, xy);
  double M[9];
  for (int k = 0; k < 9; ++k) {
    const size_t at_d = 9 * static_cast<size_t>(std::max(closest, 0)) + k;
    M[k] = cov[k] + (closest >= 0 && at_d < m->gate_d.size() ? m->gate.covariance_scale * m->gate_d[at_d] : 0.0);
  }
  // Cholesky of the 3 x 3 (lower triangle), then e^T M^-1 e = |L^-1 e|^2
  double L[9] = {0};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j <= i; ++j) {
      double v = M[3 * i + j];
      for (int k = 0; k < j; ++k) {v -= L[3 * i + k] * L[3 * j + k];}
      if (i == j) {
        if (!(v > 0.0) || !std::isfinite(v)) {return true;}
        L[3 * i + i] = std::sqrt(v);
      } else {
        L[3 * i + j] = v / L[3 * j + j];
      }
    }
  }
  double y[3], d2 = 0.0;
  for (int i = 0; i < 3; ++i) {
    double v = e[i];
    for (int k = 0; k < i; ++k) {v -= L[3 * i + k] * y[k];}
    y[i] = v / L[3 * i + i];
    d2 += y[i] * y[i];
  }
  return !(d2 <= m->gate.chi2_jump);
}
}  // namespace

int try_close_loop(kh_mapper * m, int32_t scan_id, bool & closed)
{
  closed = false;
  int32_t start_id = 0;                            // rStartNum, in id space
  const int32_t n_scans = static_cast<int32_t>(m->scans.size());
  const bool gate_on = m->gate.enabled != 0;
  const bool gate_cov = gate_on && gate_needs_covariances(m->gate);
  bool gated = gate_on;                            // false once a refresh of this scan was refused: its search runs ungated
  if (gate_cov) {m->gate_age += 1;}
  while (start_id < n_scans) {
    if (m->graph_dirty) {const int rc = sync_graph(m); if (rc) {return rc;}}
    if (gate_cov && gated && (m->gate_due || m->gate_age >= m->gate.refresh_scans)) {
      const int rc = gate_refresh(m, scan_id, gated);
      if (rc) {return rc;}
      if (!gated && m->adj[scan_id].empty()) {gated = true;}        // (zero rows: the gated call is the plain one)
    }
    if (gated) {gate_prepare_rows(m);}
    // positions in the graph store's scan list (= the scans still alive, in id order)
    const int32_t query = m->compact_of[scan_id];
    int32_t start = static_cast<int32_t>(std::lower_bound(m->alive.begin(), m->alive.end(), start_id) - m->alive.begin());
    // every chain successive FindPossibleLoopClosure calls would return from `start` on, for the CURRENT poses
    std::vector<int32_t> chain_begin(2, 0), flat;
    int32_t n_chains = 0;
    int rc = enumerate_growing(m, kProfLoopEnumeration, m->max_candidates, 2, [&](int32_t * out, int32_t cap, int32_t * total) {
        if (!gated) {
          return kh_graph_find_loop_candidates_from(m->graph, 1, &query, &start, m->p.loop_search_maximum_distance,
                   m->p.loop_match_minimum_chain_size, chain_begin.data(), out, cap, total);
        }
        return kh_graph_find_loop_candidates_gated(m->graph, 1, &query, &start, m->p.loop_search_maximum_distance,
                 m->p.loop_match_minimum_chain_size, m->gate.chi2_position, m->gate_rows.data(), chain_begin.data(), out, cap, total);
      }, flat, n_chains);
    if (rc) {return rc;}
    if (n_chains == 0) {break;}
    m->stats.loop_candidates += n_chains;
    std::vector<std::vector<int32_t>> chains(static_cast<size_t>(n_chains));
    for (int32_t c = 0; c < n_chains; ++c) {chains[c] = run_of(m, flat[2 * c], flat[2 * c + 1]);}
    MScan & scan = *m->scans[scan_id];
    // coarse: m_pLoopScanMatcher->MatchScan(pScan, candidateChain, bestPose, covariance, false, false), all chains at once
    std::vector<MatchOut> coarse;
    rc = match_chains(m, m->loop_group, std::vector<kh_scan>(chains.size(), as_kh_scan(scan)), chains, false, false, coarse);
    if (rc) {return rc;}
    std::vector<int32_t> passing;
    for (int32_t c = 0; c < n_chains; ++c) {
      if (coarse[c].response > m->p.loop_match_minimum_response_coarse &&
        coarse[c].cov[0] < m->p.loop_match_maximum_variance_coarse && coarse[c].cov[4] < m->p.loop_match_maximum_variance_coarse)
      {
        passing.push_back(c);
      }
    }
    // fine: tmpScan at the coarse pose against the same chain on the sequential matcher (doPenalize false), again one batch
    std::vector<std::unique_ptr<MScan>> tmp;
    std::vector<kh_scan> fine_queries;
    std::vector<std::vector<int32_t>> fine_chains;
    for (int32_t c : passing) {
      std::unique_ptr<MScan> t(new MScan());
      t->ranges = scan.ranges;
      t->corrected = corrected_at(m->laser, to_pose(coarse[c].mean));      // tmpScan.SetSensorPose(bestPose), Mapper.cpp:1533
      update_scan(*t, m->laser);
      fine_queries.push_back(as_kh_scan(*t));
      fine_chains.push_back(chains[c]);
      tmp.push_back(std::move(t));
    }
    std::vector<MatchOut> fine;
    rc = match_chains(m, m->seq_group, fine_queries, fine_chains, false, true, fine);
    if (rc) {return rc;}
    // consume in the reference's order up to the first accepted closure
    int32_t accepted = -1;
    for (size_t i = 0; i < passing.size(); ++i) {
      if (fine[i].response < m->p.loop_match_minimum_response_fine) {continue;}
      if (gate_on && m->gate.chi2_jump > 0.0 && gate_jump_rejects(m, scan, chains[passing[i]], fine[i].mean, fine[i].cov)) {
        m->gate_stats.jump_rejected += 1;
        continue;
      }
      accepted = static_cast<int32_t>(i); break;
    }
    if (accepted < 0) {break;}                       // every chain was looked at with the poses it would have seen
    const int32_t c = passing[accepted];
    set_sensor_pose(m, scan, fine[accepted].mean);
    rc = link_chain_to_scan(m, chains[c], scan_id, fine[accepted].mean, fine[accepted].cov);
    if (rc) {return rc;}
    rc = correct_poses(m);
    if (rc) {return rc;}
    m->gate_due = true;                              // the poses have moved: the covariances of the last refresh are no longer theirs
    closed = true;
    // FindPossibleLoopClosure returned this chain at its terminating scan (rStartNum stays there): resume behind it
    start_id = m->alive[flat[2 * c + 1]] + 1;
    m->stats.speculation_discarded += n_chains - (c + 1);
  }
  return KH_OK;
}
}  // namespace mapper
}  // namespace kh

using namespace kh;

extern "C" {

void kh_loop_gate_params_default(const kh_mapper_params * params, kh_loop_gate_params * g)
{
  if (!g) {return;}
  kh_mapper_params defaults;
  if (!params) {kh_mapper_params_default(&defaults); params = &defaults;}
  g->enabled = 0; g->refresh_scans = 1;
  g->chi2_position = 5.991;                              // 95 % of chi-square with 2 degrees of freedom
  g->chi2_jump = 7.815;                                  // 95 % with 3
  g->covariance_scale = 1.0;
  // the coarse matcher cannot pull a scan further than half its window
  g->max_reach = params->loop_search_maximum_distance + params->loop_search_space_dimension / 2;
}

int kh_mapper_set_loop_gate(kh_mapper * m, const kh_loop_gate_params * g)
{
  if (!g || g->refresh_scans < 1 || !(g->chi2_position >= 0.0) || !std::isfinite(g->chi2_position) || std::isnan(g->chi2_jump) ||
    !(g->covariance_scale >= 0.0) || !std::isfinite(g->covariance_scale) || !(g->max_reach > 0.0) || !std::isfinite(g->max_reach)) {
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  m->gate = *g;
  m->gate.enabled = g->enabled ? 1 : 0;
  m->gate_d.clear(); m->gate_age = 0; m->gate_due = true;      // what an earlier setting left is not this one's
  return KH_OK;
}

int kh_mapper_get_loop_gate(const kh_mapper * m, kh_loop_gate_params * g)
{
  if (!m || !g) {return KH_ERR_INVALID_ARG;}
  *g = m->gate;
  return KH_OK;
}

int kh_mapper_get_loop_gate_stats(const kh_mapper * m, kh_loop_gate_stats * out)
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  *out = m->gate_stats;
  return KH_OK;
}

}  // extern "C"
