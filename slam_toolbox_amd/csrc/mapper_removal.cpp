// What takes scans and edges out of a mapper, or edits them one by one: Mapper::RemoveNodeFromGraph (lib/karto_sdk/src/Mapper.cpp
// :2964-3021), the marginalizing removal that keeps the pose graph connected, the lifelong node decay
// (slam_toolbox_lifelong.cpp:149-178), single-edge edits, the constraint audit and the outlier rejection.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lifelong_internal.hpp"
#include "mapper_private.hpp"
#include "spa_internal.hpp"

namespace kh
{
namespace mapper
{
// No detach_edge next to attach_edge: the loop below and kh_mapper_remove_edge do not take an edge out the same way.  RemoveNode
// looks at the NEIGHBOUR's adjacency first, skips the edge when it is missing there, finds the direction from the neighbour's
// out_edges (missing: the leaving node was the source) and leaves the leaving node's own lists to the clear() at the end;
// kh_mapper_remove_edge is given the direction, looks at out_edges first and refuses, with nothing changed, unless all three
// entries are there.  A session file is not checked for mirrored lists, so both behaviours can be reached.
int remove_node(kh_mapper * m, int32_t id, bool in_solver)
{
  ProfScope prof(m, kProfRemoveNode);
  if (!scan_alive(m, id)) {
    set_error("RemoveNode: Failed to find node matching id");
    return KH_ERR_NOT_FOUND;
  }
  // 1) the edges leave the adjacent vertices, the graph and the optimizer
  const std::vector<int32_t> neighbours = m->adj[id];
  for (int32_t a : neighbours) {
    auto pos = std::find(m->adj[a].begin(), m->adj[a].end(), id);
    if (pos == m->adj[a].end()) {continue;}                    // "Failed to find any edge in adj. vertex"
    m->adj[a].erase(pos);
    int32_t source = id, target = a;
    auto out = std::find(m->out_edges[a].begin(), m->out_edges[a].end(), id);
    if (out != m->out_edges[a].end()) {source = a; target = id; m->out_edges[a].erase(out);}
    if (m->log) {std::fprintf(m->log, "E %d %d\n", source, target);}
    const int rc = in_solver ? kh_spa_remove_constraint(m->solver, source, target) : KH_OK;
    if (rc != KH_OK && rc != KH_ERR_NOT_FOUND) {return rc;}
    --m->n_edges;
  }
  // 2) the vertex leaves the optimizer, 3) the graph and the scan map
  if (m->log) {std::fprintf(m->log, "D %d\n", id);}
  const int rc = in_solver ? kh_spa_remove_node(m->solver, id) : KH_OK;
  if (rc != KH_OK && rc != KH_ERR_NOT_FOUND) {return rc;}
  m->adj[id].clear(); m->out_edges[id].clear();
  for (int q = 0; q < m->n_slots; ++q) {
    if (m->scans[id]->d_points[q]) {m->d_free_slots[q].push_back(m->scans[id]->d_points[q]);}
  }
  if (m->scans[id]->d_ranges) {m->r_free_slots.push_back(m->scans[id]->d_ranges);}
  m->scans[id].reset();
  // a scan that leaves the graph by any way (node decay, kh_mapper_remove_node) leaves the localization buffer with it
  m->loc_buffer.erase(std::remove(m->loc_buffer.begin(), m->loc_buffer.end(), id), m->loc_buffer.end());
  m->graph_dirty = true;
  m->stats.nodes_removed += 1;
  return KH_OK;
}

int marginalize_nodes(kh_mapper * m, int32_t n, const int32_t * ids)
{
  for (int32_t k = 0; k < n; ++k) {
    if (!scan_alive(m, ids[k])) {
      set_error("MarginalizeNodes: Failed to find node matching id");
      return KH_ERR_NOT_FOUND;
    }
  }
  const int rc = kh_spa_marginalize_nodes(m->solver, n, ids, nullptr);
  // (a call that stopped at a later round has made the edits of the earlier ones: they are mirrored whatever it answered)
  for (const MargEdit & e : spa_marginalize_edits(m->solver)) {
    if (e.kind == 2) {
      const int rr = remove_node(m, e.via, false);
      if (rr) {return rr;}
      continue;
    }
    if (m->log) {
      // (a C line carries a covariance: the inverse of the information the constraint now has)
      const double o[9] = {e.omega[0], e.omega[1], e.omega[2], e.omega[1], e.omega[3], e.omega[4], e.omega[2], e.omega[4], e.omega[5]};
      const double c00 = o[4] * o[8] - o[5] * o[7], c01 = o[2] * o[7] - o[1] * o[8], c02 = o[1] * o[5] - o[2] * o[4];
      const double c11 = o[0] * o[8] - o[2] * o[6], c12 = o[2] * o[3] - o[0] * o[5], c22 = o[0] * o[4] - o[1] * o[3];
      const double r = 1.0 / (o[0] * c00 + o[1] * c01 + o[2] * c02);
      const double cov[9] = {c00 * r, c01 * r, c02 * r, c01 * r, c11 * r, c12 * r, c02 * r, c12 * r, c22 * r};
      log_constraint(m->log, e.a, e.b, e.z, cov);
    }
    if (e.kind == 0) {                       // a new edge, the hub its source; a fused constraint changes nothing here
      attach_edge(m, e.a, e.b);
      m->graph_dirty = true;
    }
  }
  return rc;
}

kh_scan_box box_of(const kh_mapper * m, const MScan & s)
{
  kh_scan_box b;
  std::memset(&b, 0, sizeof(b));
  b.barycenter[0] = s.barycenter[0]; b.barycenter[1] = s.barycenter[1];
  b.bbox_size[0] = s.bbox[2] - s.bbox[0]; b.bbox_size[1] = s.bbox[3] - s.bbox[1];     // BoundingBox2::GetSize
  b.unique_id = s.id; b.n_edges = static_cast<int32_t>(m->adj[s.id].size()); b.score = s.score;
  b.n_points = static_cast<int32_t>(s.filtered.size() / 2); b.points_xy = s.filtered.data();
  return b;
}

int lifelong_step(kh_mapper * m, int32_t id)
{
  const auto t0 = std::chrono::steady_clock::now();
  const MScan & s = *m->scans[id];
  const double w = s.bbox[2] - s.bbox[0], h = s.bbox[3] - s.bbox[1];
  const double radius = std::sqrt(w * w + h * h) / 2.0;
  if (m->graph_dirty) {const int rc = sync_graph(m); if (rc) {return rc;}}
  std::vector<int32_t> near;
  int32_t n = 0;
  int rc = enumerate_growing(m, kProfNearLinked, 64, 1, [&](int32_t * out, int32_t cap, int32_t * total) {
      return kh_graph_find_near_linked(m->graph, m->compact_of[id], radius, out, cap, total);
    }, near, n);
  if (rc) {return rc;}
  near.resize(static_cast<size_t>(n));
  for (int32_t & c : near) {c = m->alive[c];}                     // graph store positions -> scan ids
  const kh_scan_box ref = box_of(m, s);
  std::vector<kh_scan_box> cands;
  // the candidates' readings where the matcher left them in HBM (a copy a pose update made stale is refreshed first); a scan
  // without a device copy (slot allocation failed) sends the whole call down the packed form
  std::vector<const double *> resident;
  std::vector<const uint64_t *> masks;
  bool all_resident = m->laser.n <= 4096;
  {ProfScope prof(m, kProfDecayBoxes);
  for (int32_t c : near) {
    MScan & cs = *m->scans[c];
    cands.push_back(box_of(m, cs));
    // (a candidate inside the scan buffer, and vertices 0 and 1, keep their score whatever their readings say, :204-207: the mapper
    // does not read the overlap metrics, so their readings are not fetched -- the new scan itself, always a candidate, has no copy yet)
    const bool score_kept = s.id - cs.id < m->decay.scan_buffer_size || cs.id == 0 || cs.id == 1;
    const double * d = (all_resident && !score_kept) ? resident_points(m, cs, 0) : nullptr;
    if (!d && !score_kept) {all_resident = false;}
    resident.push_back(d); masks.push_back(cs.filter_mask.data());
  }
  }
  std::vector<int32_t> kept(near.size(), 0);
  std::vector<double> scores(near.size(), 0.0);
  {ProfScope prof(m, kProfDecayScores);
  rc = decay_scores(m->device, &ref, n, cands.data(), all_resident ? resident.data() : nullptr, all_resident ? masks.data() : nullptr,
      all_resident ? m->laser.n : 0, &m->decay, kept.data(), nullptr, nullptr, nullptr, scores.data());
  }
  if (rc) {return rc;}
  (all_resident ? m->stats.decay_calls_resident : m->stats.decay_calls_packed) += 1;
  std::vector<int32_t> leaving;                  // KH_REMOVE_MARGINALIZE: the step's removals as one list, in `near` order
  for (size_t k = 0; k < near.size(); ++k) {
    if (!kept[k]) {continue;}
    if (scores[k] < m->decay.removal_score) {
      if (m->removal_mode == KH_REMOVE_MARGINALIZE && !spa_marginalize_refuses(m->solver, near[k])) {leaving.push_back(near[k]); continue;}
      if (m->removal_mode == KH_REMOVE_MARGINALIZE) {m->stats.marginalize_fallbacks += 1;}
      rc = remove_node(m, near[k]);
      if (rc) {return rc;}
    } else {
      m->scans[near[k]]->score = scores[k];
    }
  }
  if (!leaving.empty()) {
    rc = marginalize_nodes(m, static_cast<int32_t>(leaving.size()), leaving.data());
    if (rc != KH_OK && rc != KH_ERR_INVALID_ARG) {return rc;}
    // (a node that grew past 64 neighbours through the ones before it stopped the call: it and the rest leave plainly)
    for (int32_t id : leaving) {
      if (!m->scans[id]) {continue;}
      m->stats.marginalize_fallbacks += 1;
      rc = remove_node(m, id);
      if (rc) {return rc;}
    }
  }
  m->stats.lifelong_ms += ms_since(t0);
  return KH_OK;
}
}  // namespace mapper
}  // namespace kh

using namespace kh;
using namespace kh::mapper;

extern "C" {

int kh_mapper_set_lifelong(kh_mapper * m, const kh_decay_params * params)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  m->lifelong = params != nullptr;
  if (params) {m->decay = *params; m->decay.scan_buffer_size = m->p.scan_buffer_size;}
  return KH_OK;
}

int kh_mapper_remove_node(kh_mapper * m, int32_t scan_id)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  // The next Process() reads the last scan and every scan of the running window; the reference (GetLastScan /
  // GetRunningScans hold raw pointers, Mapper.cpp:2688, 2716) would be left with dangling ones, and its only caller --
  // the lifelong policy, which skips the newest scan_buffer_size scans -- never asks for this.  Refused here.
  if (scan_id == m->last || std::find(m->running.begin(), m->running.end(), scan_id) != m->running.end()) {
    set_error("RemoveNode: the scan is the last scan or in the running-scan window");
    return KH_ERR_INVALID_ARG;
  }
  return remove_node(m, scan_id);
}

int kh_mapper_marginalize_nodes(kh_mapper * m, int32_t n, const int32_t * scan_ids)
{
  if (n < 0 || (n > 0 && !scan_ids)) {return KH_ERR_INVALID_ARG;}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  for (int32_t k = 0; k < n; ++k) {                     // as kh_mapper_remove_node: the next Process() reads these scans
    if (scan_ids[k] == m->last || std::find(m->running.begin(), m->running.end(), scan_ids[k]) != m->running.end()) {
      set_error("MarginalizeNodes: a scan is the last scan or in the running-scan window");
      return KH_ERR_INVALID_ARG;
    }
  }
  return marginalize_nodes(m, n, scan_ids);
}

int kh_mapper_set_removal_mode(kh_mapper * m, int32_t mode)
{
  if (!m || (mode != KH_REMOVE_PLAIN && mode != KH_REMOVE_MARGINALIZE)) {return KH_ERR_INVALID_ARG;}
  m->removal_mode = mode;
  return KH_OK;
}

// ---- single-edge edits, the constraint audit and the rejection loop ----
int kh_mapper_correct_poses(kh_mapper * m)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  const int rc = correct_poses(m);
  m->gate_due = true;                                // the poses may have moved: the gate's covariances are no longer theirs
  return rc;
}

int kh_mapper_add_edge(kh_mapper * m, int32_t from, int32_t to, const double mean_sensor_pose[3], const double cov[9], int32_t correct)
{
  if (!mean_sensor_pose || !cov) {return KH_ERR_INVALID_ARG;}
  for (int k = 0; k < 3; ++k) {if (!std::isfinite(mean_sensor_pose[k])) {return KH_ERR_INVALID_ARG;}}
  for (int k = 0; k < 9; ++k) {if (!std::isfinite(cov[k])) {return KH_ERR_INVALID_ARG;}}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (!scan_alive(m, from) || !scan_alive(m, to) || from == to) {
    set_error("AddEdge: Failed to find the two scans");
    return KH_ERR_NOT_FOUND;
  }
  int rc = link_scans(m, from, to, mean_sensor_pose, cov);
  if (rc) {return rc;}
  m->gate_due = true;
  return correct ? kh_mapper_correct_poses(m) : KH_OK;
}

int kh_mapper_remove_edge(kh_mapper * m, int32_t from, int32_t to)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (!scan_alive(m, from) || !scan_alive(m, to)) {set_error("RemoveEdge: Failed to find the two scans"); return KH_ERR_NOT_FOUND;}
  const auto out = std::find(m->out_edges[from].begin(), m->out_edges[from].end(), to);
  const auto af = std::find(m->adj[from].begin(), m->adj[from].end(), to);
  const auto at = std::find(m->adj[to].begin(), m->adj[to].end(), from);
  if (out == m->out_edges[from].end() || af == m->adj[from].end() || at == m->adj[to].end()) {
    set_error("RemoveEdge: no edge with that source and target");
    return KH_ERR_NOT_FOUND;
  }
  m->out_edges[from].erase(out); m->adj[from].erase(af); m->adj[to].erase(at);
  --m->n_edges;
  m->graph_dirty = true;
  m->gate_due = true;
  if (m->log) {std::fprintf(m->log, "E %d %d\n", from, to);}
  const int rc = kh_spa_remove_constraint(m->solver, from, to);
  return (rc == KH_OK || rc == KH_ERR_NOT_FOUND) ? KH_OK : rc;
}

int kh_mapper_audit(kh_mapper * m, double min_redundancy, kh_spa_audit_t * out, int32_t cap, int32_t * n, kh_spa_audit_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (n) {*n = 0;}
  if (!std::isfinite(min_redundancy) || !(min_redundancy > 0.0) || !(min_redundancy < 1.0) || !out || !n || cap < 0) {return KH_ERR_INVALID_ARG;}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  const int32_t nc = kh_spa_num_constraints(m->solver);
  *n = nc;
  if (nc > cap) {set_error("kh_mapper_audit: the capacity is below the number of constraints"); return KH_ERR_INVALID_ARG;}
  return kh_spa_audit_constraints(m->solver, min_redundancy, out, summary);
}

void kh_reject_params_default(kh_reject_params * p)
{
  if (!p) {return;}
  p->chi2 = 16.266;                                  // 99.9 % of chi-square with 3 degrees of freedom
  p->min_redundancy = 1e-6; p->tie = 1e-6;
  p->min_id_gap = 2; p->max_rounds = 8;
}

int kh_mapper_reject_outliers(kh_mapper * m, const kh_reject_params * params, kh_spa_audit_t * removed, int32_t cap, kh_reject_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  kh_reject_params p;
  kh_reject_params_default(&p);
  if (params) {p = *params;}
  if (!std::isfinite(p.chi2) || !std::isfinite(p.min_redundancy) || !std::isfinite(p.tie) || !(p.chi2 >= 0.0) || !(p.min_redundancy > 0.0) ||
    !(p.min_redundancy < 1.0) || !(p.tie >= 0.0) || !(p.tie < 1.0) || p.min_id_gap < 1 || p.max_rounds < 1 || cap < 0 || (cap > 0 && !removed)) {
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  const auto t_begin = std::chrono::steady_clock::now();
  kh_reject_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  auto finish = [&](int rc) {sum.total_ms = ms_since(t_begin); if (summary) {*summary = sum;} return rc;};
  std::vector<kh_spa_audit_t> rec;
  bool solved = true;                                // whether correct_poses has run since the last removal
  for (int32_t round = 0; round < p.max_rounds; ++round) {
    ++sum.rounds;
    auto t0 = std::chrono::steady_clock::now();
    int rc = kh_mapper_correct_poses(m);
    sum.solve_ms += ms_since(t0);
    if (rc) {return finish(rc);}
    solved = true;
    rec.resize(static_cast<size_t>(std::max(1, kh_spa_num_constraints(m->solver))));
    kh_spa_audit_summary as;
    t0 = std::chrono::steady_clock::now();
    rc = kh_spa_audit_constraints(m->solver, p.min_redundancy, rec.data(), &as);
    sum.audit_ms += ms_since(t0);
    if (rc) {return finish(rc);}
    // the candidates: verifiable (never a bridge, never the only constraint that pins a direction) and not odometry
    double top = -1.0;
    for (int32_t e = 0; e < as.n_constraints; ++e) {
      const int64_t gap = std::llabs(static_cast<int64_t>(rec[e].id_a) - rec[e].id_b);
      if (rec[e].verifiable && gap >= p.min_id_gap && rec[e].chi2_loo > top) {top = rec[e].chi2_loo;}
    }
    sum.max_chi2_loo = top < 0.0 ? 0.0 : top;
    if (!(top > p.chi2)) {break;}
    // near-ties go to the newest constraint: the graph was consistent without the one added last
    int32_t pick = -1;
    for (int32_t e = 0; e < as.n_constraints; ++e) {
      const int64_t gap = std::llabs(static_cast<int64_t>(rec[e].id_a) - rec[e].id_b);
      if (rec[e].verifiable && gap >= p.min_id_gap && rec[e].chi2_loo >= (1.0 - p.tie) * top) {pick = e;}
    }
    if (sum.n_removed >= cap) {
      set_error("kh_mapper_reject_outliers: more removals than `removed` holds");
      return finish(KH_ERR_INVALID_ARG);
    }
    rc = kh_mapper_remove_edge(m, rec[pick].id_a, rec[pick].id_b);
    if (rc) {return finish(rc);}
    removed[sum.n_removed++] = rec[pick];
    solved = false;
  }
  if (!solved) {
    // the rounds ran out behind a removal: max_chi2_loo is the figure of the audit BEFORE it
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = kh_mapper_correct_poses(m);
    sum.solve_ms += ms_since(t0);
    if (rc) {return finish(rc);}
  }
  return finish(KH_OK);
}

}  // extern "C"
