// ROS-free mapper front end over the GPU hot path: what karto::Mapper::Process does around the scan matcher and the
// solver plugin, so that a scan queue can be replayed end to end (BASELINE configs 1 and 5) without the reference's
// object model.  Everything numeric goes through the library's own entry points -- kh_matcher_* (sequential and loop
// matcher), kh_spa_* (solver plugin), kh_graph_* (candidate enumeration) -- and the mapper's files keep the control flow and the
// small exact host arithmetic (poses, transforms, running-scan buffer, link bookkeeping) in the reference's operation
// order so that the run is comparable call by call with karto::Mapper driving the same queue.
//
// This file: create / destroy / log, the graph bookkeeping, Process with its four entries, the small getters and setters.  The
// loop search is in mapper_loop.cpp, removal and node decay in mapper_removal.cpp, sessions in mapper_session.cpp, relocalization
// in mapper_relocalize.cpp, the views of the merger and the live map in mapper_views.cpp, the pose arithmetic in mapper_pose.hpp.
//
// Reference: lib/karto_sdk/src/Mapper.cpp  Process :2679-2748, ProcessLocalization :2831-2909 with AddScanToLocalizationBuffer /
// ClearLocalizationBuffer :2911-2962, ProcessAgainstNodesNearBy :2751-2829, ProcessAgainstNode / ProcessAtDock :3023-3102, HasMovedEnough :3110-3142, ScanManager::AddRunningScan
// :183-206, MapperGraph::AddVertex :1418-1432, AddEdges :1434-1498, LinkScans :1620-1639,
// LinkNearChains :1641-1663, LinkChainToScan :1665-1681, CorrectPoses :2012-2030.
//
// The four entry points share one body (process_scan): they differ in where the last scan comes from, in the HasMovedEnough gate
// and in what happens to the accepted scan at the very end (the localization buffer).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "graph_internal.hpp"
#include "mapper_private.hpp"
#include "query_hook.hpp"
#include "spa_internal.hpp"

namespace kh
{
namespace mapper
{
double * take_slot(std::vector<double *> & slabs, std::vector<double *> & free_slots, int32_t device, size_t doubles_per_slot)
{
  if (free_slots.empty()) {
    constexpr int kSlabScans = 256;
    void * p = nullptr;
    if (kh_device_malloc(device, static_cast<int64_t>(sizeof(double) * doubles_per_slot) * kSlabScans, &p) == KH_OK) {
      slabs.push_back(static_cast<double *>(p));
      for (int k = kSlabScans - 1; k >= 0; --k) {free_slots.push_back(static_cast<double *>(p) + static_cast<size_t>(k) * doubles_per_slot);}
    }
  }
  if (free_slots.empty()) {return nullptr;}
  double * slot = free_slots.back();
  free_slots.pop_back();
  return slot;
}

const double * resident_points(kh_mapper * m, MScan & s, int slot, void * on_stream)
{
  const int64_t bytes = static_cast<int64_t>(sizeof(double)) * static_cast<int64_t>(s.points.size());
  if (bytes <= 0 || s.points.size() != 2 * static_cast<size_t>(m->laser.n)) {return nullptr;}
  if (!s.d_points[slot]) {
    s.d_points[slot] = take_slot(m->d_slabs[slot], m->d_free_slots[slot], m->slot_device[slot], s.points.size());
    if (s.d_points[slot]) {s.d_fresh &= static_cast<uint16_t>(~(1u << slot));}
  }
  if (s.d_points[slot] && !(s.d_fresh & (1u << slot)) &&
    (on_stream ? kh_device_upload_on(s.d_points[slot], s.points.data(), bytes, on_stream) : kh_device_upload(s.d_points[slot], s.points.data(), bytes)) == KH_OK) {
    s.d_fresh |= static_cast<uint16_t>(1u << slot);
  }
  return (s.d_points[slot] && (s.d_fresh & (1u << slot))) ? s.d_points[slot] : nullptr;
}

// the reference bounds its candidate walks by the scan map's SIZE, in id space (Mapper.cpp:1974-1976, 1751-1756): the store
// visits the scans of `alive` whose id is below the number of scans alive
static int set_scan_limit(kh_mapper * m)
{
  const int32_t n_alive = static_cast<int32_t>(m->alive.size());
  const int32_t n_visit = static_cast<int32_t>(std::lower_bound(m->alive.begin(), m->alive.end(), n_alive) - m->alive.begin());
  return kh_graph_set_scan_limit(m->graph, n_visit);
}

int sync_graph(kh_mapper * m)
{
  ProfScope prof(m, kProfSyncGraph);
  m->alive.clear();
  m->compact_of.assign(m->scans.size(), -1);
  for (size_t i = 0; i < m->scans.size(); ++i) {
    if (m->scans[i]) {m->compact_of[i] = static_cast<int32_t>(m->alive.size()); m->alive.push_back(static_cast<int32_t>(i));}
  }
  const size_t n = m->alive.size();
  // (scratch kept by the mapper and swapped with the store's arrays: no allocation, no copy -- see kh::graph_swap)
  std::vector<double> & xy = m->sync_xy, & pose = m->sync_pose;
  std::vector<int32_t> & ptr = m->sync_ptr, & idx = m->sync_idx;
  xy.resize(2 * n); pose.resize(2 * n); ptr.resize(n + 1); idx.clear();
  ptr[0] = 0;
  for (size_t c = 0; c < n; ++c) {
    reference_xy(m, *m->scans[m->alive[c]], &xy[2 * c]);
    pose[2 * c] = m->scans[m->alive[c]]->corrected.x; pose[2 * c + 1] = m->scans[m->alive[c]]->corrected.y;
    ptr[c + 1] = ptr[c] + static_cast<int32_t>(m->adj[m->alive[c]].size());
  }
  idx.reserve(static_cast<size_t>(ptr[n]));
  for (size_t c = 0; c < n; ++c) {
    for (int32_t w : m->adj[m->alive[c]]) {idx.push_back(m->compact_of[w]);}
  }
  int rc = graph_swap(m->graph, static_cast<int32_t>(n), xy, ptr, idx, pose);
  if (rc) {return rc;}
  rc = set_scan_limit(m);
  if (rc == KH_OK) {m->graph_dirty = false;}
  return rc;
}

void set_sensor_pose(kh_mapper * m, MScan & s, const double pose[3])
{
  s.corrected = corrected_at(m->laser, to_pose(pose));
  update_scan(s, m->laser);
  if (s.id < 0) {return;}               // not in the graph yet (the match of a new scan): AddScan appends it where it stands
  if (!m->graph_dirty && s.id < static_cast<int32_t>(m->compact_of.size()) && m->compact_of[s.id] >= 0) {
    double xy[2];
    reference_xy(m, s, xy);
    const double pose_xy[2] = {s.corrected.x, s.corrected.y};
    if (kh_graph_set_position(m->graph, m->compact_of[s.id], xy) != KH_OK || kh_graph_set_pose(m->graph, m->compact_of[s.id], pose_xy) != KH_OK) {
      m->graph_dirty = true;
    }
  } else {
    m->graph_dirty = true;
  }
}

void attach_edge(kh_mapper * m, int32_t from, int32_t to)
{
  m->out_edges[from].push_back(to);
  m->adj[from].push_back(to);
  m->adj[to].push_back(from);
  ++m->n_edges;
}

void log_constraint(FILE * log, int32_t from, int32_t to, const double diff[3], const double cov[9])
{
  std::fprintf(log, "C %d %d %.17g %.17g %.17g", from, to, diff[0], diff[1], diff[2]);
  for (int k = 0; k < 9; ++k) {std::fprintf(log, " %.17g", cov[k]);}
  std::fprintf(log, "\n");
}

int link_scans(kh_mapper * m, int32_t from, int32_t to, const double mean[3], const double cov[9])
{
  for (int32_t t : m->out_edges[from]) {if (t == to) {return KH_OK;}}     // not a new edge: nothing is attached
  attach_edge(m, from, to);
  // the store follows edit by edit while nothing was removed or re-posed since it was built (sync_graph rebuilds otherwise)
  if (!m->graph_dirty && kh_graph_add_edge(m->graph, m->compact_of[from], m->compact_of[to]) != KH_OK) {m->graph_dirty = true;}
  // LinkInfo(pFromScan->GetCorrectedPose(), pToScan->GetCorrectedAt(rMean), rCovariance)
  double pose1[3], pose2[3];
  put_pose(m->scans[from]->corrected, pose1);
  put_pose(corrected_at(m->laser, to_pose(mean)), pose2);
  double diff[3], cov_out[9];
  int rc = kh_link_info(pose1, pose2, cov, diff, cov_out);
  if (rc) {return rc;}
  if (m->log) {log_constraint(m->log, from, to, diff, cov_out);}
  rc = kh_spa_add_constraint(m->solver, from, to, diff, cov_out);
  // the plugin logs and carries on when it cannot add a constraint (ceres_solver.cpp:354-361)
  return (rc == KH_OK || rc == KH_ERR_NOT_FOUND || rc == KH_ERR_INVALID_ARG) ? KH_OK : rc;
}

int32_t closest_scan_to(const kh_mapper * m, const std::vector<int32_t> & chain, const double pose[2])
{
  int32_t closest = -1;
  double best = 1.7976931348623157e308;
  for (int32_t c : chain) {
    double xy[2];
    reference_xy(m, *m->scans[c], xy);
    const double dx = pose[0] - xy[0], dy = pose[1] - xy[1];
    const double d = dx * dx + dy * dy;
    if (d < best) {best = d; closest = c;}
  }
  return closest;
}

int link_chain_to_scan(kh_mapper * m, const std::vector<int32_t> & chain, int32_t scan, const double mean[3], const double cov[9])
{
  double pose[2];
  reference_xy(m, *m->scans[scan], pose);
  const int32_t closest = closest_scan_to(m, chain, pose);
  if (closest < 0) {return KH_OK;}
  double cxy[2];
  reference_xy(m, *m->scans[closest], cxy);
  const double dx = pose[0] - cxy[0], dy = pose[1] - cxy[1];
  const double squaredDistance = dx * dx + dy * dy;
  if (squaredDistance < m->p.link_scan_maximum_distance * m->p.link_scan_maximum_distance + kTolerance) {
    return link_scans(m, closest, scan, mean, cov);
  }
  return KH_OK;
}

// thousands of scans x 1081 sincos: wider than the matcher's worker pool (32 threads suit its sub-millisecond bursts;
// this is milliseconds of uniform work, so from 2048 scans it goes to the wide pool in chunks of 32 scans); below, one scan is
// one item of the ordinary pool
void update_scans_bulk(size_t n, const std::function<void(size_t)> & body)
{
  if (n >= 2048) {
    const size_t chunks = (n + 31) / 32;
    host_parallel_for_wide(chunks, [&](size_t c) {
      for (size_t k = 32 * c; k < std::min(n, 32 * c + 32); ++k) {body(k);}
    });
  } else {
    host_parallel_for(n, body);
  }
}

int correct_poses(kh_mapper * m)
{
  const auto t0 = std::chrono::steady_clock::now();
  kh_spa_summary sum;
  const int rc = kh_spa_compute(m->solver, &sum);
  const double ms = ms_since(t0);
  m->stats.solver_ms += ms; m->stats.loop_closures += 1;
  if (rc != KH_OK && rc != KH_ERR_SOLVER && rc != KH_ERR_NOT_FOUND) {return rc;}
  int32_t n = 0;
  kh_spa_get_corrections(m->solver, &n, nullptr, nullptr);
  std::vector<int32_t> ids(static_cast<size_t>(n));
  std::vector<double> poses(3 * static_cast<size_t>(n));
  if (n) {kh_spa_get_corrections(m->solver, &n, ids.data(), poses.data());}
  if (m->log) {
    std::fprintf(m->log, "X %d %.6f\n", n, ms);
    for (int32_t k = 0; k < n; ++k) {std::fprintf(m->log, "P %d %.17g %.17g %.17g\n", ids[k], poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]);}
  }
  // SetCorrectedPoseAndUpdate of every scan: N x P cos / sin in libm (the reference does the same, serially)
  const auto t1 = std::chrono::steady_clock::now();
  update_scans_bulk(static_cast<size_t>(n), [&](size_t k) {
    if (!scan_alive(m, ids[k])) {return;}
    MScan & s = *m->scans[ids[k]];
    // (a pose the solve left bit for bit where it was -- a component the closure did not touch and whose own residuals are at
    // rest -- re-projects to the same readings: nothing to do, and the device copy stays valid)
    if (std::memcmp(&s.corrected.x, &poses[3 * k], sizeof(double)) == 0 && std::memcmp(&s.corrected.y, &poses[3 * k + 1], sizeof(double)) == 0 &&
      std::memcmp(&s.corrected.h, &poses[3 * k + 2], sizeof(double)) == 0) {return;}
    s.corrected = to_pose(&poses[3 * k]);
    update_scan(s, m->laser);
  });
  m->stats.update_ms += ms_since(t1);
  m->graph_dirty = true;
  if (m->log) {std::fprintf(m->log, "K\n");}
  return kh_spa_clear(m->solver);
}

int match_chains(kh_mapper * m, kh_matcher_group * group, const std::vector<kh_scan> & queries, const std::vector<std::vector<int32_t>> & chains,
  bool penalize, bool refine, std::vector<MatchOut> & out)
{
  const size_t n = chains.size();
  out.assign(n, MatchOut());
  if (n == 0) {return KH_OK;}
  const int32_t nm = kh_matcher_group_size(group);
  std::vector<kh_scan> base;
  std::vector<int32_t> begin(n + 1, 0);
  std::vector<const double *> table;
  for (size_t i = 0; i < n; ++i) {
    const int32_t member = static_cast<int32_t>(i % static_cast<size_t>(nm));
    for (int32_t c : chains[i]) {
      MScan & s = *m->scans[c];
      base.push_back(as_kh_scan(s));
      const size_t row = table.size();
      table.resize(row + static_cast<size_t>(nm), nullptr);
      table[row + member] = resident_points(m, s, m->member_slot[member]);       // only the member that will read it
    }
    begin[i + 1] = static_cast<int32_t>(base.size());
  }
  std::vector<double> means(3 * n), covs(9 * n), resp(n);
  std::vector<int32_t> status(n, 0);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = kh_matcher_group_match_batch(group, static_cast<int32_t>(n), queries.data(), base.data(), begin.data(), table.data(),
      penalize ? 1 : 0, refine ? 1 : 0, means.data(), covs.data(), resp.data(), status.data());
  m->stats.match_ms += ms_since(t0);
  m->stats.matches += static_cast<int64_t>(n);
  if (rc) {return rc;}
  for (size_t i = 0; i < n; ++i) {
    if (status[i] != KH_OK) {return status[i];}             // the reference throws (Mapper.cpp:786-796, 828)
    out[i].response = resp[i];
    std::copy(means.begin() + 3 * i, means.begin() + 3 * i + 3, out[i].mean);
    std::copy(covs.begin() + 9 * i, covs.begin() + 9 * i + 9, out[i].cov);
  }
  return KH_OK;
}

std::vector<int32_t> run_of(const kh_mapper * m, int32_t first, int32_t last)
{
  std::vector<int32_t> v;
  for (int32_t i = first; i <= last; ++i) {v.push_back(m->alive[i]);}
  return v;
}

namespace
{
// Mapper::AddScanToLocalizationBuffer's eviction (Mapper.cpp:2919-2936) and the loop body of ClearLocalizationBuffer (:2941-2953):
// the front of the buffer leaves the graph, the solver and the scan map
int evict_front(kh_mapper * m)
{
  const int32_t old = m->loc_buffer.front();
  // In a run of ProcessLocalization calls the evicted scan is scan_buffer_size accepted scans behind the newest one and the same
  // parameter bounds the running window (AddRunningScan :183-206), so it has left the window; the reference relies on that (its
  // window holds raw pointers).  A window re-seeded by ProcessAgainstNode(sNearBy) with a BUFFERED scan breaks the assumption:
  // the reference would then match against a deleted scan.  Here the scan leaves the window with the graph.
  m->running.erase(std::remove(m->running.begin(), m->running.end(), old), m->running.end());
  if (m->last == old) {m->last = -1;}
  return remove_node(m, old);                          // (takes `old` out of loc_buffer)
}

// HasMovedEnough (:3110-3142)
bool has_moved_enough(const kh_mapper * m, const MScan & scan, const MScan & last)
{
  if (scan.time - last.time >= m->p.minimum_time_interval) {return true;}
  // the scanner's pose for the two odometric poses (GetSensorAt, :3123-3124)
  const Pose last_scanner = sensor_at(m->laser, last.odometric), scanner = sensor_at(m->laser, scan.odometric);
  const double deltaHeading = normalize_angle(scanner.h - last_scanner.h);
  if (std::fabs(deltaHeading) >= m->p.minimum_travel_heading) {return true;}
  const double dx = last_scanner.x - scanner.x, dy = last_scanner.y - scanner.y;
  return dx * dx + dy * dy >= m->p.minimum_travel_distance * m->p.minimum_travel_distance - kTolerance;
}

// the scan as a BASE scan of a match on the mapper's own device: its readings resident there
kh_scan as_base_scan(kh_mapper * m, MScan & s, void * on_stream)
{
  kh_scan k = as_kh_scan(s);
  k.device_points_xy = resident_points(m, s, 0, on_stream);
  return k;
}

// The sequential match: the new scan against the running scans (:2713-2724).  The scan's readings are made on the way (update_scan).
int match_sequential(kh_mapper * m, MScan * sp, double mean[3], double cov[9])
{
  // LocalizedRangeScan::Update of the new scan (1081 sincos) is handed to the matcher as a QueryHook: the match's rasteriser needs
  // the query's sensor pose and nothing else of it, so the readings are computed behind its launches, while the GPU works; the
  // matcher runs the hook before anything reads the readings, whatever path the call takes, and before it returns
  sp->sensor = sensor_at(m->laser, sp->corrected);
  sp->points.assign(2 * static_cast<size_t>(m->laser.n), 0.0);
  const kh_scan q = as_kh_scan(*sp);
  set_pending_query_hook([m, sp]() {ProfScope prof(m, kProfUpdateScanNew); update_scan(*sp, m->laser);});
  std::vector<kh_scan> base;
  // (uploads of scans not yet resident go in front of the match on the matcher's own stream; the match returns after its
  // last kernel, so every other reader finds them in place)
  void * seq_stream = kh_matcher_stream(m->seq);
  for (int32_t r : m->running) {base.push_back(as_base_scan(m, *m->scans[r], seq_stream));}
  double response = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = kh_matcher_match(m->seq, &q, base.data(), static_cast<int32_t>(base.size()), 1, 1, mean, cov, &response);
  run_pending_query_hook();             // (an argument check that refused the call before the hook was taken)
  m->stats.match_ms += ms_since(t0);
  m->stats.matches += 1;
  if (rc) {return rc;}
  // KH_MAPPER_DUMP_MATCH=<scan id>:<path> (debugging aid): the inputs and the result of this sequential match as raw doubles
  // (n_base, n_beams, query pose, query ranges, per base scan: pose, ranges; mean, covariance, response)
  static const char * dump_spec = std::getenv("KH_MAPPER_DUMP_MATCH");
  if (dump_spec && std::atoi(dump_spec) == static_cast<int>(m->scans.size()) && std::strchr(dump_spec, ':')) {
    if (FILE * f = std::fopen(std::strchr(dump_spec, ':') + 1, "wb")) {
      const double hdr[2] = {static_cast<double>(base.size()), static_cast<double>(q.n)};
      std::fwrite(hdr, 8, 2, f);
      std::fwrite(q.sensor_pose, 8, 3, f); std::fwrite(q.ranges, 8, static_cast<size_t>(q.n), f);
      for (const kh_scan & b : base) {std::fwrite(b.sensor_pose, 8, 3, f); std::fwrite(b.ranges, 8, static_cast<size_t>(b.n), f);}
      std::fwrite(mean, 8, 3, f); std::fwrite(cov, 8, 9, f); std::fwrite(&response, 8, 1, f);
      std::fclose(f);
    }
  }
  return KH_OK;
}

// AddScan: state id = unique id = position in the list (:2727); the graph store follows while it is in step
int32_t append_scan(kh_mapper * m, std::unique_ptr<MScan> scan)
{
  const int32_t id = static_cast<int32_t>(m->scans.size());
  scan->id = id;
  m->scans.push_back(std::move(scan));
  m->adj.emplace_back(); m->out_edges.emplace_back();
  if (!m->graph_dirty) {
    double xy[2];
    reference_xy(m, *m->scans[id], xy);
    m->compact_of.push_back(static_cast<int32_t>(m->alive.size()));
    m->alive.push_back(id);
    const double pose_xy[2] = {m->scans[id]->corrected.x, m->scans[id]->corrected.y};
    if (kh_graph_append_scan_with_pose(m->graph, xy, pose_xy) != KH_OK) {m->graph_dirty = true;}
    // the scan map's size in id space bounds the candidate walks (see set_scan_limit)
    if (!m->graph_dirty && set_scan_limit(m) != KH_OK) {m->graph_dirty = true;}
  }
  return id;
}

// LinkNearChains (:1641-1663): the near chains are independent matches of the same scan -> one batch
int link_near_chains(kh_mapper * m, int32_t id, std::vector<double> & means, std::vector<double> & covs)
{
  MScan & s = *m->scans[id];
  if (m->graph_dirty) {const int rc = sync_graph(m); if (rc) {return rc;}}
  std::vector<int32_t> flat;
  int32_t n_chains = 0;
  const int32_t query = m->compact_of[id];
  int rc = enumerate_growing(m, kProfLinkNearChains, m->max_candidates, 2, [&](int32_t * out, int32_t cap, int32_t * total) {
      return kh_graph_find_near_chains(m->graph, query, m->p.link_scan_maximum_distance, out, cap, total);
    }, flat, n_chains);
  if (rc) {return rc;}
  std::vector<std::vector<int32_t>> chains;
  for (int32_t c = 0; c < n_chains; ++c) {
    if (flat[2 * c + 1] - flat[2 * c] + 1 < m->p.loop_match_minimum_chain_size) {continue;}
    chains.push_back(run_of(m, flat[2 * c], flat[2 * c + 1]));
  }
  std::vector<MatchOut> res;
  rc = match_chains(m, m->seq_group, std::vector<kh_scan>(chains.size(), as_kh_scan(s)), chains, false, true, res);
  if (rc) {return rc;}
  for (size_t c = 0; c < chains.size(); ++c) {
    if (res[c].response > m->p.link_match_minimum_response_fine - kTolerance) {
      means.insert(means.end(), res[c].mean, res[c].mean + 3);
      covs.insert(covs.end(), res[c].cov, res[c].cov + 9);
      rc = link_chain_to_scan(m, chains[c], id, res[c].mean, res[c].cov); if (rc) {return rc;}
    }
  }
  return KH_OK;
}

// AddEdges (:1434-1498); has_last: there is a previous scan to link to (it is scan id - 1, and still in the map)
int add_edges(kh_mapper * m, int32_t id, bool has_last, const double cov[9])
{
  MScan & s = *m->scans[id];
  std::vector<double> means, covs;
  int rc;
  if (has_last) {
    double scan_pose[3];
    put_pose(s.sensor_pose(), scan_pose);
    rc = link_scans(m, id - 1, id, scan_pose, cov); if (rc) {return rc;}
    means.insert(means.end(), scan_pose, scan_pose + 3);
    covs.insert(covs.end(), cov, cov + 9);
    rc = link_chain_to_scan(m, m->running, id, scan_pose, cov); if (rc) {return rc;}
  }
  rc = link_near_chains(m, id, means, covs);
  if (rc) {return rc;}
  if (!means.empty()) {
    double wm[3];
    rc = kh_weighted_mean(static_cast<int32_t>(means.size() / 3), means.data(), covs.data(), wm); if (rc) {return rc;}
    set_sensor_pose(m, s, wm);
  }
  return KH_OK;
}

// AddRunningScan (:183-206)
void add_running_scan(kh_mapper * m, int32_t id)
{
  m->running.push_back(id);
  auto sq = [&]() {
    const Pose f = m->scans[m->running.front()]->sensor_pose(), b = m->scans[m->running.back()]->sensor_pose();
    const double dx = f.x - b.x, dy = f.y - b.y;
    return dx * dx + dy * dy;
  };
  double squaredDistance = sq();
  while (m->running.size() > static_cast<size_t>(m->p.scan_buffer_size) ||
    squaredDistance > m->p.scan_buffer_maximum_scan_distance * m->p.scan_buffer_maximum_scan_distance - kTolerance)
  {
    m->running.erase(m->running.begin());
    squaredDistance = sq();
  }
}

enum class Entry {kProcess, kLocalization, kAgainstNode, kNearBy};

// The body Mapper::Process (Mapper.cpp:2679-2748), ProcessLocalization (:2831-2909), ProcessAgainstNode (:3023-3096) and
// ProcessAgainstNodesNearBy (:2751-2829) share
int process_scan(kh_mapper * m, Entry entry, int32_t node_id, bool to_buffer, const double * ranges, const double odometric_pose[3], double time,
  int32_t * accepted, double corrected_pose[3], double covariance[9])
{
  if (!m || !ranges || !odometric_pose || !accepted) {return KH_ERR_INVALID_ARG;}
  *accepted = 0;
  if (m->failed) {
    set_error("kh_mapper_process: an earlier call failed after its scan had entered the graph; the handle is unusable");
    return KH_ERR_SOLVER;
  }
  if (to_buffer && m->p.scan_buffer_size < 1) {
    set_error("localization mode needs scan_buffer_size >= 1 (the accepted scan would evict itself)");
    return KH_ERR_INVALID_ARG;
  }
  const bool gated = entry == Entry::kProcess || entry == Entry::kLocalization;
  if (entry == Entry::kAgainstNode && !scan_alive(m, node_id)) {
    set_error("ProcessAgainstNode: no such node (unknown or removed)");         // the reference dereferences NULL (:3043-3046)
    return KH_ERR_NOT_FOUND;
  }
  if (entry == Entry::kNearBy) {
    // FindNearByScan(sensor name, pScan->GetOdometricPose()) over the vertices still in the graph (:2768-2769)
    if (m->graph_dirty) {const int rc = sync_graph(m); if (rc) {return rc;}}
    int32_t nearest = -1;
    const int rc = kh_graph_find_near_by_scan(m->graph, 1, odometric_pose, &nearest, nullptr);
    if (rc) {return rc;}
    node_id = nearest >= 0 ? m->alive[nearest] : -1;
  }
  if (!gated && node_id >= 0) {
    // ClearRunningScans, AddRunningScan(pLastScan), SetLastScan(pLastScan) (:2774-2776, 3046-3048)
    m->running.assign(1, node_id);
    m->last = node_id;
  }
  const auto t_begin = std::chrono::steady_clock::now();
  std::unique_ptr<MScan> scan(new MScan());
  scan->ranges.assign(ranges, ranges + m->laser.n);
  scan->time = time;
  scan->odometric = to_pose(odometric_pose);
  scan->corrected = scan->odometric;                      // the caller's SetCorrectedPose(odometric pose)
  MScan * last = m->last >= 0 ? m->scans[m->last].get() : nullptr;
  // update the scan's corrected pose based on the last correction (:2699-2703); not on the near-pose entries, whose caller has put
  // the scan where the match should start
  if (last && gated) {scan->corrected = transform_pose(last->odometric, last->corrected, scan->odometric);}
  if (last && gated && !has_moved_enough(m, *scan, *last)) {return KH_OK;}
  double cov[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (!(m->p.use_scan_matching && last)) {ProfScope prof(m, kProfUpdateScanNew); update_scan(*scan, m->laser);}
  // correct the scan against the running scans (:2713-2724)
  if (m->p.use_scan_matching && last) {
    double mean[3];
    const int rc = match_sequential(m, scan.get(), mean, cov);
    if (rc) {
      // an early return of the match (invalid argument, empty query, a HIP error) may leave the uploads it queued in flight:
      // wait for them, so that no other stream reads a copy marked fresh while it is still arriving
      stream_synchronize(kh_matcher_stream(m->seq));
      return rc;
    }
    set_sensor_pose(m, *scan, mean);
  }
  // pScan->SetOdometricPose(pScan->GetCorrectedPose()) (:2792, 3065): the next scan's odometry delta is measured from here
  if (!gated) {scan->odometric = scan->corrected;}
  const int32_t id = append_scan(m, std::move(scan));
  // from here on the scan is part of the mapper: an error return leaves the handle marked failed
  struct CommitGuard {kh_mapper * m; bool armed; ~CommitGuard() {if (armed) {m->failed = true;}}} guard{m, true};
  MScan & s = *m->scans[id];
  if (m->p.use_scan_matching) {
    // AddVertex (:1418-1432): the solver node carries the corrected pose
    double node[3];
    put_pose(s.corrected, node);
    if (m->log) {std::fprintf(m->log, "N %d %.17g %.17g %.17g\n", id, node[0], node[1], node[2]);}
    int rc;
    {ProfScope prof(m, kProfAddToGraph); rc = kh_spa_add_node(m->solver, id, node);}
    if (rc) {return rc;}
    const bool previous_gone = last && !m->scans[id - 1];       // AddEdges returns at once (Mapper.cpp:1444-1447)
    if (!previous_gone) {rc = add_edges(m, id, last != nullptr, cov); if (rc) {return rc;}}
    add_running_scan(m, id);
    if (m->p.do_loop_closing) {
      bool closed = false;
      rc = try_close_loop(m, id, closed);
      if (rc) {return rc;}
    }
  }
  m->last = id;
  if (m->lifelong && m->p.use_scan_matching) {
    const int rc = lifelong_step(m, id);
    if (rc) {return rc;}
  }
  // AddScanToLocalizationBuffer (:2911-2937)
  if (to_buffer) {
    m->loc_buffer.push_back(id);
    if (m->loc_buffer.size() > static_cast<size_t>(m->p.scan_buffer_size)) {
      const int rc = evict_front(m);
      if (rc) {return rc;}
    }
  }
  guard.armed = false;
  if (m->log && std::getenv("KH_LOG_FINAL_POSES")) {     // debugging aid, see oracle/ref_slam_driver.cpp
    std::fprintf(m->log, "F %d %.17g %.17g %.17g\n", id, s.corrected.x, s.corrected.y, s.corrected.h);
  }
  *accepted = 1;
  if (corrected_pose) {put_pose(s.corrected, corrected_pose);}
  if (covariance) {std::copy(cov, cov + 9, covariance);}
  m->stats.scans_processed += 1;
  m->stats.process_ms += ms_since(t_begin);
  return KH_OK;
}

// kh_mapper_get_relative_covariances / _difference_covariances: the column of ref_scan made resident when it is not, then `get`
int covariances_against(kh_mapper * m, int32_t ref_scan, int32_t n, const int32_t * scan_ids, double * out, kh_spa_cov_columns_summary * summary,
  int (*get)(kh_spa *, int32_t, int32_t, const int32_t *, double *))
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (n < 0 || (n > 0 && !out)) {return KH_ERR_INVALID_ARG;}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  // (the solver keeps track of whether the column of ref_scan is resident and still belongs to the graph)
  if (!spa_covariance_column_resident(m->solver, ref_scan)) {
    const int rc = kh_spa_compute_covariance_columns(m->solver, 1, &ref_scan, summary);
    if (rc) {return rc;}
  }
  return get(m->solver, ref_scan, n, scan_ids, out);
}
}  // namespace
}  // namespace mapper
}  // namespace kh

using namespace kh;
using namespace kh::mapper;

extern "C" {

void kh_mapper_params_default(kh_mapper_params * p)
{
  if (!p) {return;}
  // config/mapper_params_offline.yaml:31-66 (the offline / sync launches)
  p->use_scan_matching = 1; p->use_scan_barycenter = 1;
  p->minimum_time_interval = 3600.0;                 // Mapper.cpp:2108-2118 (not in the yaml)
  p->minimum_travel_distance = 0.5; p->minimum_travel_heading = 0.5;
  p->scan_buffer_size = 10; p->scan_buffer_maximum_scan_distance = 10.0;
  p->link_match_minimum_response_fine = 0.1; p->link_scan_maximum_distance = 1.5;
  p->loop_search_maximum_distance = 3.0; p->do_loop_closing = 1;
  p->loop_match_minimum_chain_size = 10;
  p->loop_match_maximum_variance_coarse = 3.0 * 3.0;  // the setter squares it (Mapper.cpp:2512-2515)
  p->loop_match_minimum_response_coarse = 0.35; p->loop_match_minimum_response_fine = 0.45;
  p->correlation_search_space_dimension = 0.5; p->correlation_search_space_resolution = 0.01;
  p->correlation_search_space_smear_deviation = 0.1;
  p->loop_search_space_dimension = 8.0; p->loop_search_space_resolution = 0.05; p->loop_search_space_smear_deviation = 0.03;
  p->match.coarse_search_angle_offset = 0.349; p->match.coarse_angle_resolution = 0.0349;
  p->match.fine_search_angle_offset = 0.00349; p->match.use_response_expansion = 1;
  p->match.distance_variance_penalty = 0.5 * 0.5; p->match.minimum_distance_penalty = 0.5;
  p->match.angle_variance_penalty = 1.0 * 1.0; p->match.minimum_angle_penalty = 0.9;
}

int kh_mapper_create_on_devices(const kh_mapper_params * params, const kh_laser * laser, const int32_t * devices, int32_t n_devices,
  int32_t max_candidates, kh_mapper ** out)
{
  if (!out || !params || !laser || laser->n_beams <= 0 || max_candidates < 1 || !devices || n_devices < 1) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  std::unique_ptr<kh_mapper> m(new kh_mapper());
  m->p = *params; m->device = devices[0]; m->max_candidates = max_candidates;
  m->laser = to_laser(*laser);
  std::memset(&m->stats, 0, sizeof(m->stats));
  std::memset(&m->gate_stats, 0, sizeof(m->gate_stats));
  kh_loop_gate_params_default(&m->p, &m->gate);
  auto fail = [&](int rc) {kh_mapper_destroy(m.release()); return rc;};
  // scan copies: one slot per DISTINCT device (members that share a device share the copies)
  for (int32_t k = 0; k < n_devices; ++k) {
    int32_t slot = -1;
    for (size_t q = 0; q < m->slot_device.size(); ++q) {if (m->slot_device[q] == devices[k]) {slot = static_cast<int32_t>(q);}}
    if (slot < 0) {
      if (static_cast<int>(m->slot_device.size()) >= MScan::kMaxDeviceSlots) {
        set_error("kh_mapper_create_on_devices: more than 16 distinct devices");
        return fail(KH_ERR_INVALID_ARG);
      }
      slot = static_cast<int32_t>(m->slot_device.size());
      m->slot_device.push_back(devices[k]);
    }
    m->member_device.push_back(devices[k]);
    m->member_slot.push_back(slot);
  }
  m->n_slots = static_cast<int32_t>(m->slot_device.size());
  // Mapper::Initialize (Mapper.cpp:2606-2631): the sequential matcher; MapperGraph's constructor: the loop matcher (:1397-1400);
  // here one of each per member, member 0 = the reference's two matchers
  int rc = kh_matcher_group_create(params->correlation_search_space_dimension, params->correlation_search_space_resolution,
      params->correlation_search_space_smear_deviation, laser->range_threshold, devices, n_devices, max_candidates, &m->seq_group);
  if (rc) {return fail(rc);}
  rc = kh_matcher_group_create(params->loop_search_space_dimension, params->loop_search_space_resolution,
      params->loop_search_space_smear_deviation, laser->range_threshold, devices, n_devices, max_candidates, &m->loop_group);
  if (rc) {return fail(rc);}
  rc = kh_matcher_group_set_params(m->seq_group, &params->match); if (rc) {return fail(rc);}
  rc = kh_matcher_group_set_params(m->loop_group, &params->match); if (rc) {return fail(rc);}
  m->seq = kh_matcher_group_member(m->seq_group, 0);
  m->loop = kh_matcher_group_member(m->loop_group, 0);
  rc = kh_spa_create(m->device, &m->solver); if (rc) {return fail(rc);}
  rc = kh_graph_create(m->device, &m->graph); if (rc) {return fail(rc);}
  *out = m.release();
  return KH_OK;
}

int kh_mapper_create(const kh_mapper_params * params, const kh_laser * laser, int32_t device, int32_t max_candidates, kh_mapper ** out)
{
  return kh_mapper_create_on_devices(params, laser, &device, 1, max_candidates, out);
}

void kh_mapper_destroy(kh_mapper * m)
{
  if (!m) {return;}
  if (std::getenv("KH_MAPPER_TIMING")) {
    std::fprintf(stderr, "[kh_mapper] host pieces (ms, calls):");
    for (int k = 0; k < kProfPieces; ++k) {if (m->prof_n[k]) {std::fprintf(stderr, "  %s %.1f (%ld)", kProfNames[k], m->prof_ms[k], m->prof_n[k]);}}
    std::fprintf(stderr, "\n");
  }
  if (m->log) {std::fclose(m->log);}
  kh_matcher_group_destroy(m->seq_group); kh_matcher_group_destroy(m->loop_group);
  kh_spa_destroy(m->solver); kh_graph_destroy(m->graph);
  for (auto & slabs : m->d_slabs) {
    for (double * slab : slabs) {kh_device_free(slab);}
  }
  for (double * slab : m->r_slabs) {kh_device_free(slab);}
  delete m;
}

int kh_mapper_set_log(kh_mapper * m, const char * path)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (m->log) {std::fclose(m->log); m->log = nullptr;}
  if (path) {
    m->log = std::fopen(path, "w");
    if (!m->log) {set_error("kh_mapper_set_log: cannot open the file"); return KH_ERR_IO;}
  }
  return KH_OK;
}

kh_spa * kh_mapper_solver(kh_mapper * m) {return m ? m->solver : nullptr;}

int kh_mapper_get_covariances(kh_mapper * m, int32_t n, const int32_t * scan_ids, double * cov, kh_spa_cov_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (n < 0 || (n > 0 && !cov)) {return KH_ERR_INVALID_ARG;}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  // (a scan's solver node carries the scan's id; every change of the graph or of a pose goes through the solver, which keeps
  // track of whether its resident covariances still hold)
  if (!spa_covariances_valid(m->solver)) {
    const int rc = kh_spa_compute_covariances(m->solver, summary);
    if (rc) {return rc;}
  }
  return kh_spa_get_covariances(m->solver, n, scan_ids, cov);
}

int kh_mapper_get_relative_covariances(kh_mapper * m, int32_t ref_scan, int32_t n, const int32_t * scan_ids, double * out, kh_spa_cov_columns_summary * summary)
{
  return covariances_against(m, ref_scan, n, scan_ids, out, summary, kh_spa_get_relative_covariances);
}

int kh_mapper_get_difference_covariances(kh_mapper * m, int32_t ref_scan, int32_t n, const int32_t * scan_ids, double * out, kh_spa_cov_columns_summary * summary)
{
  return covariances_against(m, ref_scan, n, scan_ids, out, summary, kh_spa_get_difference_covariances);
}

// Mapper::Process (Mapper.cpp:2679-2748)
int kh_mapper_process(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time, int32_t * accepted,
  double corrected_pose[3], double covariance[9])
{
  return process_scan(m, Entry::kProcess, -1, false, ranges, odometric_pose, time, accepted, corrected_pose, covariance);
}

// Mapper::ProcessLocalization (Mapper.cpp:2831-2909)
int kh_mapper_process_localization(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time, int32_t * accepted,
  double corrected_pose[3], double covariance[9])
{
  return process_scan(m, Entry::kLocalization, -1, true, ranges, odometric_pose, time, accepted, corrected_pose, covariance);
}

// Mapper::ProcessAgainstNode (Mapper.cpp:3023-3096); ProcessAtDock (:3098-3102) is node 0
int kh_mapper_process_against_node(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time, int32_t node_id,
  int32_t * accepted, double corrected_pose[3], double covariance[9])
{
  return process_scan(m, Entry::kAgainstNode, node_id, false, ranges, odometric_pose, time, accepted, corrected_pose, covariance);
}

// Mapper::ProcessAgainstNodesNearBy (Mapper.cpp:2751-2829)
int kh_mapper_process_against_nodes_near_by(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time,
  int32_t add_to_localization_buffer, int32_t * accepted, double corrected_pose[3], double covariance[9])
{
  return process_scan(m, Entry::kNearBy, -1, add_to_localization_buffer != 0, ranges, odometric_pose, time, accepted, corrected_pose, covariance);
}

// Mapper::ClearLocalizationBuffer (Mapper.cpp:2939-2962)
int kh_mapper_clear_localization_buffer(kh_mapper * m)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  while (!m->loc_buffer.empty()) {
    const int rc = evict_front(m);
    if (rc) {m->failed = true; return rc;}
  }
  m->running.clear();                                  // ClearRunningScans / ClearLastScan of every sensor (:2955-2960)
  m->last = -1;
  return KH_OK;
}

int kh_mapper_localization_buffer(const kh_mapper * m, int32_t * ids, int32_t cap, int32_t * n)
{
  if (!m || !n || cap < 0) {return KH_ERR_INVALID_ARG;}
  *n = static_cast<int32_t>(m->loc_buffer.size());
  if (ids) {std::copy(m->loc_buffer.begin(), m->loc_buffer.begin() + std::min(*n, cap), ids);}
  return KH_OK;
}

int32_t kh_mapper_num_scans(const kh_mapper * m) {return m ? static_cast<int32_t>(m->scans.size()) : 0;}
int64_t kh_mapper_num_edges(const kh_mapper * m) {return m ? m->n_edges : 0;}

int kh_mapper_get_poses(const kh_mapper * m, double * corrected_poses)
{
  if (!m || !corrected_poses) {return KH_ERR_INVALID_ARG;}
  for (size_t i = 0; i < m->scans.size(); ++i) {
    if (!m->scans[i]) {corrected_poses[3 * i] = corrected_poses[3 * i + 1] = corrected_poses[3 * i + 2] = std::nan(""); continue;}   // removed
    put_pose(m->scans[i]->corrected, &corrected_poses[3 * i]);
  }
  return KH_OK;
}

int kh_mapper_get_scan(const kh_mapper * m, int32_t index, kh_scan * scan, kh_scan_box * box)
{
  if (!m || !scan_alive(m, index)) {return KH_ERR_NOT_FOUND;}
  const MScan & s = *m->scans[index];
  if (scan) {*scan = as_kh_scan(s);}
  if (box) {*box = box_of(m, s);}
  return KH_OK;
}

int kh_mapper_get_adjacency(const kh_mapper * m, int32_t scan_id, int32_t * adjacent, int32_t capacity, int32_t * n)
{
  if (!m || !n || !scan_alive(m, scan_id)) {return KH_ERR_NOT_FOUND;}
  const std::vector<int32_t> & a = m->adj[scan_id];
  *n = static_cast<int32_t>(a.size());
  if (adjacent) {std::copy(a.begin(), a.begin() + std::min<size_t>(a.size(), static_cast<size_t>(std::max(capacity, 0))), adjacent);}
  return KH_OK;
}

int kh_mapper_set_node_score(kh_mapper * m, int32_t scan_id, double score)
{
  if (!m || !scan_alive(m, scan_id)) {return KH_ERR_NOT_FOUND;}
  m->scans[scan_id]->score = score;
  return KH_OK;
}

// LocalizedRangeScan::SetCorrectedPose followed by Update (Karto.h:5644-5704): the scan's readings, box and barycentre follow the
// pose.  The solver's node is left alone, as in the reference, so the next CorrectPoses puts the scan where the solver has it.
int kh_mapper_set_scan_pose(kh_mapper * m, int32_t scan_id, const double corrected_pose[3])
{
  if (!m || !corrected_pose) {return KH_ERR_INVALID_ARG;}
  if (!scan_alive(m, scan_id)) {
    set_error("kh_mapper_set_scan_pose: no such scan (unknown or removed)");
    return KH_ERR_NOT_FOUND;
  }
  MScan & s = *m->scans[scan_id];
  s.corrected = to_pose(corrected_pose);
  update_scan(s, m->laser);
  m->graph_dirty = true;
  return KH_OK;
}

int32_t kh_mapper_num_alive(const kh_mapper * m)
{
  int32_t n = 0;
  if (m) {for (const auto & s : m->scans) {n += s ? 1 : 0;}}
  return n;
}

int kh_mapper_get_alive(const kh_mapper * m, int32_t * ids)
{
  if (!m || !ids) {return KH_ERR_INVALID_ARG;}
  int32_t n = 0;
  for (size_t i = 0; i < m->scans.size(); ++i) {if (m->scans[i]) {ids[n++] = static_cast<int32_t>(i);}}
  return KH_OK;
}

int kh_mapper_get_stats(const kh_mapper * m, kh_mapper_stats * out)
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  *out = m->stats;
  int64_t seq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (m->seq && kh_matcher_seq_stats(m->seq, seq) == KH_OK) {
    out->fused_matches = seq[0]; out->fused_fine_passes = seq[1]; out->fused_declined = seq[6]; out->fused_declined_reason = seq[7];
  }
  return KH_OK;
}

int kh_mapper_get_params(const kh_mapper * m, kh_mapper_params * out)
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  *out = m->p;
  return KH_OK;
}

}  // extern "C"
