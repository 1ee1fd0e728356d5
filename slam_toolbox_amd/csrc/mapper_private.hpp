// Private definitions of the mapper front end (kh_mapper_*), shared by its source files:
//   mapper_host.cpp        create / destroy / log, the graph bookkeeping, Process and its four entries, small getters and setters
//   mapper_loop.cpp        the covariance gate and TryCloseLoop
//   mapper_removal.cpp     RemoveNode, marginalizing removal, node decay, edge edits, audit and outlier rejection
//   mapper_session.cpp     the session file: save, load, info
//   mapper_relocalize.cpp  global relocalization
//   mapper_views.cpp       what merge.cpp and live_map.cpp read of a mapper (mapper_internal.hpp: they do not include this header)
// Not part of the ABI (include/karto_hip.h).  The shared names live in kh::mapper; what one file alone uses stays in that file's
// anonymous namespace.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <vector>

#include "../../include/karto_hip.h"
#include "host_common.hpp"
#include "mapper_pose.hpp"       // Pose, MScan, Laser and the reference's arithmetic on them

namespace kh
{
namespace mapper
{
struct MatchOut {double response; double mean[3]; double cov[9];};

// KH_MAPPER_TIMING=1 (measurement aid): the pieces of the host code whose wall time kh_mapper_destroy prints
enum Prof {kProfSyncGraph = 0, kProfNearLinked, kProfDecayBoxes, kProfDecayScores, kProfRemoveNode, kProfUpdateScanNew, kProfAddToGraph,
           kProfLoopEnumeration, kProfLinkNearChains, kProfPieces = 12};
constexpr const char * kProfNames[kProfPieces] = {"sync_graph", "near_linked", "decay_boxes", "decay_scores", "remove_node", "update_scan(new)",
                                                  "add_to_graph", "loop_enumeration", "link_near_chains", "", "", ""};
}  // namespace mapper
}  // namespace kh

struct kh_mapper
{
  kh_mapper_params p;
  kh::mapper::Laser laser;
  int32_t device = 0, max_candidates = 64;
  kh_matcher * seq = nullptr;                            // = member 0 of seq_group
  kh_matcher * loop = nullptr;                           // = member 0 of loop_group
  // candidate batches (loop closure, near chains) are dealt over the members of these groups: one member per entry of the
  // device list the mapper was created on (kh_mapper_create_on_devices), each with its own scan copies
  kh_matcher_group * seq_group = nullptr;
  kh_matcher_group * loop_group = nullptr;
  std::vector<int32_t> member_device;                    // device of member k
  std::vector<int32_t> member_slot;                      // scan-copy slot of member k (members on one device share a slot)
  int32_t n_slots = 1;
  kh_spa * solver = nullptr;
  kh_graph * graph = nullptr;
  std::vector<std::unique_ptr<kh::mapper::MScan>> scans; // processed scans, index = state id = unique id; null once removed
  std::vector<int32_t> alive;                            // ids still in the scan map, ascending: the graph store's scan list
  std::vector<int32_t> compact_of;                       // id -> position in `alive`, -1 when removed
  std::vector<double> sync_xy, sync_pose; std::vector<int32_t> sync_ptr, sync_idx;      // sync_graph's scratch (swapped with the store's arrays)
  std::vector<int32_t> loc_buffer;                       // m_LocalizationScanVertices: ids of the scans localization mode accepted, oldest first
  // KH_MAPPER_TIMING=1 (measurement aid): wall time per piece of the host code (Prof), printed by kh_mapper_destroy
  double prof_ms[kh::mapper::kProfPieces] = {0}; long prof_n[kh::mapper::kProfPieces] = {0};
  bool lifelong = false;
  kh_decay_params decay;
  std::vector<int32_t> running;
  int32_t last = -1;
  // set when Process() fails after its scan was committed to the scan list, the graph store and the solver: the
  // `id - 1 = previous scan` bookkeeping no longer matches, so every later Process() refuses instead of mis-linking
  bool failed = false;
  std::vector<std::vector<int32_t>> adj;                 // Vertex::GetAdjacentVertices order (Mapper.h:338-361)
  std::vector<std::vector<int32_t>> out_edges;           // targets of the edges whose SOURCE is the vertex (AddEdge's duplicate test)
  int64_t n_edges = 0;
  bool graph_dirty = true;
  int32_t removal_mode = KH_REMOVE_PLAIN;                // kh_mapper_set_removal_mode (not part of a session file)
  FILE * log = nullptr;
  kh_mapper_stats stats;
  // the covariance gate of the loop search (kh_mapper_set_loop_gate; not part of a session file)
  kh_loop_gate_params gate;
  kh_loop_gate_stats gate_stats;
  std::vector<double> gate_d;                            // 9 doubles per scan ID: D of the last refresh; ids beyond it (appended since) are zeros
  int32_t gate_age = 0;                                  // try_close_loop calls since the last refresh
  bool gate_due = true;                                  // a refresh is owed whatever the age: never refreshed, or correct_poses has run
  std::vector<double> gate_rows;                         // the prepared rows of one enumeration, in list order
  // device copies of the scans' readings: slots of 2 * laser.n doubles carved from slabs of 256 (one hipMalloc per 256
  // scans instead of one per scan), recycled when a node is removed
  std::vector<double *> d_slabs[kh::mapper::MScan::kMaxDeviceSlots], d_free_slots[kh::mapper::MScan::kMaxDeviceSlots];
  std::vector<int32_t> slot_device;                      // device of scan-copy slot q
  std::vector<double *> r_slabs, r_free_slots;           // the same for the range readings (laser.n doubles per slot, device 0 of the mapper)
  int64_t map_stats[6] = {0, 0, 0, 0, 0, 0};             // kh_mapper_map_stats
};

namespace kh
{
namespace mapper
{
// ---- small idioms, one copy each (ms_between, ms_since: host_common.hpp) ----
struct ProfScope
{
  kh_mapper * m; Prof k; std::chrono::steady_clock::time_point t0;
  ProfScope(kh_mapper * m_, Prof k_) : m(m_), k(k_), t0(std::chrono::steady_clock::now()) {}
  ~ProfScope() {m->prof_ms[k] += ms_since(t0); m->prof_n[k] += 1;}
};

// whether `id` names a scan still in the map
inline bool scan_alive(const kh_mapper * m, int32_t id) {return id >= 0 && id < static_cast<int32_t>(m->scans.size()) && m->scans[id];}

inline Laser to_laser(const kh_laser & l)
{
  Laser L;
  L.n = l.n_beams; L.min_angle = l.minimum_angle; L.ang_res = l.angular_resolution;
  L.min_range = l.minimum_range; L.max_range = l.maximum_range; L.range_threshold = l.range_threshold;
  L.offset.x = l.offset_x; L.offset.y = l.offset_y; L.offset.h = l.offset_heading;
  return L;
}
inline kh_laser to_kh_laser(const Laser & L)
{
  kh_laser l;
  l.n_beams = L.n; l.minimum_angle = L.min_angle; l.angular_resolution = L.ang_res;
  l.minimum_range = L.min_range; l.maximum_range = L.max_range; l.range_threshold = L.range_threshold;
  l.offset_x = L.offset.x; l.offset_y = L.offset.y; l.offset_heading = L.offset.h;
  return l;
}

inline kh_scan as_kh_scan(const MScan & s)
{
  kh_scan k;
  k.n = static_cast<int32_t>(s.ranges.size());
  k.ranges = s.ranges.data();
  k.points_xy = s.points.data();
  put_pose(s.sensor_pose(), k.sensor_pose);
  k.device_points_xy = nullptr;
  return k;
}

inline void reference_xy(const kh_mapper * m, const MScan & s, double xy[2])     // GetReferencePose(useScanBarycenter)
{
  if (m->p.use_scan_barycenter) {xy[0] = s.barycenter[0]; xy[1] = s.barycenter[1];} else {const Pose sp = s.sensor_pose(); xy[0] = sp.x; xy[1] = sp.y;}
}

// Enumerate, grow, enumerate again: call(items, cap, &n) writes at most `cap` items of `per_item` int32 each and says in n how many
// there are; when they did not fit, the call is made once more with room for all.  The first call is timed as `piece`, the retry
// is not.  `items` keeps the capacity of the call that filled it.
template <class Call>
int enumerate_growing(kh_mapper * m, Prof piece, int32_t cap, int32_t per_item, Call call, std::vector<int32_t> & items, int32_t & n)
{
  items.assign(static_cast<size_t>(per_item) * static_cast<size_t>(cap), 0);
  n = 0;
  int rc;
  {
    ProfScope prof(m, piece);
    rc = call(items.data(), cap, &n);
  }
  if (rc || n <= cap) {return rc;}
  items.resize(static_cast<size_t>(per_item) * static_cast<size_t>(n));
  return call(items.data(), n, &n);
}

// ---- mapper_host.cpp ----
// one slot of `doubles_per_slot` doubles on `device`, from the free list or from a new slab of 256 slots (one hipMalloc per 256
// scans instead of one per scan; slots are handed out from the back); nullptr when the slab could not be allocated
double * take_slot(std::vector<double *> & slabs, std::vector<double *> & free_slots, int32_t device, size_t doubles_per_slot);
// the scan's readings resident in scan-copy slot `slot` (= on that slot's device): the device address, or NULL when the
// copy could not be made (the match call then uploads the scan itself)
// on_stream (nullptr = none): the upload is queued on that HIP stream instead of waited for -- for a scan whose next reader is a
// kernel of the same stream (the sequential matcher's: a synchronous copy of 17 KB out of pageable memory costs 25 us of the
// caller's time, once per accepted scan and again for every scan a loop closure moved)
const double * resident_points(kh_mapper * m, MScan & s, int slot, void * on_stream = nullptr);
// the graph store the enumeration kernels and the near-chain walks read: reference positions + adjacency of the scans
// still in the map, in id order (a removed scan is a NULL entry the reference's walks skip)
int sync_graph(kh_mapper * m);
// SetSensorPose (Karto.h:5552-5557): corrected = GetCorrectedAt(pose), then Update
void set_sensor_pose(kh_mapper * m, MScan & s, const double pose[3]);
// the edge from -> to in the mapper's own topology: out_edges, both adjacency lists, n_edges.  graph_dirty and the store's
// incremental kh_graph_add_edge are the caller's (LinkScans and the marginalizing removal differ there)
void attach_edge(kh_mapper * m, int32_t from, int32_t to);
// the solver log's `C from to diff cov` line
void log_constraint(FILE * log, int32_t from, int32_t to, const double diff[3], const double cov[9]);
// MapperGraph::LinkScans (Mapper.cpp:1620-1639) incl. AddEdge's "edge already exists" test (:1585-1618)
int link_scans(kh_mapper * m, int32_t from, int32_t to, const double mean[3], const double cov[9]);
// GetClosestScanToPose (Mapper.cpp:1563-1582): the chain's scan whose reference position is nearest to `pose`, -1 for an empty chain
int32_t closest_scan_to(const kh_mapper * m, const std::vector<int32_t> & chain, const double pose[2]);
// MapperGraph::LinkChainToScan (Mapper.cpp:1665-1681)
int link_chain_to_scan(kh_mapper * m, const std::vector<int32_t> & chain, int32_t scan, const double mean[3], const double cov[9]);
// body(k) for k in [0, n), each a LocalizedRangeScan::Update of one scan, on the host pools: N x P libm sincos that have to stay on
// the host for bit-exactness (Karto.h:5488-5493, 5644-5704)
void update_scans_bulk(size_t n, const std::function<void(size_t)> & body);
// MapperGraph::CorrectPoses (Mapper.cpp:2012-2030)
int correct_poses(kh_mapper * m);
// n independent MatchScan calls (query i against chain i) on the members of `group` (candidate i on member i % members,
// each member on the scan copies of its own device), results in candidate order
int match_chains(kh_mapper * m, kh_matcher_group * group, const std::vector<kh_scan> & queries, const std::vector<std::vector<int32_t>> & chains,
  bool penalize, bool refine, std::vector<MatchOut> & out);
// scan ids of the run [first, last] of the graph store's scan list
std::vector<int32_t> run_of(const kh_mapper * m, int32_t first, int32_t last);

// ---- mapper_loop.cpp ----
// MapperGraph::TryCloseLoop (Mapper.cpp:1500-1561), speculative batches
int try_close_loop(kh_mapper * m, int32_t scan_id, bool & closed);

// ---- mapper_removal.cpp ----
kh_scan_box box_of(const kh_mapper * m, const MScan & s);
// Mapper::RemoveNodeFromGraph (Mapper.cpp:2964-3021) + MapperSensorManager::RemoveScan (:208-218)
// in_solver = false: the solver has already let the node and its constraints go (kh_spa_marginalize_nodes); the log lines stay
int remove_node(kh_mapper * m, int32_t id, bool in_solver = true);
// kh_spa_marginalize_nodes on the mapper's solver, then the same edits in the mapper's own topology, in the order they were made
int marginalize_nodes(kh_mapper * m, int32_t n, const int32_t * ids);
// LifelongSlamToolbox::evaluateNodeDepreciation (slam_toolbox_lifelong.cpp:149-178), lifelong_search_use_tree false
int lifelong_step(kh_mapper * m, int32_t id);

}  // namespace mapper
}  // namespace kh
