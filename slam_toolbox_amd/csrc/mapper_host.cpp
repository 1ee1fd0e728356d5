// ROS-free mapper front end over the GPU hot path: what karto::Mapper::Process does around the scan matcher and the
// solver plugin, so that a scan queue can be replayed end to end (BASELINE configs 1 and 5) without the reference's
// object model.  Everything numeric goes through the library's own entry points -- kh_matcher_* (sequential and loop
// matcher), kh_spa_* (solver plugin), kh_graph_* (candidate enumeration) -- and this file keeps the control flow and the
// small exact host arithmetic (poses, transforms, running-scan buffer, link bookkeeping) in the reference's operation
// order so that the run is comparable call by call with karto::Mapper driving the same queue.
//
// Reference: lib/karto_sdk/src/Mapper.cpp  Process :2679-2748, ProcessLocalization :2831-2909 with AddScanToLocalizationBuffer /
// ClearLocalizationBuffer :2911-2962, ProcessAgainstNodesNearBy :2751-2829, ProcessAgainstNode / ProcessAtDock :3023-3102, HasMovedEnough :3110-3142, ScanManager::AddRunningScan
// :183-206, MapperGraph::AddVertex :1418-1432, AddEdges :1434-1498, TryCloseLoop :1500-1561, LinkScans :1620-1639,
// LinkNearChains :1641-1663, LinkChainToScan :1665-1681, CorrectPoses :2012-2030; Karto.h LocalizedRangeScan::Update
// :5644-5704, GetSensorAt / GetCorrectedAt :5566-5586, Transform :2946-3041, Matrix3::FromAxisAngle :2482-2511.
//
// TryCloseLoop is where the GPU changes the SHAPE of the computation without changing its result: the reference matches
// one candidate chain after another; here all chains FindPossibleLoopClosure would return for the current poses are
// enumerated in one kernel, coarse-matched in one kh_matcher_match_batch, the ones passing the coarse gate fine-matched
// in a second batch, and the results consumed in the reference's order up to the first accepted closure.  CorrectPoses
// then moves every pose, so what was computed for later chains is discarded and the enumeration resumes behind the
// accepted chain with the new poses (closures are rare, the speculation almost always commits).
//
// The four entry points share one body (process_scan): they differ in where the last scan comes from, in the HasMovedEnough gate
// and in what happens to the accepted scan at the very end (the localization buffer).
//
// Scope: one laser (mounted anywhere on the robot: kh_laser::offset_*, Karto.h:5566-5586).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <atomic>
#include <vector>

#include "../../include/karto_hip.h"
#include "mapper_internal.hpp"
#include "marginalize.hpp"

namespace kh
{
void stream_synchronize(void * hip_stream);      // comm.cpp
int decay_scores(int32_t device, const kh_scan_box * reference, int32_t n, const kh_scan_box * candidates, const double * const * resident,
  const uint64_t * const * masks, int32_t n_scan, const kh_decay_params * params, int32_t * kept, double * iou, double * area_overlap,
  double * reading_overlap, double * scores);                                                                       // lifelong.hip
void set_pending_query_hook(std::function<void()> fn);       // matcher_seq.cpp (QueryHook, matcher_private.hpp)
void run_pending_query_hook();
void spa_export_session_state(kh_spa * s, int64_t words[7], std::vector<int32_t> & sn_ptr, std::vector<int32_t> & sn_ids);
void spa_import_session_state(kh_spa * s, const int64_t words[7], const std::vector<int32_t> & sn_ptr, const std::vector<int32_t> & sn_ids);
bool spa_covariances_valid(const kh_spa * s);
bool spa_covariance_column_resident(const kh_spa * s, int32_t id);
bool spa_covariance_has_node(const kh_spa * s, int32_t id);
const std::vector<MargEdit> & spa_marginalize_edits(const kh_spa * s);       // spa_host.cpp (MargEdit: marginalize.hpp)
bool spa_marginalize_refuses(const kh_spa * s, int32_t id);
int graph_swap(kh_graph * g, int32_t n_scans, std::vector<double> & ref_xy, std::vector<int32_t> & adj_ptr, std::vector<int32_t> & adj_idx,
  std::vector<double> & pose_xy);   // graph.hip
int graph_relocalize_candidates(kh_graph * g, double seed_spacing, double base_radius, int32_t max_base, const double * center_xy, double radius,
  std::vector<int32_t> & seeds, std::vector<int32_t> & base_begin, std::vector<int32_t> & base_idx);   // graph.hip

void set_error(const std::string & s);
void host_parallel_for(size_t n, const std::function<void(size_t)> & fn);
void host_parallel_for_wide(size_t n, const std::function<void(size_t)> & fn);

namespace
{
// cos and sin of ONE angle, the way the reference's Release build computes them: GCC (-O1 and up) merges a cos(a) / sin(a)
// pair into one sincos(a) call, and glibc's sincos is NOT bit-identical to its cos and sin everywhere (a = 0.11462314399891493:
// cos(a) = 0.9934379567501339, sincos(a) gives 0.993437956750134).  Every place where the reference takes both of the same
// angle goes through here, so that the library does not depend on whether ITS compiler merges the pair (clang does not).
static inline void ref_sincos(double a, double * s, double * c) {::sincos(a, s, c);}
constexpr double kTolerance = 1e-06;                  // KT_TOLERANCE, Math.h:41
constexpr double kPi = 3.14159265358979323846;        // Math.h:31
constexpr double k2Pi = 6.28318530717958647692;       // Math.h:32

double normalize_angle(double angle)                  // math::NormalizeAngle, Math.h:181-202
{
  while (angle < -kPi) {
    if (angle < -k2Pi) {angle += static_cast<uint32_t>(angle / -k2Pi) * k2Pi;} else {angle += k2Pi;}
  }
  while (angle > kPi) {
    if (angle > k2Pi) {angle -= static_cast<uint32_t>(angle / k2Pi) * k2Pi;} else {angle -= k2Pi;}
  }
  return angle;
}

struct Pose {double x = 0.0, y = 0.0, h = 0.0;};
inline bool same_pose(const Pose & a, const Pose & b) {return a.x == b.x && a.y == b.y && a.h == b.h;}   // Karto.h:2180-2183

struct Mat3
{
  double m[3][3];
  void identity() {std::memset(m, 0, sizeof(m)); m[0][0] = m[1][1] = m[2][2] = 1.0;}
  // Rodrigues' rotation about a unit axis, in the operation order of Matrix3::FromAxisAngle (Karto.h:2482-2511) -- the solver log
  // is compared with the reference's at 17 digits: diagonal a_i a_i (1 - c) + c; off-diagonal (a_i a_j)(1 - c) -+ a_k s, "+" where
  // (i, j, k) is an odd permutation
  void from_axis_angle(double ax, double ay, double az, double angle)
  {
    const double axis[3] = {ax, ay, az};
    double s, c;
    ref_sincos(angle, &s, &c);
    const double versine = 1.0 - c;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) {
        if (i == j) {m[i][i] = axis[i] * axis[i] * versine + c; continue;}
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const double symmetric = axis[lo] * axis[hi] * versine, skew = axis[3 - i - j] * s;
        m[i][j] = ((j - i + 3) % 3 == 2) ? symmetric + skew : symmetric - skew;
      }
    }
  }
  Pose mul(const Pose & p) const                                          // Matrix3 * Pose2, Karto.h:2654-2666
  {
    Pose r;
    r.x = m[0][0] * p.x + m[0][1] * p.y + m[0][2] * p.h;
    r.y = m[1][0] * p.x + m[1][1] * p.y + m[1][2] * p.h;
    r.h = m[2][0] * p.x + m[2][1] * p.y + m[2][2] * p.h;
    return r;
  }
};

// karto::Transform(rPose1, rPose2).TransformPose(src), Karto.h:2946-3024
Pose transform_pose(const Pose & p1, const Pose & p2, const Pose & src)
{
  Mat3 rot;
  Pose t;
  if (same_pose(p1, p2)) {
    rot.identity();
  } else {
    rot.from_axis_angle(0, 0, 1, p2.h - p1.h);
    if (p1.x != 0.0 || p1.y != 0.0) {
      const Pose r = rot.mul(p1);
      t.x = p2.x - r.x; t.y = p2.y - r.y;
    } else {
      t.x = p2.x; t.y = p2.y;
    }
    t.h = p2.h - p1.h;
  }
  const Pose r = rot.mul(src);
  Pose out;
  out.x = t.x + r.x; out.y = t.y + r.y;
  out.h = normalize_angle(src.h + t.h);
  return out;
}

// One processed scan: what LocalizedRangeScan holds (zero mount offset: the sensor pose is the corrected pose with its
// heading normalised, GetSensorAt / GetCorrectedAt Karto.h:5566-5586)
struct MScan
{
  int32_t id = -1;
  double time = 0.0;
  Pose odometric, corrected;
  std::vector<double> ranges;
  std::vector<double> points;        // unfiltered point readings, x0 y0 x1 y1 ...
  std::vector<double> filtered;      // point readings with the range inside [minimum range, range threshold]
  std::vector<uint64_t> filter_mask; // bit i: reading i is one of `filtered` (the node-decay kernel reads `points` in HBM through it)
  double score = 1.0;                // Vertex::GetScore (Mapper.h: vertices start at 1.0)
  double barycenter[2] = {0.0, 0.0};
  double bbox[4] = {0.0, 0.0, 0.0, 0.0};   // min x, min y, max x, max y of the sensor position and the filtered readings
  int32_t n_filtered = 0;
  // the unfiltered readings once more, in HBM: as a base scan of a match the scan is read where it lies (kh_scan::
  // device_points_xy).  Uploaded on first use and again after the pose has moved (update_scan marks it stale).
  static constexpr int kMaxDeviceSlots = 16;
  double * d_points[kMaxDeviceSlots] = {};       // one copy per distinct device of the mapper (slot 0 = the mapper's own device)
  uint16_t d_fresh = 0;                          // bit k: the copy in slot k holds the current points
  // the range readings in HBM on the mapper's own device (kh_mapper_build_map reads them there): they never change after the scan
  // is made, so they are uploaded once
  double * d_ranges = nullptr;
  bool d_ranges_fresh = false;
  Pose sensor;                                   // GetSensorAt(corrected), refreshed by update_scan (every write of `corrected` is followed by one)
  Pose sensor_pose() const {return sensor;}
  MScan() = default;
  MScan(const MScan &) = delete;
  MScan & operator=(const MScan &) = delete;
  // d_points is a slot of the mapper's device slabs (take_slot / remove_node / kh_mapper_destroy), not owned here
};

struct Laser
{
  int32_t n = 0;
  double min_angle = 0, ang_res = 0, min_range = 0, max_range = 0, range_threshold = 0;
  Pose offset;                                   // LaserRangeFinder::GetOffsetPose: the sensor in the robot's frame
};

// LocalizedRangeScan::GetSensorAt (Karto.h:5566-5569): Transform(robot pose).TransformPose(offset pose)
Pose sensor_at(const Laser & L, const Pose & robot) {return transform_pose(Pose(), robot, L.offset);}

// LocalizedRangeScan::GetCorrectedAt (Karto.h:5576-5588): the robot pose that puts the sensor at `sensor`
Pose corrected_at(const Laser & L, const Pose & sensor)
{
  const double offset_length = std::sqrt(L.offset.x * L.offset.x + L.offset.y * L.offset.y);       // Vector2::Length
  const double offset_heading = L.offset.h;
  const double angle_offset = std::atan2(L.offset.y, L.offset.x);
  const double heading = normalize_angle(sensor.h);
  double sin_w, cos_w;
  ref_sincos(heading + angle_offset - offset_heading, &sin_w, &cos_w);
  Pose robot;                                      // Pose2::operator-: positions subtract, the heading difference is normalised
  robot.x = sensor.x - offset_length * cos_w;
  robot.y = sensor.y - offset_length * sin_w;
  robot.h = normalize_angle(sensor.h - offset_heading);
  return robot;
}

// LocalizedRangeScan::Update, Karto.h:5644-5704
void update_scan(MScan & s, const Laser & L)
{
  s.sensor = sensor_at(L, s.corrected);
  const Pose sp = s.sensor;
  s.points.resize(2 * static_cast<size_t>(L.n));
  s.d_fresh = 0;
  s.filtered.clear();
  s.filter_mask.assign((static_cast<size_t>(L.n) + 63) / 64, 0);
  double sum_x = 0.0, sum_y = 0.0;
  int32_t n_filtered = 0;
  double bb[4] = {sp.x, sp.y, sp.x, sp.y};
  for (int32_t i = 0; i < L.n; ++i) {
    const double r = s.ranges[i];
    const double angle = sp.h + L.min_angle + static_cast<uint32_t>(i) * L.ang_res;
    double sin_a, cos_a;
    ref_sincos(angle, &sin_a, &cos_a);
    const double px = sp.x + (r * cos_a);
    const double py = sp.y + (r * sin_a);
    s.points[2 * i] = px; s.points[2 * i + 1] = py;
    if (r >= L.min_range && r <= L.range_threshold) {          // math::InRange
      sum_x += px; sum_y += py; ++n_filtered;
      s.filtered.push_back(px); s.filtered.push_back(py);
      s.filter_mask[static_cast<size_t>(i) >> 6] |= 1ull << (i & 63);
      bb[0] = std::min(bb[0], px); bb[1] = std::min(bb[1], py); bb[2] = std::max(bb[2], px); bb[3] = std::max(bb[3], py);
    }
  }
  const double n_points = static_cast<double>(n_filtered);
  if (n_points != 0.0) {
    s.barycenter[0] = sum_x / n_points; s.barycenter[1] = sum_y / n_points;
  } else {
    s.barycenter[0] = sp.x; s.barycenter[1] = sp.y;
  }
  s.n_filtered = n_filtered;
  std::copy(bb, bb + 4, s.bbox);
}

}  // namespace
}  // namespace kh

using namespace kh;

struct kh_mapper
{
  kh_mapper_params p;
  Laser laser;
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
  std::vector<std::unique_ptr<MScan>> scans;             // processed scans, index = state id = unique id; null once removed
  std::vector<int32_t> alive;                            // ids still in the scan map, ascending: the graph store's scan list
  std::vector<int32_t> compact_of;                       // id -> position in `alive`, -1 when removed
  std::vector<double> sync_xy, sync_pose; std::vector<int32_t> sync_ptr, sync_idx;      // sync_graph's scratch (swapped with the store's arrays)
  std::vector<int32_t> loc_buffer;                       // m_LocalizationScanVertices: ids of the scans localization mode accepted, oldest first
  // KH_MAPPER_TIMING=1 (measurement aid): wall time per piece of the host code, printed by kh_mapper_destroy
  double prof_ms[12] = {0}; long prof_n[12] = {0};
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
  std::vector<double *> d_slabs[MScan::kMaxDeviceSlots], d_free_slots[MScan::kMaxDeviceSlots];
  std::vector<int32_t> slot_device;                      // device of scan-copy slot q
  std::vector<double *> r_slabs, r_free_slots;           // the same for the range readings (laser.n doubles per slot, device 0 of the mapper)
  int64_t map_stats[6] = {0, 0, 0, 0, 0, 0};             // kh_mapper_map_stats
};

namespace kh
{
namespace
{

kh_scan as_kh_scan(const MScan & s)
{
  kh_scan k;
  k.n = static_cast<int32_t>(s.ranges.size());
  k.ranges = s.ranges.data();
  k.points_xy = s.points.data();
  const Pose sp = s.sensor_pose();
  k.sensor_pose[0] = sp.x; k.sensor_pose[1] = sp.y; k.sensor_pose[2] = sp.h;
  k.device_points_xy = nullptr;
  return k;
}

// the scan's readings resident in scan-copy slot `slot` (= on that slot's device): the device address, or NULL when the
// copy could not be made (the match call then uploads the scan itself)
// on_stream (nullptr = none): the upload is queued on that HIP stream instead of waited for -- for a scan whose next reader is a
// kernel of the same stream (the sequential matcher's: a synchronous copy of 17 KB out of pageable memory costs 25 us of the
// caller's time, once per accepted scan and again for every scan a loop closure moved)
const double * resident_points(kh_mapper * m, MScan & s, int slot, void * on_stream = nullptr)
{
  const int64_t bytes = static_cast<int64_t>(sizeof(double)) * static_cast<int64_t>(s.points.size());
  if (bytes <= 0 || s.points.size() != 2 * static_cast<size_t>(m->laser.n)) {return nullptr;}
  if (!s.d_points[slot]) {
    if (m->d_free_slots[slot].empty()) {
      constexpr int kSlabScans = 256;
      void * p = nullptr;
      if (kh_device_malloc(m->slot_device[slot], bytes * kSlabScans, &p) == KH_OK) {
        m->d_slabs[slot].push_back(static_cast<double *>(p));
        for (int k = kSlabScans - 1; k >= 0; --k) {m->d_free_slots[slot].push_back(static_cast<double *>(p) + static_cast<size_t>(k) * s.points.size());}
      }
    }
    if (!m->d_free_slots[slot].empty()) {
      s.d_points[slot] = m->d_free_slots[slot].back(); m->d_free_slots[slot].pop_back();
      s.d_fresh &= static_cast<uint16_t>(~(1u << slot));
    }
  }
  if (s.d_points[slot] && !(s.d_fresh & (1u << slot)) &&
    (on_stream ? kh_device_upload_on(s.d_points[slot], s.points.data(), bytes, on_stream) : kh_device_upload(s.d_points[slot], s.points.data(), bytes)) == KH_OK) {
    s.d_fresh |= static_cast<uint16_t>(1u << slot);
  }
  return (s.d_points[slot] && (s.d_fresh & (1u << slot))) ? s.d_points[slot] : nullptr;
}

// the scan as a BASE scan of a match on the mapper's own device: its readings resident there
kh_scan as_base_scan(kh_mapper * m, MScan & s, void * on_stream = nullptr)
{
  kh_scan k = as_kh_scan(s);
  k.device_points_xy = resident_points(m, s, 0, on_stream);
  return k;
}

void reference_xy(const kh_mapper * m, const MScan & s, double xy[2])     // GetReferencePose(useScanBarycenter)
{
  if (m->p.use_scan_barycenter) {xy[0] = s.barycenter[0]; xy[1] = s.barycenter[1];} else {const Pose sp = s.sensor_pose(); xy[0] = sp.x; xy[1] = sp.y;}
}

// the graph store the enumeration kernels and the near-chain walks read: reference positions + adjacency of the scans
// still in the map, in id order (a removed scan is a NULL entry the reference's walks skip)
struct ProfScope
{
  kh_mapper * m; int k; std::chrono::steady_clock::time_point t0;
  ProfScope(kh_mapper * m_, int k_) : m(m_), k(k_), t0(std::chrono::steady_clock::now()) {}
  ~ProfScope() {m->prof_ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); m->prof_n[k] += 1;}
};
static const char * const kProfNames[12] = {"sync_graph", "near_linked", "decay_boxes", "decay_scores", "remove_node", "update_scan(new)", "add_to_graph",
                                           "loop_enumeration", "link_near_chains", "", "", ""};

int sync_graph(kh_mapper * m)
{
  ProfScope prof(m, 0);
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
  int rc = kh::graph_swap(m->graph, static_cast<int32_t>(n), xy, ptr, idx, pose);
  if (rc) {return rc;}
  // the reference bounds its candidate walks by the scan map's SIZE, in id space (Mapper.cpp:1974-1976, 1751-1756)
  const int32_t n_visit = static_cast<int32_t>(std::lower_bound(m->alive.begin(), m->alive.end(), static_cast<int32_t>(n)) - m->alive.begin());
  rc = kh_graph_set_scan_limit(m->graph, n_visit);
  if (rc == KH_OK) {m->graph_dirty = false;}
  return rc;
}

// SetSensorPose (Karto.h:5552-5557): corrected = GetCorrectedAt(pose), then Update
void set_sensor_pose(kh_mapper * m, MScan & s, const double pose[3])
{
  Pose sensor; sensor.x = pose[0]; sensor.y = pose[1]; sensor.h = pose[2];
  s.corrected = corrected_at(m->laser, sensor);
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

// MapperGraph::LinkScans (Mapper.cpp:1620-1639) incl. AddEdge's "edge already exists" test (:1585-1618)
int link_scans(kh_mapper * m, int32_t from, int32_t to, const double mean[3], const double cov[9])
{
  for (int32_t t : m->out_edges[from]) {if (t == to) {return KH_OK;}}     // not a new edge: nothing is attached
  m->out_edges[from].push_back(to);
  m->adj[from].push_back(to);
  m->adj[to].push_back(from);
  ++m->n_edges;
  // the store follows edit by edit while nothing was removed or re-posed since it was built (sync_graph rebuilds otherwise)
  if (!m->graph_dirty && kh_graph_add_edge(m->graph, m->compact_of[from], m->compact_of[to]) != KH_OK) {m->graph_dirty = true;}
  // LinkInfo(pFromScan->GetCorrectedPose(), pToScan->GetCorrectedAt(rMean), rCovariance)
  const MScan & f = *m->scans[from];
  const double pose1[3] = {f.corrected.x, f.corrected.y, f.corrected.h};
  Pose mean_sensor; mean_sensor.x = mean[0]; mean_sensor.y = mean[1]; mean_sensor.h = mean[2];
  const Pose to_robot = corrected_at(m->laser, mean_sensor);
  const double pose2[3] = {to_robot.x, to_robot.y, to_robot.h};
  double diff[3], cov_out[9];
  int rc = kh_link_info(pose1, pose2, cov, diff, cov_out);
  if (rc) {return rc;}
  if (m->log) {
    std::fprintf(m->log, "C %d %d %.17g %.17g %.17g", from, to, diff[0], diff[1], diff[2]);
    for (int k = 0; k < 9; ++k) {std::fprintf(m->log, " %.17g", cov_out[k]);}
    std::fprintf(m->log, "\n");
  }
  rc = kh_spa_add_constraint(m->solver, from, to, diff, cov_out);
  // the plugin logs and carries on when it cannot add a constraint (ceres_solver.cpp:354-361)
  return (rc == KH_OK || rc == KH_ERR_NOT_FOUND || rc == KH_ERR_INVALID_ARG) ? KH_OK : rc;
}

// GetClosestScanToPose (Mapper.cpp:1563-1582): the chain's scan whose reference position is nearest to `pose`, -1 for an empty chain
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

// MapperGraph::LinkChainToScan (Mapper.cpp:1665-1681)
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

// MapperGraph::CorrectPoses (Mapper.cpp:2012-2030)
int correct_poses(kh_mapper * m)
{
  const auto t0 = std::chrono::steady_clock::now();
  kh_spa_summary sum;
  const int rc = kh_spa_compute(m->solver, &sum);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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
  auto one = [&](size_t k) {
    const int32_t id = ids[k];
    if (id < 0 || id >= static_cast<int32_t>(m->scans.size()) || !m->scans[id]) {return;}
    MScan & s = *m->scans[id];
    // (a pose the solve left bit for bit where it was -- a component the closure did not touch and whose own residuals are at
    // rest -- re-projects to the same readings: nothing to do, and the device copy stays valid)
    if (std::memcmp(&s.corrected.x, &poses[3 * k], sizeof(double)) == 0 && std::memcmp(&s.corrected.y, &poses[3 * k + 1], sizeof(double)) == 0 &&
      std::memcmp(&s.corrected.h, &poses[3 * k + 2], sizeof(double)) == 0) {return;}
    s.corrected.x = poses[3 * k]; s.corrected.y = poses[3 * k + 1]; s.corrected.h = poses[3 * k + 2];
    update_scan(s, m->laser);
  };
  // thousands of scans x 1081 sincos: wider than the matcher's worker pool (32 threads suit its sub-millisecond bursts;
  // this is milliseconds of uniform work -- N x 1081 libm calls that have to stay on the host for bit-exactness,
  // Karto.h:5488-5493, 5644-5704 -- so it goes to the wide pool in chunks of 32 scans)
  if (n >= 2048) {
    const size_t chunks = (static_cast<size_t>(n) + 31) / 32;
    host_parallel_for_wide(chunks, [&](size_t c) {
      for (size_t k = 32 * c; k < std::min(static_cast<size_t>(n), 32 * c + 32); ++k) {one(k);}
    });
  } else {
    host_parallel_for(static_cast<size_t>(n), one);
  }
  m->stats.update_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  m->graph_dirty = true;
  if (m->log) {std::fprintf(m->log, "K\n");}
  return kh_spa_clear(m->solver);
}

struct MatchOut {double response; double mean[3]; double cov[9];};

// n independent MatchScan calls (query i against chain i) on the members of `group` (candidate i on member i % members,
// each member on the scan copies of its own device), results in candidate order
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
  m->stats.match_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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

// scan ids of the run [first, last] of the graph store's scan list
std::vector<int32_t> run_of(const kh_mapper * m, int32_t first, int32_t last)
{
  std::vector<int32_t> v;
  for (int32_t i = first; i <= last; ++i) {v.push_back(m->alive[i]);}
  return v;
}

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
  m->gate_stats.column_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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
  Pose at; at.x = mean[0]; at.y = mean[1]; at.h = mean[2];
  moved.corrected = corrected_at(m->laser, at);
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

// MapperGraph::TryCloseLoop (Mapper.cpp:1500-1561), speculative batches
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
    auto enumerate = [&](int32_t n_q, const int32_t * q, const int32_t * st, int32_t * begin, int32_t * out, int32_t cap, int32_t * total) {
      if (!gated) {
        return kh_graph_find_loop_candidates_from(m->graph, n_q, q, st, m->p.loop_search_maximum_distance, m->p.loop_match_minimum_chain_size,
                 begin, out, cap, total);
      }
      return kh_graph_find_loop_candidates_gated(m->graph, n_q, q, st, m->p.loop_search_maximum_distance, m->p.loop_match_minimum_chain_size,
               m->gate.chi2_position, m->gate_rows.data(), begin, out, cap, total);
    };
    // positions in the graph store's scan list (= the scans still alive, in id order)
    const int32_t query = m->compact_of[scan_id];
    int32_t start = static_cast<int32_t>(std::lower_bound(m->alive.begin(), m->alive.end(), start_id) - m->alive.begin());
    // every chain successive FindPossibleLoopClosure calls would return from `start` on, for the CURRENT poses
    std::vector<int32_t> chain_begin(2, 0), flat(2 * static_cast<size_t>(m->max_candidates));
    int32_t n_chains = 0;
    int rc;
    {ProfScope prof(m, 7);
    rc = enumerate(1, &query, &start, chain_begin.data(), flat.data(), m->max_candidates, &n_chains);
    }
    if (rc) {return rc;}
    if (n_chains > m->max_candidates) {
      flat.resize(2 * static_cast<size_t>(n_chains));
      rc = enumerate(1, &query, &start, chain_begin.data(), flat.data(), n_chains, &n_chains);
      if (rc) {return rc;}
    }
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
      t->ranges = scan.ranges; t->corrected = scan.corrected;
      Pose best; best.x = coarse[c].mean[0]; best.y = coarse[c].mean[1]; best.h = coarse[c].mean[2];
      t->corrected = corrected_at(m->laser, best);                 // tmpScan.SetSensorPose(bestPose), Mapper.cpp:1533
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

// Mapper::RemoveNodeFromGraph (Mapper.cpp:2964-3021) + MapperSensorManager::RemoveScan (:208-218)
// in_solver = false: the solver has already let the node and its constraints go (kh_spa_marginalize_nodes); the log lines stay
int remove_node(kh_mapper * m, int32_t id, bool in_solver = true)
{
  ProfScope prof(m, 4);
  if (id < 0 || id >= static_cast<int32_t>(m->scans.size()) || !m->scans[id]) {
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

// kh_spa_marginalize_nodes on the mapper's solver, then the same edits in the mapper's own topology, in the order they were made
int marginalize_nodes(kh_mapper * m, int32_t n, const int32_t * ids)
{
  for (int32_t k = 0; k < n; ++k) {
    if (ids[k] < 0 || ids[k] >= static_cast<int32_t>(m->scans.size()) || !m->scans[ids[k]]) {
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
      std::fprintf(m->log, "C %d %d %.17g %.17g %.17g", e.a, e.b, e.z[0], e.z[1], e.z[2]);
      for (int k = 0; k < 9; ++k) {std::fprintf(m->log, " %.17g", cov[k]);}
      std::fprintf(m->log, "\n");
    }
    if (e.kind == 0) {                       // a new edge, the hub its source; a fused constraint changes nothing here
      m->out_edges[e.a].push_back(e.b);
      m->adj[e.a].push_back(e.b);
      m->adj[e.b].push_back(e.a);
      ++m->n_edges;
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

// LifelongSlamToolbox::evaluateNodeDepreciation (slam_toolbox_lifelong.cpp:149-178), lifelong_search_use_tree false
int lifelong_step(kh_mapper * m, int32_t id)
{
  const auto t0 = std::chrono::steady_clock::now();
  const MScan & s = *m->scans[id];
  const double w = s.bbox[2] - s.bbox[0], h = s.bbox[3] - s.bbox[1];
  const double radius = std::sqrt(w * w + h * h) / 2.0;
  if (m->graph_dirty) {const int rc = sync_graph(m); if (rc) {return rc;}}
  std::vector<int32_t> near(64);
  int32_t n = 0;
  int rc;
  {
  ProfScope prof(m, 1);
  rc = kh_graph_find_near_linked(m->graph, m->compact_of[id], radius, near.data(), static_cast<int32_t>(near.size()), &n);
  }
  if (rc) {return rc;}
  if (n > static_cast<int32_t>(near.size())) {
    near.resize(static_cast<size_t>(n));
    rc = kh_graph_find_near_linked(m->graph, m->compact_of[id], radius, near.data(), n, &n);
    if (rc) {return rc;}
  }
  near.resize(static_cast<size_t>(n));
  for (int32_t & c : near) {c = m->alive[c];}                     // graph store positions -> scan ids
  const kh_scan_box ref = box_of(m, s);
  std::vector<kh_scan_box> cands;
  // the candidates' readings where the matcher left them in HBM (a copy a pose update made stale is refreshed first); a scan
  // without a device copy (slot allocation failed) sends the whole call down the packed form
  std::vector<const double *> resident;
  std::vector<const uint64_t *> masks;
  bool all_resident = m->laser.n <= 4096;
  {ProfScope prof(m, 2);
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
  {ProfScope prof(m, 3);
  rc = kh::decay_scores(m->device, &ref, n, cands.data(), all_resident ? resident.data() : nullptr, all_resident ? masks.data() : nullptr,
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
  m->stats.lifelong_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return KH_OK;
}

}  // namespace
}  // namespace kh

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
  m->laser.n = laser->n_beams; m->laser.min_angle = laser->minimum_angle; m->laser.ang_res = laser->angular_resolution;
  m->laser.min_range = laser->minimum_range; m->laser.max_range = laser->maximum_range; m->laser.range_threshold = laser->range_threshold;
  m->laser.offset.x = laser->offset_x; m->laser.offset.y = laser->offset_y; m->laser.offset.h = laser->offset_heading;
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
        kh::set_error("kh_mapper_create_on_devices: more than 16 distinct devices");
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
    for (int k = 0; k < 12; ++k) {if (m->prof_n[k]) {std::fprintf(stderr, "  %s %.1f (%ld)", kh::kProfNames[k], m->prof_ms[k], m->prof_n[k]);}}
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
    if (!m->log) {kh::set_error("kh_mapper_set_log: cannot open the file"); return KH_ERR_IO;}
  }
  return KH_OK;
}

kh_spa * kh_mapper_solver(kh_mapper * m) {return m ? m->solver : nullptr;}

int kh_mapper_get_covariances(kh_mapper * m, int32_t n, const int32_t * scan_ids, double * cov, kh_spa_cov_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (n < 0 || (n > 0 && !cov)) {return KH_ERR_INVALID_ARG;}
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  // (a scan's solver node carries the scan's id; every change of the graph or of a pose goes through the solver, which keeps
  // track of whether its resident covariances still hold)
  if (!kh::spa_covariances_valid(m->solver)) {
    const int rc = kh_spa_compute_covariances(m->solver, summary);
    if (rc) {return rc;}
  }
  return kh_spa_get_covariances(m->solver, n, scan_ids, cov);
}

int kh_mapper_get_relative_covariances(kh_mapper * m, int32_t ref_scan, int32_t n, const int32_t * scan_ids, double * out, kh_spa_cov_columns_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (n < 0 || (n > 0 && !out)) {return KH_ERR_INVALID_ARG;}
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  // (the solver keeps track of whether the column of ref_scan is resident and still belongs to the graph)
  if (!kh::spa_covariance_column_resident(m->solver, ref_scan)) {
    const int rc = kh_spa_compute_covariance_columns(m->solver, 1, &ref_scan, summary);
    if (rc) {return rc;}
  }
  return kh_spa_get_relative_covariances(m->solver, ref_scan, n, scan_ids, out);
}

int kh_mapper_get_difference_covariances(kh_mapper * m, int32_t ref_scan, int32_t n, const int32_t * scan_ids, double * out, kh_spa_cov_columns_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (n < 0 || (n > 0 && !out)) {return KH_ERR_INVALID_ARG;}
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (!kh::spa_covariance_column_resident(m->solver, ref_scan)) {
    const int rc = kh_spa_compute_covariance_columns(m->solver, 1, &ref_scan, summary);
    if (rc) {return rc;}
  }
  return kh_spa_get_difference_covariances(m->solver, ref_scan, n, scan_ids, out);
}

}  // extern "C"
namespace kh
{
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

enum class Entry {kProcess, kLocalization, kAgainstNode, kNearBy};

// The body Mapper::Process (Mapper.cpp:2679-2748), ProcessLocalization (:2831-2909), ProcessAgainstNode (:3023-3096) and
// ProcessAgainstNodesNearBy (:2751-2829) share
int process_scan(kh_mapper * m, Entry entry, int32_t node_id, bool to_buffer, const double * ranges, const double odometric_pose[3], double time,
  int32_t * accepted, double corrected_pose[3], double covariance[9])
{
  if (!m || !ranges || !odometric_pose || !accepted) {return KH_ERR_INVALID_ARG;}
  *accepted = 0;
  if (m->failed) {
    kh::set_error("kh_mapper_process: an earlier call failed after its scan had entered the graph; the handle is unusable");
    return KH_ERR_SOLVER;
  }
  if (to_buffer && m->p.scan_buffer_size < 1) {
    kh::set_error("localization mode needs scan_buffer_size >= 1 (the accepted scan would evict itself)");
    return KH_ERR_INVALID_ARG;
  }
  const bool gated = entry == Entry::kProcess || entry == Entry::kLocalization;
  if (entry == Entry::kAgainstNode && (node_id < 0 || node_id >= static_cast<int32_t>(m->scans.size()) || !m->scans[node_id])) {
    kh::set_error("ProcessAgainstNode: no such node (unknown or removed)");         // the reference dereferences NULL (:3043-3046)
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
  scan->odometric.x = odometric_pose[0]; scan->odometric.y = odometric_pose[1]; scan->odometric.h = odometric_pose[2];
  scan->corrected = scan->odometric;                      // the caller's SetCorrectedPose(odometric pose)
  MScan * last = m->last >= 0 ? m->scans[m->last].get() : nullptr;
  // update the scan's corrected pose based on the last correction (:2699-2703); not on the near-pose entries, whose caller has put
  // the scan where the match should start
  if (last && gated) {scan->corrected = transform_pose(last->odometric, last->corrected, scan->odometric);}
  // HasMovedEnough (:3110-3142)
  if (last && gated) {
    bool moved = false;
    if (scan->time - last->time >= m->p.minimum_time_interval) {moved = true;}
    // the scanner's pose for the two odometric poses (GetSensorAt, :3123-3124)
    const Pose last_scanner = sensor_at(m->laser, last->odometric), scanner = sensor_at(m->laser, scan->odometric);
    if (!moved) {
      const double deltaHeading = normalize_angle(scanner.h - last_scanner.h);
      if (std::fabs(deltaHeading) >= m->p.minimum_travel_heading) {moved = true;}
    }
    if (!moved) {
      const double dx = last_scanner.x - scanner.x, dy = last_scanner.y - scanner.y;
      if (dx * dx + dy * dy >= m->p.minimum_travel_distance * m->p.minimum_travel_distance - kTolerance) {moved = true;}
    }
    if (!moved) {return KH_OK;}
  }
  double cov[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (!(m->p.use_scan_matching && last)) {ProfScope prof(m, 5); update_scan(*scan, m->laser);}
  // correct the scan against the running scans (:2713-2724)
  if (m->p.use_scan_matching && last) {
    // LocalizedRangeScan::Update of the new scan (1081 sincos) is handed to the matcher as a QueryHook: the match's rasteriser needs
    // the query's sensor pose and nothing else of it, so the readings are computed behind its launches, while the GPU works; the
    // matcher runs the hook before anything reads the readings, whatever path the call takes, and before it returns
    MScan * const sp = scan.get();
    sp->sensor = sensor_at(m->laser, sp->corrected);
    sp->points.assign(2 * static_cast<size_t>(m->laser.n), 0.0);
    const kh_scan q = as_kh_scan(*sp);
    kh::set_pending_query_hook([m, sp]() {ProfScope prof(m, 5); update_scan(*sp, m->laser);});
    std::vector<kh_scan> base;
    // (uploads of scans not yet resident go in front of the match on the matcher's own stream; the match returns after its
    // last kernel, so every other reader finds them in place)
    void * seq_stream = kh_matcher_stream(m->seq);
    for (int32_t r : m->running) {base.push_back(as_base_scan(m, *m->scans[r], seq_stream));}
    double mean[3], response = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = kh_matcher_match(m->seq, &q, base.data(), static_cast<int32_t>(base.size()), 1, 1, mean, cov, &response);
    kh::run_pending_query_hook();             // (an argument check that refused the call before the hook was taken)
    m->stats.match_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    m->stats.matches += 1;
    if (rc) {
      // an early return of the match (invalid argument, empty query, a HIP error) may leave the uploads queued above in flight:
      // wait for them, so that no other stream reads a copy marked fresh while it is still arriving
      kh::stream_synchronize(seq_stream);
      return rc;
    }
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
    set_sensor_pose(m, *scan, mean);
  }
  // pScan->SetOdometricPose(pScan->GetCorrectedPose()) (:2792, 3065): the next scan's odometry delta is measured from here
  if (!gated) {scan->odometric = scan->corrected;}
  // AddScan: state id = unique id = position in the list (:2727)
  const int32_t id = static_cast<int32_t>(m->scans.size());
  scan->id = id;
  m->scans.push_back(std::move(scan));
  m->adj.emplace_back(); m->out_edges.emplace_back();
  // from here on the scan is part of the mapper: an error return leaves the handle marked failed
  struct CommitGuard {kh_mapper * m; bool armed; ~CommitGuard() {if (armed) {m->failed = true;}}} guard{m, true};
  if (!m->graph_dirty) {
    double xy[2];
    reference_xy(m, *m->scans[id], xy);
    m->compact_of.push_back(static_cast<int32_t>(m->alive.size()));
    m->alive.push_back(id);
    const double pose_xy[2] = {m->scans[id]->corrected.x, m->scans[id]->corrected.y};
    if (kh_graph_append_scan_with_pose(m->graph, xy, pose_xy) != KH_OK) {m->graph_dirty = true;}
    // the scan map's size in id space bounds the candidate walks (see sync_graph)
    const int32_t n_alive = static_cast<int32_t>(m->alive.size());
    const int32_t n_visit = static_cast<int32_t>(std::lower_bound(m->alive.begin(), m->alive.end(), n_alive) - m->alive.begin());
    if (!m->graph_dirty && kh_graph_set_scan_limit(m->graph, n_visit) != KH_OK) {m->graph_dirty = true;}
  }
  MScan & s = *m->scans[id];
  if (m->p.use_scan_matching) {
    // AddVertex (:1418-1432): the solver node carries the corrected pose
    const double node[3] = {s.corrected.x, s.corrected.y, s.corrected.h};
    if (m->log) {std::fprintf(m->log, "N %d %.17g %.17g %.17g\n", id, node[0], node[1], node[2]);}
    int rc;
    {ProfScope prof(m, 6); rc = kh_spa_add_node(m->solver, id, node);}
    if (rc) {return rc;}
    // AddEdges (:1434-1498)
    std::vector<double> means, covs;
    const bool previous_gone = last && !m->scans[id - 1];       // AddEdges returns at once (Mapper.cpp:1444-1447)
    if (last && !previous_gone) {
      const Pose sp = s.sensor_pose();
      const double scan_pose[3] = {sp.x, sp.y, sp.h};
      rc = link_scans(m, id - 1, id, scan_pose, cov); if (rc) {return rc;}
      means.insert(means.end(), scan_pose, scan_pose + 3);
      covs.insert(covs.end(), cov, cov + 9);
      rc = link_chain_to_scan(m, m->running, id, scan_pose, cov); if (rc) {return rc;}
    }
    // LinkNearChains (:1641-1663): the near chains are independent matches of the same scan -> one batch
    if (!previous_gone) {
      if (m->graph_dirty) {rc = sync_graph(m); if (rc) {return rc;}}
      std::vector<int32_t> flat(2 * static_cast<size_t>(m->max_candidates));
      int32_t n_chains = 0;
      const int32_t query = m->compact_of[id];
      {ProfScope prof(m, 8);
      rc = kh_graph_find_near_chains(m->graph, query, m->p.link_scan_maximum_distance, flat.data(), m->max_candidates, &n_chains);
      }
      if (rc) {return rc;}
      if (n_chains > m->max_candidates) {
        flat.resize(2 * static_cast<size_t>(n_chains));
        rc = kh_graph_find_near_chains(m->graph, query, m->p.link_scan_maximum_distance, flat.data(), n_chains, &n_chains);
        if (rc) {return rc;}
      }
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
    }
    if (!means.empty()) {
      double wm[3];
      rc = kh_weighted_mean(static_cast<int32_t>(means.size() / 3), means.data(), covs.data(), wm); if (rc) {return rc;}
      set_sensor_pose(m, s, wm);
    }
    // AddRunningScan (:183-206)
    m->running.push_back(id);
    {
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
    if (m->p.do_loop_closing) {
      bool closed = false;
      rc = kh::try_close_loop(m, id, closed);
      if (rc) {return rc;}
    }
  }
  m->last = id;
  if (m->lifelong && m->p.use_scan_matching) {
    const int rc = kh::lifelong_step(m, id);
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
  if (corrected_pose) {corrected_pose[0] = s.corrected.x; corrected_pose[1] = s.corrected.y; corrected_pose[2] = s.corrected.h;}
  if (covariance) {std::copy(cov, cov + 9, covariance);}
  m->stats.scans_processed += 1;
  m->stats.process_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return KH_OK;
}
}  // namespace
}  // namespace kh

extern "C" {

// Mapper::Process (Mapper.cpp:2679-2748)
int kh_mapper_process(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time, int32_t * accepted,
  double corrected_pose[3], double covariance[9])
{
  return kh::process_scan(m, kh::Entry::kProcess, -1, false, ranges, odometric_pose, time, accepted, corrected_pose, covariance);
}

// Mapper::ProcessLocalization (Mapper.cpp:2831-2909)
int kh_mapper_process_localization(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time, int32_t * accepted,
  double corrected_pose[3], double covariance[9])
{
  return kh::process_scan(m, kh::Entry::kLocalization, -1, true, ranges, odometric_pose, time, accepted, corrected_pose, covariance);
}

// Mapper::ProcessAgainstNode (Mapper.cpp:3023-3096); ProcessAtDock (:3098-3102) is node 0
int kh_mapper_process_against_node(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time, int32_t node_id,
  int32_t * accepted, double corrected_pose[3], double covariance[9])
{
  return kh::process_scan(m, kh::Entry::kAgainstNode, node_id, false, ranges, odometric_pose, time, accepted, corrected_pose, covariance);
}

// Mapper::ProcessAgainstNodesNearBy (Mapper.cpp:2751-2829)
int kh_mapper_process_against_nodes_near_by(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time,
  int32_t add_to_localization_buffer, int32_t * accepted, double corrected_pose[3], double covariance[9])
{
  return kh::process_scan(m, kh::Entry::kNearBy, -1, add_to_localization_buffer != 0, ranges, odometric_pose, time, accepted, corrected_pose,
           covariance);
}

// Mapper::ClearLocalizationBuffer (Mapper.cpp:2939-2962)
int kh_mapper_clear_localization_buffer(kh_mapper * m)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  while (!m->loc_buffer.empty()) {
    const int rc = kh::evict_front(m);
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
    corrected_poses[3 * i] = m->scans[i]->corrected.x; corrected_poses[3 * i + 1] = m->scans[i]->corrected.y;
    corrected_poses[3 * i + 2] = m->scans[i]->corrected.h;
  }
  return KH_OK;
}

int kh_mapper_get_scan(const kh_mapper * m, int32_t index, kh_scan * scan, kh_scan_box * box)
{
  if (!m || index < 0 || index >= static_cast<int32_t>(m->scans.size()) || !m->scans[index]) {return KH_ERR_NOT_FOUND;}
  const MScan & s = *m->scans[index];
  if (scan) {*scan = kh::as_kh_scan(s);}
  if (box) {*box = kh::box_of(m, s);}
  return KH_OK;
}

int kh_mapper_get_adjacency(const kh_mapper * m, int32_t scan_id, int32_t * adjacent, int32_t capacity, int32_t * n)
{
  if (!m || !n || scan_id < 0 || scan_id >= static_cast<int32_t>(m->scans.size()) || !m->scans[scan_id]) {return KH_ERR_NOT_FOUND;}
  const std::vector<int32_t> & a = m->adj[scan_id];
  *n = static_cast<int32_t>(a.size());
  if (adjacent) {std::copy(a.begin(), a.begin() + std::min<size_t>(a.size(), static_cast<size_t>(std::max(capacity, 0))), adjacent);}
  return KH_OK;
}

int kh_mapper_set_node_score(kh_mapper * m, int32_t scan_id, double score)
{
  if (!m || scan_id < 0 || scan_id >= static_cast<int32_t>(m->scans.size()) || !m->scans[scan_id]) {return KH_ERR_NOT_FOUND;}
  m->scans[scan_id]->score = score;
  return KH_OK;
}

int kh_mapper_remove_node(kh_mapper * m, int32_t scan_id)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  // The next Process() reads the last scan and every scan of the running window; the reference (GetLastScan /
  // GetRunningScans hold raw pointers, Mapper.cpp:2688, 2716) would be left with dangling ones, and its only caller --
  // the lifelong policy, which skips the newest scan_buffer_size scans -- never asks for this.  Refused here.
  if (scan_id == m->last || std::find(m->running.begin(), m->running.end(), scan_id) != m->running.end()) {
    kh::set_error("RemoveNode: the scan is the last scan or in the running-scan window");
    return KH_ERR_INVALID_ARG;
  }
  return kh::remove_node(m, scan_id);
}

int kh_mapper_marginalize_nodes(kh_mapper * m, int32_t n, const int32_t * scan_ids)
{
  if (n < 0 || (n > 0 && !scan_ids)) {return KH_ERR_INVALID_ARG;}
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  for (int32_t k = 0; k < n; ++k) {                     // as kh_mapper_remove_node: the next Process() reads these scans
    if (scan_ids[k] == m->last || std::find(m->running.begin(), m->running.end(), scan_ids[k]) != m->running.end()) {
      kh::set_error("MarginalizeNodes: a scan is the last scan or in the running-scan window");
      return KH_ERR_INVALID_ARG;
    }
  }
  return kh::marginalize_nodes(m, n, scan_ids);
}

int kh_mapper_set_removal_mode(kh_mapper * m, int32_t mode)
{
  if (!m || (mode != KH_REMOVE_PLAIN && mode != KH_REMOVE_MARGINALIZE)) {return KH_ERR_INVALID_ARG;}
  m->removal_mode = mode;
  return KH_OK;
}

// ---- single-edge edits, the constraint audit and the rejection loop ----
static bool scan_alive(const kh_mapper * m, int32_t id) {return id >= 0 && id < static_cast<int32_t>(m->scans.size()) && m->scans[id];}

int kh_mapper_correct_poses(kh_mapper * m)
{
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  const int rc = kh::correct_poses(m);
  m->gate_due = true;                                // the poses may have moved: the gate's covariances are no longer theirs
  return rc;
}

int kh_mapper_add_edge(kh_mapper * m, int32_t from, int32_t to, const double mean_sensor_pose[3], const double cov[9], int32_t correct)
{
  if (!mean_sensor_pose || !cov) {return KH_ERR_INVALID_ARG;}
  for (int k = 0; k < 3; ++k) {if (!std::isfinite(mean_sensor_pose[k])) {return KH_ERR_INVALID_ARG;}}
  for (int k = 0; k < 9; ++k) {if (!std::isfinite(cov[k])) {return KH_ERR_INVALID_ARG;}}
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (!scan_alive(m, from) || !scan_alive(m, to) || from == to) {
    kh::set_error("AddEdge: Failed to find the two scans");
    return KH_ERR_NOT_FOUND;
  }
  int rc = kh::link_scans(m, from, to, mean_sensor_pose, cov);
  if (rc) {return rc;}
  m->gate_due = true;
  return correct ? kh_mapper_correct_poses(m) : KH_OK;
}

int kh_mapper_remove_edge(kh_mapper * m, int32_t from, int32_t to)
{
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (!scan_alive(m, from) || !scan_alive(m, to)) {kh::set_error("RemoveEdge: Failed to find the two scans"); return KH_ERR_NOT_FOUND;}
  const auto out = std::find(m->out_edges[from].begin(), m->out_edges[from].end(), to);
  const auto af = std::find(m->adj[from].begin(), m->adj[from].end(), to);
  const auto at = std::find(m->adj[to].begin(), m->adj[to].end(), from);
  if (out == m->out_edges[from].end() || af == m->adj[from].end() || at == m->adj[to].end()) {
    kh::set_error("RemoveEdge: no edge with that source and target");
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
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  const int32_t nc = kh_spa_num_constraints(m->solver);
  *n = nc;
  if (nc > cap) {kh::set_error("kh_mapper_audit: the capacity is below the number of constraints"); return KH_ERR_INVALID_ARG;}
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
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  const auto t_begin = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
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
      kh::set_error("kh_mapper_reject_outliers: more removals than `removed` holds");
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
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
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

int kh_mapper_set_lifelong(kh_mapper * m, const kh_decay_params * params)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  m->lifelong = params != nullptr;
  if (params) {m->decay = *params; m->decay.scan_buffer_size = m->p.scan_buffer_size;}
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

}  // extern "C"

// ---- mapping sessions (slam_toolbox's serializePoseGraph / deserializePoseGraph + loadSerializedPoseGraph, slam_toolbox_common.cpp:952-1017) ----
// The file is the library's own format (DESIGN.md section 7 has it byte by byte):
//   header   "KHMS", u32 version, u64 file size, u32 section count, u32 CRC-32 (IEEE, as zlib's) of everything behind the header
//   table    per section: 4-byte tag, u32 0, u64 offset, u64 size; the sections follow in table order, each a multiple of 8 bytes
//   PARM LASR LIFE STAT RUNB SCAN RNGS ADJL SNOD SCON SANA
// All integers and doubles little endian.  Parsing never trusts a count: every section's size is recomputed from the counts of
// STAT / its own head in 128-bit arithmetic and compared with the table before anything is read through it.
namespace kh
{
namespace
{
static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the session file is written by memcpy: little-endian hosts only");
constexpr uint32_t kSessionVersion = 1;
constexpr int kSections = 11;
const char kSectionTags[kSections][5] = {"PARM", "LASR", "LIFE", "STAT", "RUNB", "SCAN", "RNGS", "ADJL", "SNOD", "SCON", "SANA"};
constexpr size_t kHeaderBytes = 24, kTableBytes = 24 * kSections;
double g_last_load_ms[4] = {0.0, 0.0, 0.0, 0.0};      // kh_session_last_load_ms

uint32_t crc32_ieee(const uint8_t * p, size_t n)
{
  static const std::vector<uint32_t> table = [] {
      std::vector<uint32_t> t(256);
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) {c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;}
        t[i] = c;
      }
      return t;
    }();
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);}
  return c ^ 0xFFFFFFFFu;
}

// kh_mapper_params as 29 words of 8 bytes in declaration order: the int32 fields as int64, the doubles as they are
#define KH_SESSION_PARAM_WORDS(I, D)                                                                                              \
  I(use_scan_matching) I(use_scan_barycenter) D(minimum_time_interval) D(minimum_travel_distance) D(minimum_travel_heading)      \
  I(scan_buffer_size) D(scan_buffer_maximum_scan_distance) D(link_match_minimum_response_fine) D(link_scan_maximum_distance)     \
  D(loop_search_maximum_distance) I(do_loop_closing) I(loop_match_minimum_chain_size) D(loop_match_maximum_variance_coarse)      \
  D(loop_match_minimum_response_coarse) D(loop_match_minimum_response_fine) D(correlation_search_space_dimension)                \
  D(correlation_search_space_resolution) D(correlation_search_space_smear_deviation) D(loop_search_space_dimension)              \
  D(loop_search_space_resolution) D(loop_search_space_smear_deviation) D(match.coarse_search_angle_offset)                       \
  D(match.coarse_angle_resolution) D(match.fine_search_angle_offset) I(match.use_response_expansion)                             \
  D(match.distance_variance_penalty) D(match.minimum_distance_penalty) D(match.angle_variance_penalty) D(match.minimum_angle_penalty)
constexpr size_t kParamWords = 29, kLaserWords = 9, kLifeWords = 9, kStatWords = 6;

struct Blob
{
  std::string b;
  void raw(const void * p, size_t n) {b.append(static_cast<const char *>(p), n);}
  void i64(int64_t v) {raw(&v, 8);}
  void f64(double v) {raw(&v, 8);}
  void i32s(const std::vector<int32_t> & v) {if (!v.empty()) {raw(v.data(), 4 * v.size());}}
  void pad8() {while (b.size() % 8) {b.push_back('\0');}}
};

// what a session file holds, as parsed (and as kh_mapper_load puts it into a mapper)
struct Session
{
  kh_mapper_params p; kh_laser laser; int64_t lifelong = 0; kh_decay_params decay;
  int64_t n_slots = 0, n_alive = 0, n_edges = 0, last = -1, n_running = 0, n_loc = 0;
  std::vector<int32_t> running, loc;
  std::vector<int32_t> ids; std::vector<double> time, odom, corr, score, ranges;
  std::vector<int32_t> adj_count, out_count, adj, out;
  int64_t n_nodes = 0, words[7] = {0, 0, 0, 0, 0, 0, 0};
  std::vector<int32_t> node_ids; std::vector<double> node_poses;
  int64_t n_cons = 0;
  std::vector<int32_t> ca, cb; std::vector<double> cz, cinfo;
  int64_t n_sn = 0;
  std::vector<int32_t> sn_ptr, sn_ids;
  int64_t version = 0, file_bytes = 0;
};

bool read_file(const char * path, std::string & out)
{
  FILE * f = std::fopen(path, "rb");
  if (!f) {return false;}
  char buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) {out.append(buf, n);}
  const bool ok = !std::ferror(f);
  std::fclose(f);
  return ok;
}

int bad_file(const std::string & why)
{
  set_error("session file: " + why);
  return KH_ERR_IO;
}

typedef unsigned __int128 u128;
inline uint64_t round8(uint64_t v) {return (v + 7) & ~static_cast<uint64_t>(7);}

// bounds-checked cursor over one section
struct Cursor
{
  const uint8_t * p; size_t left;
  bool take(void * dst, size_t n) {if (n > left) {return false;} if (n) {std::memcpy(dst, p, n);} p += n; left -= n; return true;}
  bool skip(size_t n) {if (n > left) {return false;} p += n; left -= n; return true;}
  template <class T> bool vec(std::vector<T> & v, uint64_t count)
  {
    if (static_cast<u128>(count) * sizeof(T) > left) {return false;}
    v.resize(static_cast<size_t>(count));
    return take(v.data(), static_cast<size_t>(count) * sizeof(T));
  }
};

// header, table, checksum, every section's size against its counts, and every id against the lists it indexes
int parse_session(const std::string & data, Session & S)
{
  const uint8_t * base = reinterpret_cast<const uint8_t *>(data.data());
  const uint64_t size = data.size();
  if (size < kHeaderBytes) {return bad_file("truncated inside the header");}
  if (std::memcmp(base, "KHMS", 4) != 0) {return bad_file("wrong magic (not a mapping session)");}
  uint32_t version, n_sections, crc; uint64_t file_size;
  std::memcpy(&version, base + 4, 4); std::memcpy(&file_size, base + 8, 8); std::memcpy(&n_sections, base + 16, 4); std::memcpy(&crc, base + 20, 4);
  if (version != kSessionVersion) {return bad_file("unknown version " + std::to_string(version));}
  if (file_size != size) {return bad_file("truncated: the header says " + std::to_string(file_size) + " bytes, the file has " + std::to_string(size));}
  if (n_sections != kSections || size < kHeaderBytes + kTableBytes) {return bad_file("section table does not fit");}
  if (crc32_ieee(base + kHeaderBytes, static_cast<size_t>(size - kHeaderBytes)) != crc) {return bad_file("checksum mismatch");}
  uint64_t off[kSections], len[kSections], at = kHeaderBytes + kTableBytes;
  for (int k = 0; k < kSections; ++k) {
    const uint8_t * e = base + kHeaderBytes + 24 * k;
    uint32_t zero;
    std::memcpy(&zero, e + 4, 4); std::memcpy(&off[k], e + 8, 8); std::memcpy(&len[k], e + 16, 8);
    if (std::memcmp(e, kSectionTags[k], 4) != 0 || zero != 0) {return bad_file("section table: unexpected tag");}
    if (off[k] != at || (len[k] & 7) || len[k] > size - at) {return bad_file(std::string("section ") + kSectionTags[k] + " does not fit the file");}
    at += len[k];
  }
  if (at != size) {return bad_file("bytes behind the last section");}
  S.version = version; S.file_bytes = static_cast<int64_t>(size);
  auto cursor = [&](int k) {return Cursor{base + off[k], static_cast<size_t>(len[k])};};
  auto misfit = [&](int k) {return bad_file(std::string("counts do not fit section ") + kSectionTags[k]);};
  // PARM, LASR, LIFE, STAT: fixed size
  if (len[0] != 8 * kParamWords || len[1] != 8 * kLaserWords || len[2] != 8 * kLifeWords || len[3] != 8 * kStatWords) {return misfit(0);}
  {
    Cursor c = cursor(0);
    int64_t iv;
#define KH_RD_I(f) c.take(&iv, 8); S.p.f = static_cast<int32_t>(iv);
#define KH_RD_D(f) c.take(&S.p.f, 8);
    KH_SESSION_PARAM_WORDS(KH_RD_I, KH_RD_D)
#undef KH_RD_I
#undef KH_RD_D
    c = cursor(1);
    c.take(&iv, 8);
    if (iv < 1 || iv > (1 << 20)) {return bad_file("laser: beam count out of range");}
    S.laser.n_beams = static_cast<int32_t>(iv);
    c.take(&S.laser.minimum_angle, 8); c.take(&S.laser.angular_resolution, 8); c.take(&S.laser.minimum_range, 8); c.take(&S.laser.maximum_range, 8);
    c.take(&S.laser.range_threshold, 8); c.take(&S.laser.offset_x, 8); c.take(&S.laser.offset_y, 8); c.take(&S.laser.offset_heading, 8);
    c = cursor(2);
    c.take(&S.lifelong, 8);
    c.take(&S.decay.iou_thresh, 8); c.take(&S.decay.iou_match, 8); c.take(&S.decay.removal_score, 8); c.take(&S.decay.overlap_scale, 8);
    c.take(&S.decay.constraint_scale, 8); c.take(&S.decay.nearby_penalty, 8); c.take(&S.decay.candidates_scale, 8);
    c.take(&iv, 8); S.decay.scan_buffer_size = static_cast<int32_t>(iv);
    c = cursor(3);
    c.take(&S.n_slots, 8); c.take(&S.n_alive, 8); c.take(&S.n_edges, 8); c.take(&S.last, 8); c.take(&S.n_running, 8); c.take(&S.n_loc, 8);
  }
  const int64_t nb = S.laser.n_beams;
  if (S.n_slots < 0 || S.n_slots > INT32_MAX || S.n_alive < 0 || S.n_alive > S.n_slots || S.n_edges < 0 || S.last < -1 || S.last >= S.n_slots ||
    S.n_running < 0 || S.n_running > S.n_alive || S.n_loc < 0 || S.n_loc > S.n_alive) {return bad_file("scan counts out of range");}
  // RUNB: running[n_running], loc[n_loc] (int32), padded
  if (len[4] != round8(4 * static_cast<uint64_t>(S.n_running + S.n_loc))) {return misfit(4);}
  {Cursor c = cursor(4); if (!c.vec(S.running, S.n_running) || !c.vec(S.loc, S.n_loc)) {return misfit(4);}}
  // SCAN: per scan alive, ascending id: i32 id, i32 0, f64 time, odometric pose, corrected pose, score = 72 bytes
  if (static_cast<u128>(S.n_alive) * 72 != len[5]) {return misfit(5);}
  if (static_cast<u128>(S.n_alive) * static_cast<u128>(nb) * 8 != len[6]) {return misfit(6);}
  {
    Cursor c = cursor(5);
    const size_t n = static_cast<size_t>(S.n_alive);
    S.ids.resize(n); S.time.resize(n); S.odom.resize(3 * n); S.corr.resize(3 * n); S.score.resize(n);
    for (size_t k = 0; k < n; ++k) {
      int32_t zero = 0;
      if (!c.take(&S.ids[k], 4) || !c.take(&zero, 4) || !c.take(&S.time[k], 8) || !c.take(&S.odom[3 * k], 24) || !c.take(&S.corr[3 * k], 24) ||
        !c.take(&S.score[k], 8)) {return misfit(5);}
      if (S.ids[k] < 0 || S.ids[k] >= S.n_slots || (k > 0 && S.ids[k] <= S.ids[k - 1])) {return bad_file("scan ids are not ascending ids below the slot count");}
    }
    c = cursor(6);
    if (!c.vec(S.ranges, static_cast<uint64_t>(S.n_alive) * static_cast<uint64_t>(nb))) {return misfit(6);}
  }
  std::vector<uint8_t> is_alive(static_cast<size_t>(S.n_slots), 0);
  for (int32_t id : S.ids) {is_alive[id] = 1;}
  auto alive_id = [&](int64_t id) {return id >= 0 && id < S.n_slots && is_alive[static_cast<size_t>(id)];};
  if (S.last >= 0 && !alive_id(S.last)) {return bad_file("the last scan is not in the map");}
  for (int32_t r : S.running) {if (!alive_id(r)) {return bad_file("a running scan is not in the map");}}
  for (int32_t r : S.loc) {if (!alive_id(r)) {return bad_file("a buffered scan is not in the map");}}
  // ADJL: adj_count[n_slots], out_count[n_slots], adj[], out[] (int32), padded
  {
    if (static_cast<u128>(S.n_slots) * 8 > len[7]) {return misfit(7);}
    Cursor c = cursor(7);
    if (!c.vec(S.adj_count, S.n_slots) || !c.vec(S.out_count, S.n_slots)) {return misfit(7);}
    u128 n_adj = 0, n_out = 0;
    for (int64_t i = 0; i < S.n_slots; ++i) {
      if (S.adj_count[i] < 0 || S.out_count[i] < 0 || (!is_alive[i] && (S.adj_count[i] || S.out_count[i]))) {return bad_file("adjacency counts of a removed scan");}
      n_adj += static_cast<uint32_t>(S.adj_count[i]); n_out += static_cast<uint32_t>(S.out_count[i]);
    }
    if (round8(static_cast<uint64_t>((static_cast<u128>(S.n_slots) * 2 + n_adj + n_out) * 4)) != len[7] || (static_cast<u128>(S.n_slots) * 2 + n_adj + n_out) * 4 > len[7]) {
      return misfit(7);
    }
    if (!c.vec(S.adj, static_cast<uint64_t>(n_adj)) || !c.vec(S.out, static_cast<uint64_t>(n_out))) {return misfit(7);}
    for (int32_t a : S.adj) {if (!alive_id(a)) {return bad_file("an adjacent scan is not in the map");}}
    for (int32_t a : S.out) {if (!alive_id(a)) {return bad_file("an edge target is not in the map");}}
  }
  // SNOD: i64 n, 7 words of gauge + analysis cache, i32 id[n] padded, f64 pose[3n]
  {
    Cursor c = cursor(8);
    if (!c.take(&S.n_nodes, 8) || !c.take(S.words, 56)) {return misfit(8);}
    if (S.n_nodes < 0 || static_cast<u128>(64) + round8(4 * static_cast<uint64_t>(std::min<int64_t>(S.n_nodes, INT32_MAX))) + static_cast<u128>(S.n_nodes) * 24 != len[8] ||
      S.n_nodes > INT32_MAX) {return misfit(8);}
    if (!c.vec(S.node_ids, S.n_nodes) || !c.skip(static_cast<size_t>(round8(4 * S.n_nodes) - 4 * S.n_nodes)) || !c.vec(S.node_poses, 3 * static_cast<uint64_t>(S.n_nodes))) {return misfit(8);}
  }
  std::vector<int32_t> sorted_nodes = S.node_ids;
  std::sort(sorted_nodes.begin(), sorted_nodes.end());
  if (std::adjacent_find(sorted_nodes.begin(), sorted_nodes.end()) != sorted_nodes.end()) {return bad_file("duplicate solver node");}
  auto known_node = [&](int32_t id) {return std::binary_search(sorted_nodes.begin(), sorted_nodes.end(), id);};
  // SCON: i64 m, i32 a[m], i32 b[m], f64 z[3m], f64 info[6m]
  {
    Cursor c = cursor(9);
    if (!c.take(&S.n_cons, 8)) {return misfit(9);}
    if (S.n_cons < 0 || S.n_cons > INT32_MAX || static_cast<u128>(8) + static_cast<u128>(S.n_cons) * (8 + 24 + 48) != len[9]) {return misfit(9);}
    if (!c.vec(S.ca, S.n_cons) || !c.vec(S.cb, S.n_cons) || !c.vec(S.cz, 3 * static_cast<uint64_t>(S.n_cons)) || !c.vec(S.cinfo, 6 * static_cast<uint64_t>(S.n_cons))) {return misfit(9);}
    for (int64_t k = 0; k < S.n_cons; ++k) {
      if (S.ca[k] == S.cb[k] || !known_node(S.ca[k]) || !known_node(S.cb[k])) {return bad_file("a constraint between unknown solver nodes");}
    }
  }
  // SANA: i64 n_supernodes, i32 ptr[n + 1], i32 ids[ptr[n]], padded
  {
    Cursor c = cursor(10);
    if (!c.take(&S.n_sn, 8)) {return misfit(10);}
    if (S.n_sn < 0 || static_cast<u128>(S.n_sn) * 4 + 12 > len[10]) {return misfit(10);}
    if (!c.vec(S.sn_ptr, static_cast<uint64_t>(S.n_sn) + 1)) {return misfit(10);}
    if (S.sn_ptr[0] != 0) {return misfit(10);}
    for (int64_t k = 0; k < S.n_sn; ++k) {if (S.sn_ptr[k + 1] < S.sn_ptr[k]) {return misfit(10);}}
    const uint64_t total = static_cast<uint64_t>(S.sn_ptr[static_cast<size_t>(S.n_sn)]);
    if (round8(8 + 4 * (static_cast<uint64_t>(S.n_sn) + 1 + total)) != len[10]) {return misfit(10);}
    if (!c.vec(S.sn_ids, total)) {return misfit(10);}
  }
  return KH_OK;
}

int load_and_parse(const char * path, Session & S)
{
  std::string data;
  if (!read_file(path, data)) {return bad_file(std::string("cannot read ") + path);}
  return parse_session(data, S);
}
}  // namespace
}  // namespace kh

extern "C" {

int kh_mapper_save(const kh_mapper * m, const char * path)
{
  if (!m || !path) {return KH_ERR_INVALID_ARG;}
  if (m->failed) {
    kh::set_error("kh_mapper_save: an earlier Process() failed after its scan had entered the graph; the state is not a run's state");
    return KH_ERR_INVALID_ARG;
  }
  kh::Blob sec[kh::kSections];
  {
    const kh_mapper_params & p = m->p;
#define KH_WR_I(f) sec[0].i64(p.f);
#define KH_WR_D(f) sec[0].f64(p.f);
    KH_SESSION_PARAM_WORDS(KH_WR_I, KH_WR_D)
#undef KH_WR_I
#undef KH_WR_D
  }
  const Laser & L = m->laser;
  sec[1].i64(L.n); sec[1].f64(L.min_angle); sec[1].f64(L.ang_res); sec[1].f64(L.min_range); sec[1].f64(L.max_range); sec[1].f64(L.range_threshold);
  sec[1].f64(L.offset.x); sec[1].f64(L.offset.y); sec[1].f64(L.offset.h);
  kh_decay_params d;
  std::memset(&d, 0, sizeof(d));
  if (m->lifelong) {d = m->decay;}
  sec[2].i64(m->lifelong ? 1 : 0);
  sec[2].f64(d.iou_thresh); sec[2].f64(d.iou_match); sec[2].f64(d.removal_score); sec[2].f64(d.overlap_scale); sec[2].f64(d.constraint_scale);
  sec[2].f64(d.nearby_penalty); sec[2].f64(d.candidates_scale); sec[2].i64(d.scan_buffer_size);
  int64_t n_alive = 0;
  for (const auto & s : m->scans) {n_alive += s ? 1 : 0;}
  sec[3].i64(static_cast<int64_t>(m->scans.size())); sec[3].i64(n_alive); sec[3].i64(m->n_edges); sec[3].i64(m->last);
  sec[3].i64(static_cast<int64_t>(m->running.size())); sec[3].i64(static_cast<int64_t>(m->loc_buffer.size()));
  sec[4].i32s(m->running); sec[4].i32s(m->loc_buffer); sec[4].pad8();
  sec[5].b.reserve(static_cast<size_t>(n_alive) * 72); sec[6].b.reserve(static_cast<size_t>(n_alive) * 8 * static_cast<size_t>(L.n));
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    const MScan & s = *sp;
    const int32_t head[2] = {s.id, 0};
    sec[5].raw(head, 8); sec[5].f64(s.time);
    sec[5].f64(s.odometric.x); sec[5].f64(s.odometric.y); sec[5].f64(s.odometric.h);
    sec[5].f64(s.corrected.x); sec[5].f64(s.corrected.y); sec[5].f64(s.corrected.h);
    sec[5].f64(s.score);
    sec[6].raw(s.ranges.data(), 8 * s.ranges.size());
  }
  {
    std::vector<int32_t> counts;
    for (const auto & a : m->adj) {counts.push_back(static_cast<int32_t>(a.size()));}
    sec[7].i32s(counts);
    counts.clear();
    for (const auto & a : m->out_edges) {counts.push_back(static_cast<int32_t>(a.size()));}
    sec[7].i32s(counts);
    for (const auto & a : m->adj) {sec[7].i32s(a);}
    for (const auto & a : m->out_edges) {sec[7].i32s(a);}
    sec[7].pad8();
  }
  {
    int64_t words[7];
    std::vector<int32_t> sn_ptr, sn_ids;
    kh::spa_export_session_state(m->solver, words, sn_ptr, sn_ids);
    const int32_t n = kh_spa_num_nodes(m->solver), nc = kh_spa_num_constraints(m->solver);
    std::vector<int32_t> ids(static_cast<size_t>(n));
    std::vector<double> poses(3 * static_cast<size_t>(n));
    if (n) {kh_spa_get_nodes(m->solver, ids.data(), poses.data());}
    sec[8].i64(n); sec[8].raw(words, 56); sec[8].i32s(ids); sec[8].pad8();
    if (n) {sec[8].raw(poses.data(), 8 * poses.size());}
    std::vector<int32_t> ca(static_cast<size_t>(nc)), cb(static_cast<size_t>(nc));
    std::vector<double> cz(3 * static_cast<size_t>(nc)), ci(6 * static_cast<size_t>(nc));
    for (int32_t k = 0; k < nc; ++k) {
      const int rc = kh_spa_get_constraint(m->solver, k, &ca[k], &cb[k], &cz[3 * k], &ci[6 * k]);
      if (rc) {return rc;}
    }
    sec[9].i64(nc); sec[9].i32s(ca); sec[9].i32s(cb);
    if (nc) {sec[9].raw(cz.data(), 8 * cz.size()); sec[9].raw(ci.data(), 8 * ci.size());}
    sec[10].i64(static_cast<int64_t>(sn_ptr.size()) - 1); sec[10].i32s(sn_ptr); sec[10].i32s(sn_ids); sec[10].pad8();
  }
  std::string body;                                  // section table + sections = what the checksum covers
  uint64_t at = kh::kHeaderBytes + kh::kTableBytes;
  for (int k = 0; k < kh::kSections; ++k) {
    const uint32_t zero = 0;
    const uint64_t len = sec[k].b.size();
    body.append(kh::kSectionTags[k], 4); body.append(reinterpret_cast<const char *>(&zero), 4);
    body.append(reinterpret_cast<const char *>(&at), 8); body.append(reinterpret_cast<const char *>(&len), 8);
    at += len;
  }
  for (int k = 0; k < kh::kSections; ++k) {body += sec[k].b; sec[k].b.clear(); sec[k].b.shrink_to_fit();}
  const uint32_t version = kh::kSessionVersion, n_sections = kh::kSections;
  const uint32_t crc = kh::crc32_ieee(reinterpret_cast<const uint8_t *>(body.data()), body.size());
  FILE * f = std::fopen(path, "wb");
  if (!f) {kh::set_error("kh_mapper_save: cannot open the file for writing"); return KH_ERR_IO;}
  bool ok = std::fwrite("KHMS", 1, 4, f) == 4 && std::fwrite(&version, 4, 1, f) == 1 && std::fwrite(&at, 8, 1, f) == 1 &&
    std::fwrite(&n_sections, 4, 1, f) == 1 && std::fwrite(&crc, 4, 1, f) == 1 && std::fwrite(body.data(), 1, body.size(), f) == body.size();
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) {kh::set_error("kh_mapper_save: write failed"); return KH_ERR_IO;}
  return KH_OK;
}

int kh_session_info(const char * path, kh_session_info_t * out)
{
  if (!path || !out) {return KH_ERR_INVALID_ARG;}
  kh::Session S;
  const int rc = kh::load_and_parse(path, S);
  if (rc) {return rc;}
  out->version = S.version; out->file_bytes = S.file_bytes; out->n_beams = S.laser.n_beams; out->n_scan_slots = S.n_slots; out->n_alive = S.n_alive;
  out->n_edges = S.n_edges; out->n_running = S.n_running; out->last_scan = S.last; out->n_localization_buffer = S.n_loc; out->lifelong = S.lifelong;
  out->n_solver_nodes = S.n_nodes; out->n_solver_constraints = S.n_cons; out->n_supernodes = S.n_sn;
  return KH_OK;
}

int kh_mapper_load(const char * path, const int32_t * devices, int32_t n_devices, int32_t max_candidates, kh_mapper ** out)
{
  if (!path || !out || !devices || n_devices < 1 || max_candidates < 1) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  kh::Session S;
  int rc = kh::load_and_parse(path, S);                 // the whole file is validated before a device is touched
  if (rc) {return rc;}
  const auto t1 = std::chrono::steady_clock::now();
  kh_mapper * m = nullptr;
  rc = kh_mapper_create_on_devices(&S.p, &S.laser, devices, n_devices, max_candidates, &m);
  if (rc) {return rc;}
  auto fail = [&](int code) {kh_mapper_destroy(m); return code;};
  if (S.lifelong) {m->lifelong = true; m->decay = S.decay;}
  const size_t nb = static_cast<size_t>(S.laser.n_beams);
  m->scans.resize(static_cast<size_t>(S.n_slots));
  for (size_t k = 0; k < S.ids.size(); ++k) {
    std::unique_ptr<MScan> s(new MScan());
    s->id = S.ids[k]; s->time = S.time[k]; s->score = S.score[k];
    s->odometric.x = S.odom[3 * k]; s->odometric.y = S.odom[3 * k + 1]; s->odometric.h = S.odom[3 * k + 2];
    s->corrected.x = S.corr[3 * k]; s->corrected.y = S.corr[3 * k + 1]; s->corrected.h = S.corr[3 * k + 2];
    s->ranges.assign(S.ranges.begin() + static_cast<std::ptrdiff_t>(k * nb), S.ranges.begin() + static_cast<std::ptrdiff_t>((k + 1) * nb));
    m->scans[static_cast<size_t>(S.ids[k])] = std::move(s);
  }
  // LocalizedRangeScan::Update of every scan: N x P glibc sincos, on the wide host pool in chunks of 32 scans like CorrectPoses
  {
    const size_t n = S.ids.size(), chunks = (n + 31) / 32;
    auto chunk = [&](size_t c) {
      for (size_t k = 32 * c; k < std::min(n, 32 * c + 32); ++k) {update_scan(*m->scans[static_cast<size_t>(S.ids[k])], m->laser);}
    };
    if (n >= 2048) {host_parallel_for_wide(chunks, chunk);} else {host_parallel_for(chunks, chunk);}
  }
  const auto t2 = std::chrono::steady_clock::now();
  m->adj.assign(static_cast<size_t>(S.n_slots), {}); m->out_edges.assign(static_cast<size_t>(S.n_slots), {});
  {
    size_t a = 0, o = 0;
    for (size_t i = 0; i < static_cast<size_t>(S.n_slots); ++i) {
      m->adj[i].assign(S.adj.begin() + static_cast<std::ptrdiff_t>(a), S.adj.begin() + static_cast<std::ptrdiff_t>(a + S.adj_count[i])); a += S.adj_count[i];
    }
    for (size_t i = 0; i < static_cast<size_t>(S.n_slots); ++i) {
      m->out_edges[i].assign(S.out.begin() + static_cast<std::ptrdiff_t>(o), S.out.begin() + static_cast<std::ptrdiff_t>(o + S.out_count[i])); o += S.out_count[i];
    }
  }
  m->n_edges = S.n_edges; m->running = S.running; m->loc_buffer = S.loc; m->last = static_cast<int32_t>(S.last);
  // the solver: Reset, AddNode*, AddConstraint* in the stored order with the stored information matrices (loadSerializedPoseGraph,
  // slam_toolbox_common.cpp:959-1016), then the gauge and the analysis cache as they stood.  No Compute(): see DESIGN.md section 7
  kh_spa_reset(m->solver);
  for (int64_t k = 0; k < S.n_nodes; ++k) {
    rc = kh_spa_add_node(m->solver, S.node_ids[k], &S.node_poses[3 * k]);
    if (rc) {return fail(rc);}
  }
  for (int64_t k = 0; k < S.n_cons; ++k) {
    rc = kh_spa_add_constraint_information(m->solver, S.ca[k], S.cb[k], &S.cz[3 * k], &S.cinfo[6 * k]);
    if (rc) {kh::bad_file("a constraint's information matrix is not positive definite"); return fail(KH_ERR_IO);}
  }
  kh::spa_import_session_state(m->solver, S.words, S.sn_ptr, S.sn_ids);
  const auto t3 = std::chrono::steady_clock::now();
  m->graph_dirty = true;
  rc = kh::sync_graph(m);
  if (rc) {return fail(rc);}
  const auto t4 = std::chrono::steady_clock::now();
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {return std::chrono::duration<double, std::milli>(b - a).count();};
  kh::g_last_load_ms[0] = ms(t0, t1); kh::g_last_load_ms[1] = ms(t1, t2); kh::g_last_load_ms[2] = ms(t2, t3); kh::g_last_load_ms[3] = ms(t3, t4);
  *out = m;
  return KH_OK;
}

int kh_session_last_load_ms(double out[4])
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  std::copy(kh::g_last_load_ms, kh::g_last_load_ms + 4, out);
  return KH_OK;
}

}  // extern "C"

namespace kh
{
// The residency loop kh_mapper_build_map and the session merger (merge.cpp) share: every scan still in the map gets its ranges
// (once in its life) and its point readings (again only after its pose moved) into HBM on the mapper's own device, the uploads
// queued on `stream`; table gains one record per scan in id order (ResidentScan, the record of kh::occupancy_add_resident).
// *up_points / *up_ranges = uploads this call made.
// ids = NULL: every scan still in the map; otherwise the n_ids scans named (each still in the map), in the order given.
int mapper_resident_table_of(kh_mapper * m, void * stream, const char * who, const int32_t * ids, size_t n_ids, std::vector<ResidentScan> & table,
  int64_t * up_points, int64_t * up_ranges)
{
  const int64_t range_bytes = static_cast<int64_t>(sizeof(double)) * m->laser.n;
  table.clear();
  table.reserve(ids ? n_ids : m->scans.size());
  *up_points = 0; *up_ranges = 0;
  const size_t n_visit = ids ? n_ids : m->scans.size();
  for (size_t k = 0; k < n_visit; ++k) {
    const size_t id = ids ? static_cast<size_t>(ids[k]) : k;
    if (id >= m->scans.size() || !m->scans[id]) {
      if (!ids) {continue;}
      set_error(std::string(who) + ": scan " + std::to_string(id) + " is not in the map");
      return KH_ERR_NOT_FOUND;
    }
    MScan & s = *m->scans[id];
    if (!s.d_ranges) {
      if (m->r_free_slots.empty()) {
        constexpr int kSlabScans = 256;
        void * p = nullptr;
        if (kh_device_malloc(m->device, range_bytes * kSlabScans, &p) == KH_OK) {
          m->r_slabs.push_back(static_cast<double *>(p));
          for (int k = kSlabScans - 1; k >= 0; --k) {m->r_free_slots.push_back(static_cast<double *>(p) + static_cast<size_t>(k) * static_cast<size_t>(m->laser.n));}
        }
      }
      if (!m->r_free_slots.empty()) {s.d_ranges = m->r_free_slots.back(); m->r_free_slots.pop_back(); s.d_ranges_fresh = false;}
    }
    if (s.d_ranges && !s.d_ranges_fresh && s.ranges.size() == static_cast<size_t>(m->laser.n) &&
      kh_device_upload_on(s.d_ranges, s.ranges.data(), range_bytes, stream) == KH_OK) {s.d_ranges_fresh = true; ++*up_ranges;}
    const bool points_stale = !(s.d_points[0] && (s.d_fresh & 1u));
    const double * d_points = resident_points(m, s, 0, stream);
    if (!d_points || !s.d_ranges || !s.d_ranges_fresh) {
      set_error(std::string(who) + ": a scan could not be made resident on the device");
      return KH_ERR_HIP;
    }
    *up_points += points_stale ? 1 : 0;
    table.push_back(ResidentScan{d_points, s.d_ranges, s.sensor.x, s.sensor.y});
  }
  return KH_OK;
}

int mapper_resident_table(kh_mapper * m, void * stream, const char * who, std::vector<ResidentScan> & table, int64_t * up_points, int64_t * up_ranges)
{
  return mapper_resident_table_of(m, stream, who, nullptr, 0, table, up_points, up_ranges);
}

void mapper_sensor_poses(const kh_mapper * m, std::vector<SensorView> & out)
{
  out.clear();
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    SensorView v;
    v.id = sp->id; v.sensor[0] = sp->sensor.x; v.sensor[1] = sp->sensor.y; v.sensor[2] = sp->sensor.h;
    std::copy(sp->bbox, sp->bbox + 4, v.bbox);
    out.push_back(v);
  }
}

// what merge.cpp reads of a mapper (mapper_internal.hpp)
int32_t mapper_device(const kh_mapper * m) {return m->device;}

kh_laser mapper_laser(const kh_mapper * m)
{
  kh_laser l;
  l.n_beams = m->laser.n; l.minimum_angle = m->laser.min_angle; l.angular_resolution = m->laser.ang_res;
  l.minimum_range = m->laser.min_range; l.maximum_range = m->laser.max_range; l.range_threshold = m->laser.range_threshold;
  l.offset_x = m->laser.offset.x; l.offset_y = m->laser.offset.y; l.offset_heading = m->laser.offset.h;
  return l;
}

void mapper_alive_scans(const kh_mapper * m, std::vector<ScanView> & out)
{
  out.clear();
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    ScanView v;
    v.id = sp->id; v.points = sp->points.data(); v.ranges = sp->ranges.data();
    v.corrected[0] = sp->corrected.x; v.corrected[1] = sp->corrected.y; v.corrected[2] = sp->corrected.h;
    v.odometric[0] = sp->odometric.x; v.odometric[1] = sp->odometric.y; v.odometric[2] = sp->odometric.h;
    v.barycenter[0] = sp->barycenter[0]; v.barycenter[1] = sp->barycenter[1];
    v.barycenter[2] = sp->n_filtered != 0 ? 0.0 : sp->sensor.h;       // Pose2(averagePosition, 0.0), or the sensor pose (Karto.h:5687-5692)
    std::copy(sp->bbox, sp->bbox + 4, v.bbox);
    out.push_back(v);
  }
}

void laser_sensor_at(const kh_laser & laser, const double robot[3], double sensor[3])
{
  Laser L;
  L.offset.x = laser.offset_x; L.offset.y = laser.offset_y; L.offset.h = laser.offset_heading;
  Pose r; r.x = robot[0]; r.y = robot[1]; r.h = robot[2];
  const Pose s = sensor_at(L, r);
  sensor[0] = s.x; sensor[1] = s.y; sensor[2] = s.h;
}

double karto_normalize_angle(double angle) {return normalize_angle(angle);}
}  // namespace kh

extern "C" {

// OccupancyGrid::CreateFromScans (Karto.h:5947-5962) from the scans where they lie in HBM
int kh_mapper_build_map(kh_mapper * m, double resolution, uint32_t min_pass_through, double occupancy_threshold, kh_occupancy ** out)
{
  if (!m || !out || !(resolution > 0)) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  // ComputeDimensions (Karto.h:6086-6112): every scan's box is the min / max of its sensor position and its in-range readings
  // (update_scan), so the min / max over the boxes are the min / max kh_occupancy_compute_dimensions finds beam by beam
  kh::Box box;
  int32_t n_alive = 0;
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    ++n_alive;
    box.add(sp->bbox[0], sp->bbox[1]); box.add(sp->bbox[2], sp->bbox[3]);
  }
  if (n_alive == 0) {kh::set_error("kh_mapper_build_map: no scan in the map"); return KH_ERR_INVALID_ARG;}
  int32_t width, height;
  double offset[2];
  kh::grid_dimensions(box, resolution, &width, &height, offset);
  kh_occupancy * g = nullptr;
  int rc = kh_occupancy_create(width, height, offset[0], offset[1], resolution, m->device, &g);
  if (rc) {return rc;}
  void * stream = kh::occupancy_stream(g);
  std::vector<kh::ResidentScan> table;
  int64_t up_points = 0, up_ranges = 0;
  rc = kh::mapper_resident_table(m, stream, "kh_mapper_build_map", table, &up_points, &up_ranges);
  if (rc) {kh::stream_synchronize(stream); kh_occupancy_destroy(g); return rc;}
  rc = kh::occupancy_add_resident(g, n_alive, table.data(), m->laser.n, m->laser.range_threshold, m->laser.min_range, m->laser.max_range);
  if (rc == KH_OK) {rc = kh_occupancy_update(g, min_pass_through, occupancy_threshold);}
  if (rc) {kh::stream_synchronize(stream); kh_occupancy_destroy(g); return rc;}
  m->map_stats[0] += 1; m->map_stats[1] = n_alive; m->map_stats[2] = up_points; m->map_stats[3] = up_ranges;
  m->map_stats[4] += up_points; m->map_stats[5] += up_ranges;
  *out = g;
  return KH_OK;
}

// LocalizedRangeScan::SetCorrectedPose followed by Update (Karto.h:5644-5704): the scan's readings, box and barycentre follow the
// pose.  The solver's node is left alone, as in the reference, so the next CorrectPoses puts the scan where the solver has it.
int kh_mapper_set_scan_pose(kh_mapper * m, int32_t scan_id, const double corrected_pose[3])
{
  if (!m || !corrected_pose) {return KH_ERR_INVALID_ARG;}
  if (scan_id < 0 || scan_id >= static_cast<int32_t>(m->scans.size()) || !m->scans[scan_id]) {
    kh::set_error("kh_mapper_set_scan_pose: no such scan (unknown or removed)");
    return KH_ERR_NOT_FOUND;
  }
  MScan & s = *m->scans[scan_id];
  s.corrected.x = corrected_pose[0]; s.corrected.y = corrected_pose[1]; s.corrected.h = corrected_pose[2];
  kh::update_scan(s, m->laser);
  m->graph_dirty = true;
  return KH_OK;
}

int kh_mapper_map_stats(const kh_mapper * m, int64_t out[6])
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  std::copy(m->map_stats, m->map_stats + 6, out);
  return KH_OK;
}

int kh_mapper_get_params(const kh_mapper * m, kh_mapper_params * out)
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  *out = m->p;
  return KH_OK;
}

// ---- global relocalization: TryCloseLoop's test (Mapper.cpp:1515-1549) for one scan placed at poses taken
// from the map -- a seed vertex per cell of a lattice, n_headings headings each -- instead of at its odometric pose
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
    kh::set_error("kh_mapper_relocalize: seed_spacing > 0, n_headings >= 0, max_base >= 1, top_k >= 0 and finite values are required");
    return KH_ERR_INVALID_ARG;
  }
  if (kh::require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (m->failed) {
    kh::set_error("kh_mapper_relocalize: an earlier Process call failed after its scan had entered the graph; the handle is unusable");
    return KH_ERR_SOLVER;
  }
  const auto t_begin = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) {return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();};
  int32_t n_headings = params->n_headings;
  if (n_headings == 0) {
    const double window = 2.0 * m->p.match.coarse_search_angle_offset;
    const double turns = window > 0 ? std::ceil(kh::k2Pi / window) : 1.0;
    n_headings = (turns >= 1.0 && turns <= 4096.0) ? static_cast<int32_t>(turns) : 1;
  }
  summary->n_headings = n_headings;
  // the graph store is the mapper's own view of itself (rebuilt from the scans whenever an edit outran it): bringing it up to date
  // changes nothing a Process call computes
  if (m->graph_dirty) {const int rc = kh::sync_graph(m); if (rc) {return rc;}}
  if (m->alive.empty()) {summary->total_ms = ms_since(t_begin); return KH_OK;}
  // (1) where to try: seeds and their bases, as positions in the store's scan list
  std::vector<int32_t> seeds, base_begin, base_idx;
  int rc = kh::graph_relocalize_candidates(m->graph, params->seed_spacing, m->p.loop_search_maximum_distance, params->max_base,
      params->radius > 0 ? params->center_xy : nullptr, params->radius, seeds, base_begin, base_idx);
  if (rc) {return rc;}
  summary->kernel_ms = kh_graph_last_relocalize_kernel_ms(m->graph);
  summary->candidates_ms = ms_since(t_begin);
  const size_t n_seeds = seeds.size(), nh = static_cast<size_t>(n_headings);
  const size_t n_hyp = n_seeds * nh;
  if (n_hyp > static_cast<size_t>(0x7fffffff)) {kh::set_error("kh_mapper_relocalize: more than 2^31 hypotheses"); return KH_ERR_INVALID_ARG;}
  summary->n_seeds = static_cast<int32_t>(n_seeds); summary->n_hypotheses = static_cast<int32_t>(n_hyp);
  for (int32_t v : base_idx) {
    if (v < 0 || v >= static_cast<int32_t>(m->alive.size())) {kh::set_error("kh_mapper_relocalize: base index out of range"); return KH_ERR_HIP;}
  }
  struct Result {double cm[3], cc[9], cr, fm[3], fc[9], fr; int32_t passed;};
  std::vector<Result> results(n_hyp);
  // (2) the hypotheses in pieces of max_candidates per member; hypothesis i goes to member i % members, each member runs
  // kh_loop_closure_batch on its own loop / sequential matcher pair against the scan copies of its own device
  const size_t nm = m->member_device.size(), nb = static_cast<size_t>(m->laser.n);
  const size_t piece = static_cast<size_t>(m->max_candidates) * nm;
  const double step = kh::k2Pi / static_cast<double>(n_headings);
  std::vector<double> poses, points;
  for (size_t at = 0; at < n_hyp; at += piece) {
    const size_t np = std::min(piece, n_hyp - at);
    // the query scans of the piece: LocalizedRangeScan::Update at the hypothesis' sensor pose (n_beams libm sincos each, on the worker pool)
    const auto t_scans = std::chrono::steady_clock::now();
    poses.resize(3 * np); points.resize(2 * nb * np);
    for (size_t j = 0; j < np; ++j) {
      const size_t i = at + j;
      const MScan & seed = *m->scans[m->alive[seeds[i / nh]]];
      Pose robot; robot.x = seed.corrected.x; robot.y = seed.corrected.y; robot.h = -kh::kPi + static_cast<double>(i % nh) * step;
      const Pose sensor = kh::sensor_at(m->laser, robot);
      poses[3 * j] = sensor.x; poses[3 * j + 1] = sensor.y; poses[3 * j + 2] = sensor.h;
    }
    kh::host_parallel_for_wide(np, [&](size_t j) {
      kh_scan_points(ranges, m->laser.n, &poses[3 * j], m->laser.min_angle, m->laser.ang_res, &points[2 * nb * j]);
    });
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
          kh_scan b = kh::as_kh_scan(s);
          b.device_points_xy = kh::resident_points(m, s, m->member_slot[k]);
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
      if (shares[k].rc) {kh::set_error(shares[k].error); return shares[k].rc;}
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
  // (3) acceptance and ranking
  std::vector<int32_t> accepted;
  for (size_t i = 0; i < n_hyp; ++i) {
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
    h.index = i; h.seed_scan = m->alive[seeds[static_cast<size_t>(i) / nh]];
    h.heading = -kh::kPi + static_cast<double>(static_cast<size_t>(i) % nh) * step;
    std::copy(r.cm, r.cm + 3, h.coarse_mean); std::copy(r.cc, r.cc + 9, h.coarse_cov); h.coarse_response = r.cr;
    std::copy(r.fm, r.fm + 3, h.fine_mean); std::copy(r.fc, r.fc + 9, h.fine_cov); h.fine_response = r.fr;
    Pose sensor; sensor.x = r.fm[0]; sensor.y = r.fm[1]; sensor.h = r.fm[2];
    const Pose robot = kh::corrected_at(m->laser, sensor);
    h.robot_pose[0] = robot.x; h.robot_pose[1] = robot.y; h.robot_pose[2] = robot.h;
  }
  summary->n_returned = static_cast<int32_t>(n_out);
  summary->total_ms = ms_since(t_begin);
  return KH_OK;
}

}  // extern "C"
