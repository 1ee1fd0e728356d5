// The distance field of a map (kh_map_field_*): the handle owns a copy of the window's cells -- the field is a
// snapshot -- and the values made from it; costs, clearance, the endpoint score and the refinement read those.  The kernels and
// their launchers are occupancy_field.hip's, the rules that need no device map_field_plan.hpp's.
//
// A field that follows its map (kh_map_field_update) is the same handle with its column distances kept
// resident: an update compares the view with the copy, recomputes the part the change can reach and leaves every reader's answer
// what a fresh field would give.  Its kernels are occupancy_field_update.hip's, its rules map_field_update_plan.hpp's, its failure
// rule stands at kh_map_field_update.  The binding to a live map is live_map.cpp's.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "map_field_plan.hpp"
#include "map_field_update_plan.hpp"
#include "occupancy_device.hpp"

using namespace kh;

struct kh_map_field
{
  kh_map_view view;                    // the window and its lattice; the cells are the handle's own copy, row stride ws
  DeviceWork work;                     // the stream, the events around a kernel, a call's tables and answers
  uint8_t * d_cells = nullptr;
  uint32_t * d_d2 = nullptr;
  int32_t radius = 0, obstacles = 0;
  kh_map_field_stats stats;
  // ---- a field that has been updated (section 7p)
  uint16_t * d_g = nullptr;            // the column distances, resident from the first update on
  bool rebuild_next = false;           // an update failed half-way: the next one recomputes the whole window
  bool stats_stale = false;            // the values changed since the three counters were taken: kh_map_field_stats_get recounts
  int32_t forced_band_rows = 0;        // kh_map_field_set_band_rows; 0: band_rows()'s choice
  kh_live_map * live = nullptr;        // the live map the field follows, if any
  size_t cells() const {return static_cast<size_t>(view.width_step) * static_cast<size_t>(view.height);}
  FieldWindow window(uint16_t * g = nullptr) const
  {
    return FieldWindow{d_cells, g, d_d2, view.ox, view.oy, view.width, view.height, view.width_step, view.anchor[0], view.anchor[1], view.scale,
                       radius, obstacles};
  }
  bool same_window(const kh_map_view & v) const {return v.ox == view.ox && v.oy == view.oy && v.width == view.width && v.height == view.height;}
};

namespace
{
const double kInf = std::numeric_limits<double>::infinity();

int failed(kh_map_field * f, const char * who)
{
  (void)hipStreamSynchronize(f->work.stream);
  set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return KH_ERR_HIP;
}

// what every call on a handle begins with once its own arguments are judged: the device, then the handle
int enter(kh_map_field * f)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!f) {return KH_ERR_INVALID_ARG;}
  return hipSetDevice(f->view.device) == hipSuccess ? KH_OK : KH_ERR_HIP;
}

double metres_of(uint32_t d2, double scale) {return d2 == KH_FIELD_FAR ? kInf : std::sqrt(static_cast<double>(d2)) / scale;}

// rows of `row_bytes` bytes out of a device array of stride `stride_bytes` into a host array without padding
bool download_rows(kh_map_field * f, void * out, const void * d_src, size_t row_bytes, size_t stride_bytes)
{
  return hipMemcpy2DAsync(out, row_bytes, d_src, stride_bytes, row_bytes, static_cast<size_t>(f->view.height), hipMemcpyDeviceToHost,
           f->work.stream) == hipSuccess && hipStreamSynchronize(f->work.stream) == hipSuccess;
}

// the snapshot, then the two passes
int build(kh_map_field * f, const kh_map_view & source)
{
  const size_t n = f->cells();
  uint16_t * d_g = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&f->d_cells), n) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&f->d_d2), n * sizeof(uint32_t)) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&d_g), n * sizeof(uint16_t)) != hipSuccess)
  {
    (void)hipGetLastError();
    (void)hipFree(d_g);
    set_error("kh_map_field_create: HIP allocation failed");
    return KH_ERR_HIP;
  }
  hipStream_t s = f->work.stream;
  const size_t ws = static_cast<size_t>(f->view.width_step), width = static_cast<size_t>(f->view.width), height = static_cast<size_t>(f->view.height);
  if (hipMemsetAsync(f->d_cells, 0, n, s) != hipSuccess ||
    hipMemcpy2DAsync(f->d_cells, ws, source.device_cells, static_cast<size_t>(source.width_step), width, height, hipMemcpyDeviceToDevice, s) != hipSuccess)
  {
    (void)hipFree(d_g);
    return failed(f, "kh_map_field_create");
  }
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counters are downloaded as they lie");
  Part parts[] = {{kZeros, kFieldCounters * sizeof(unsigned long long)}};
  int rc = work_stage(f->work, "kh_map_field_create", "counter", false, parts);
  const FieldWindow w = f->window(d_g);
  if (rc == KH_OK) {rc = work_run(f->work, "kh_map_field_create", [&] {field_columns(s, w);}, nullptr, nullptr, &f->stats.times_ms[0]);}
  uint64_t counts[kFieldCounters] = {0, 0, 0};
  bool launched = true;
  if (rc == KH_OK) {
    rc = work_run(f->work, "kh_map_field_create", [&] {launched = field_rows(s, w, parts[0].as<unsigned long long>());}, &parts[0], counts,
        &f->stats.times_ms[1]);
  }
  (void)hipFree(d_g);
  if (rc == KH_OK && !launched) {(void)hipGetLastError(); set_error("kh_map_field_create: the row kernel could not be launched"); rc = KH_ERR_HIP;}
  if (rc) {return rc;}
  f->stats.n_obstacles = counts[kFieldObstacles]; f->stats.n_far = counts[kFieldFar]; f->stats.max_d2 = static_cast<uint32_t>(counts[kFieldMaxD2]);
  return KH_OK;
}

// ---------------------------------------------------------------- the stages of kh_map_field_update
FieldRect field_rect(const Rect & r)
{
  return FieldRect{static_cast<int32_t>(r.x0), static_cast<int32_t>(r.y0), static_cast<int32_t>(r.x1), static_cast<int32_t>(r.y1)};
}

// window columns and rows -> x, y, w, h in lattice cells; none: all zero
void box_out(int32_t out[4], const Rect & r, const kh_map_view & v)
{
  out[0] = r.empty() ? 0 : static_cast<int32_t>(r.x0 + v.ox); out[1] = r.empty() ? 0 : static_cast<int32_t>(r.y0 + v.oy);
  out[2] = static_cast<int32_t>(r.width()); out[3] = static_cast<int32_t>(r.height());
}

// The one statement of "after a failure the next update recomputes the whole window": alive from the first thing queued on the
// field's arrays to the end of the update.
struct RebuildNextUnlessDone
{
  kh_map_field * f;
  bool done = false;
  ~RebuildNextUnlessDone() {if (!done) {f->rebuild_next = true;}}
};

// the three counters from the values as they stand (an updated field keeps none while it works)
int recount(kh_map_field * f)
{
  Part parts[] = {{kZeros, kFieldCounters * sizeof(unsigned long long)}};
  int rc = work_stage(f->work, "kh_map_field_stats_get", "counter", false, parts);
  if (rc) {return rc;}
  uint64_t counts[kFieldCounters] = {0, 0, 0};
  rc = work_run(f->work, "kh_map_field_stats_get", [&] {field_count(f->work.stream, f->window(), parts[0].as<unsigned long long>());}, &parts[0], counts,
      nullptr);
  if (rc) {return rc;}
  f->stats.n_obstacles = counts[kFieldObstacles]; f->stats.n_far = counts[kFieldFar]; f->stats.max_d2 = static_cast<uint32_t>(counts[kFieldMaxD2]);
  f->stats_stale = false;
  return KH_OK;
}

// The arrays of the view's window where the field's differs, the column distances where the field has none: allocated beside what
// the field holds and swapped in only once all are there, so a failure leaves the field as it was.
int layout_stage(kh_map_field * f, const kh_map_view & v, bool relayout)
{
  const int32_t ws = relayout ? field_stride(v.width) : f->view.width_step;
  const size_t n = static_cast<size_t>(ws) * static_cast<size_t>(relayout ? v.height : f->view.height);
  uint8_t * d_cells = nullptr; uint32_t * d_d2 = nullptr; uint16_t * d_g = nullptr;
  bool ok = hipMalloc(reinterpret_cast<void **>(&d_g), n * sizeof(uint16_t)) == hipSuccess;
  if (relayout) {
    ok = ok && hipMalloc(reinterpret_cast<void **>(&d_cells), n) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&d_d2), n * sizeof(uint32_t)) == hipSuccess &&
      hipMemsetAsync(d_cells, 0, n, f->work.stream) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    (void)hipFree(d_cells); (void)hipFree(d_d2); (void)hipFree(d_g);
    set_error("kh_map_field_update: HIP allocation failed");
    return KH_ERR_HIP;
  }
  (void)hipStreamSynchronize(f->work.stream);
  (void)hipFree(f->d_g);
  f->d_g = d_g;
  if (relayout) {
    (void)hipFree(f->d_cells); (void)hipFree(f->d_d2);
    f->d_cells = d_cells; f->d_d2 = d_d2;
    f->view.ox = v.ox; f->view.oy = v.oy; f->view.width = v.width; f->view.height = v.height; f->view.width_step = ws;
    f->view.device_cells = d_cells;
    f->stats.ox = v.ox; f->stats.oy = v.oy; f->stats.width = v.width; f->stats.height = v.height;
  }
  return KH_OK;
}

// the two passes over the rectangles an update names (capped fields): times_ms[1], [2]
int region_stage(kh_map_field * f, const Rect & columns, const Rect & values, kh_field_update & u)
{
  const FieldWindow w = f->window(f->d_g);
  const FieldRect c = field_rect(columns), v = field_rect(values);
  const int32_t band = band_rows(f->radius, columns.height(), f->forced_band_rows);
  int rc = work_run(f->work, "kh_map_field_update", [&] {field_columns_band(f->work.stream, w, c, band);}, nullptr, nullptr, &u.times_ms[1]);
  if (rc) {return rc;}
  bool launched = true;
  rc = work_run(f->work, "kh_map_field_update", [&] {launched = field_rows_region(f->work.stream, w, v);}, nullptr, nullptr, &u.times_ms[2]);
  if (rc == KH_OK && !launched) {(void)hipGetLastError(); set_error("kh_map_field_update: the row kernel could not be launched"); rc = KH_ERR_HIP;}
  if (rc) {return rc;}
  f->stats_stale = true;
  u.cells_recomputed = values.width() * values.height();
  return KH_OK;
}

// the whole window again: the copy, then both passes -- a capped field's by the region kernels over everything, an uncapped field's
// by k_field_columns and k_field_rows, whose counters are the statistics
int rebuild_stage(kh_map_field * f, const kh_map_view & v, kh_field_update & u)
{
  const size_t ws = static_cast<size_t>(f->view.width_step), width = static_cast<size_t>(f->view.width), height = static_cast<size_t>(f->view.height);
  if (hipMemcpy2DAsync(f->d_cells, ws, v.device_cells, static_cast<size_t>(v.width_step), width, height, hipMemcpyDeviceToDevice, f->work.stream) != hipSuccess) {
    return failed(f, "kh_map_field_update");
  }
  const Rect whole = field_window_rect(f->view.width, f->view.height);
  u.rebuilt = 1;
  box_out(u.cells_box, whole, f->view); box_out(u.values_box, whole, f->view);
  if (f->radius > 0) {return region_stage(f, whole, whole, u);}
  Part parts[] = {{kZeros, kFieldCounters * sizeof(unsigned long long)}};
  int rc = work_stage(f->work, "kh_map_field_update", "counter", false, parts);
  const FieldWindow w = f->window(f->d_g);
  if (rc == KH_OK) {rc = work_run(f->work, "kh_map_field_update", [&] {field_columns(f->work.stream, w);}, nullptr, nullptr, &u.times_ms[1]);}
  uint64_t counts[kFieldCounters] = {0, 0, 0};
  bool launched = true;
  if (rc == KH_OK) {
    rc = work_run(f->work, "kh_map_field_update", [&] {launched = field_rows(f->work.stream, w, parts[0].as<unsigned long long>());}, &parts[0], counts,
        &u.times_ms[2]);
  }
  if (rc == KH_OK && !launched) {(void)hipGetLastError(); set_error("kh_map_field_update: the row kernel could not be launched"); rc = KH_ERR_HIP;}
  if (rc) {return rc;}
  f->stats.n_obstacles = counts[kFieldObstacles]; f->stats.n_far = counts[kFieldFar]; f->stats.max_d2 = static_cast<uint32_t>(counts[kFieldMaxD2]);
  f->stats_stale = false;
  u.cells_recomputed = whole.width() * whole.height();
  return KH_OK;
}

// what changed inside `clip`: the copy follows the view, the two boxes and the count come down; times_ms[0]
int compare_stage(kh_map_field * f, const kh_map_view & v, const Rect & clip, kh_field_update & u, Rect * obstacles)
{
  int32_t words[kChangedWords] = {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, 0, 0};
  Part parts[] = {{words, sizeof(words)}};
  int rc = work_stage(f->work, "kh_map_field_update", "result", false, parts);
  if (rc) {return rc;}
  rc = work_run(f->work, "kh_map_field_update", [&] {
    field_changed(f->work.stream, f->window(f->d_g), f->d_cells, static_cast<const uint8_t *>(v.device_cells), v.width_step, field_rect(clip),
      parts[0].as<int32_t>());
  }, &parts[0], words, &u.times_ms[0]);
  if (rc) {return rc;}
  uint64_t compared = 0;
  std::memcpy(&compared, words + kChangedCount, sizeof(compared));
  u.cells_compared = static_cast<int64_t>(compared);
  box_out(u.cells_box, changed_box(words + kChangedStates), f->view);
  *obstacles = changed_box(words + kChangedObstacles);
  return KH_OK;
}

// what the costs refuse once the handle, whose scale and reach they need, is known; then the table, padded to whole 16 bytes
int cost_table(const kh_map_field * f, const char * who, const kh_inflation_params & p, int32_t * rt, std::vector<uint8_t> & padded)
{
  *rt = inflation_radius_cells(p, f->view.scale);
  if (*rt < 0) {set_error(std::string(who) + ": the inflation radius lies above 1024 cells"); return KH_ERR_INVALID_ARG;}
  if (f->radius > 0 && f->radius < *rt) {
    set_error(std::string(who) + ": the field reaches " + std::to_string(f->radius) + " cells, the costs ask for " + std::to_string(*rt));
    return KH_ERR_INVALID_ARG;
  }
  const std::vector<uint8_t> table = inflation_table(p, f->view.scale, *rt);
  padded.assign((table.size() + 15) / 16 * 16, 0);
  std::memcpy(padded.data(), table.data(), table.size());
  return KH_OK;
}

// what a score or a refinement refuses before a device is looked for (the lattice that judges the poses is the handle's)
bool score_inputs_ok(const kh_laser * laser, const double * ranges, int32_t n_poses, const double * sensor_poses, int32_t truncate_cells)
{
  return laser && ranges && sensor_poses && n_poses >= 1 && laser->n_beams >= 1 && truncate_cells >= 0 && truncate_cells <= kMaxFieldRadius;
}

// n_poses poses scored in one launch: the five sums of every pose into `sums`; *kernel_ms += the kernel by events
int score_poses(kh_map_field * f, const char * who, const kh_laser & laser, const double * ranges, int32_t n_poses, const double * sensor_poses, int32_t t,
  std::vector<uint64_t> & sums, double * kernel_ms)
{
  const size_t nb = static_cast<size_t>(laser.n_beams), np = static_cast<size_t>(n_poses);
  if (blocks_per_pose(laser.n_beams, n_poses) == 0) {set_error(std::string(who) + ": too many poses for one launch"); return KH_ERR_INVALID_ARG;}
  std::vector<double> points(2 * nb * np), sensor_xy(2 * np);
  scan_points_at(ranges, 0, laser.n_beams, laser.minimum_angle, laser.angular_resolution, np, sensor_poses, points.data(), sensor_xy.data());
  sums.assign(np * kScoreCounters, 0);
  // the sums first, then the tables: every part a multiple of 8 bytes
  Part parts[] = {{kZeros, np * kScoreCounters * sizeof(unsigned long long)}, {sensor_xy.data(), np * 2 * sizeof(double)}, {ranges, nb * sizeof(double)},
    {points.data(), np * nb * 2 * sizeof(double)}};
  int rc = work_stage(f->work, who, "table", true, parts);
  if (rc) {return rc;}
  double ms = 0.0;
  rc = work_run(f->work, who, [&] {
    field_score(f->work.stream, f->window(), parts[2].as<const double>(), parts[3].as<const double>(), parts[1].as<const double>(), laser.n_beams, n_poses,
      laser.range_threshold, laser.minimum_range, laser.maximum_range, static_cast<uint32_t>(t) * static_cast<uint32_t>(t), parts[0].as<unsigned long long>());
  }, &parts[0], sums.data(), &ms);
  if (kernel_ms) {*kernel_ms += ms;}
  return rc;
}

// the view-level refusals of a score: the laser and the poses as kh_map_fit judges them
int fit_check(const char * who, const kh_map_view & view, const kh_laser & laser, int32_t n_poses, const double * sensor_poses)
{
  const FitInputs in = fit_inputs_check(laser.range_threshold, laser.minimum_range, laser.maximum_range, laser.minimum_angle, laser.angular_resolution,
      static_cast<size_t>(n_poses), sensor_poses, view.anchor[0], view.anchor[1], view.scale);
  if (in.failed) {set_error(fit_inputs_text(in, who, kViewLaserWords, kViewPoseWords)); return KH_ERR_INVALID_ARG;}
  return KH_OK;
}
}  // namespace

extern "C" {

void kh_map_field_params_default(kh_map_field_params * p)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  p->max_distance = 2.0; p->obstacles = KH_FIELD_OBSTACLE_OCCUPIED;
}

int kh_map_field_create(const kh_map_view * view, const kh_map_field_params * params, kh_map_field ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (!params || map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  int32_t radius = 0;
  switch (field_check(view->width, view->height, view->scale, *params, &radius)) {
    case kFieldBadDistance:
      set_error("kh_map_field_create: max_distance must be finite, >= 0 and at most " + std::to_string(kMaxFieldRadius) + " cells");
      return KH_ERR_INVALID_ARG;
    case kFieldBadObstacles:
      set_error("kh_map_field_create: obstacles must be a KH_FIELD_OBSTACLE_ value");
      return KH_ERR_INVALID_ARG;
    case kFieldSideTooLong:
      set_error("kh_map_field_create: a side of the window is longer than 32768 cells");
      return KH_ERR_INVALID_ARG;
    case kFieldTooManyCells:
      set_error("kh_map_field_create: the window holds more than 2^28 cells");
      return KH_ERR_INVALID_ARG;
    case kFieldUncappedTooLong:
      set_error("kh_map_field_create: an uncapped field (max_distance 0) takes sides of at most 4096 cells");
      return KH_ERR_INVALID_ARG;
    default:
      break;
  }
  if (require_device(0) != KH_OK || require_device(view->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  const auto t_begin = std::chrono::steady_clock::now();
  kh_map_field * f = new kh_map_field();
  std::memset(&f->stats, 0, sizeof(f->stats));
  f->view = *view;
  f->view.device_cells = nullptr;
  f->view.width_step = field_stride(view->width);
  f->radius = radius; f->obstacles = params->obstacles;
  f->stats.ox = view->ox; f->stats.oy = view->oy; f->stats.width = view->width; f->stats.height = view->height; f->stats.radius_cells = radius;
  if (!work_open(f->work, view->device)) {
    (void)hipGetLastError();
    set_error("kh_map_field_create: HIP stream / event creation failed");
    kh_map_field_destroy(f);
    return KH_ERR_HIP;
  }
  const int rc = build(f, *view);
  if (rc) {kh_map_field_destroy(f); return rc;}
  f->view.device_cells = f->d_cells;
  f->stats.times_ms[2] = ms_since(t_begin);
  *out = f;
  return KH_OK;
}

void kh_map_field_destroy(kh_map_field * f)
{
  if (!f) {return;}
  if (f->live) {live_map_forget_field(f->live, f);}
  (void)hipSetDevice(f->view.device);
  if (f->work.stream) {(void)hipStreamSynchronize(f->work.stream);}
  (void)hipFree(f->d_cells); (void)hipFree(f->d_d2); (void)hipFree(f->d_g);
  work_close(f->work);
  delete f;
}

int kh_map_field_stats_get(kh_map_field * f, kh_map_field_stats * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  int rc = enter(f);
  if (rc) {return rc;}
  if (f->stats_stale && (rc = recount(f)) != KH_OK) {return rc;}
  *out = f->stats;
  return KH_OK;
}

int kh_map_field_read(kh_map_field * f, uint32_t * d2, double * metres)
{
  const int rc = enter(f);
  if (rc) {return rc;}
  if (!d2 && !metres) {return KH_OK;}
  const size_t width = static_cast<size_t>(f->view.width), total = width * static_cast<size_t>(f->view.height);
  std::vector<uint32_t> own(d2 ? 0 : total);
  uint32_t * const values = d2 ? d2 : own.data();
  if (!download_rows(f, values, f->d_d2, width * sizeof(uint32_t), static_cast<size_t>(f->view.width_step) * sizeof(uint32_t))) {
    return failed(f, "kh_map_field_read");
  }
  if (metres) {
    for (size_t k = 0; k < total; ++k) {metres[k] = metres_of(values[k], f->view.scale);}
  }
  return KH_OK;
}

void kh_inflation_params_default(kh_inflation_params * p)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  p->inscribed_radius = 0.22; p->inflation_radius = 0.55; p->cost_scaling_factor = 10.0; p->track_unknown = 1; p->inflate_unknown = 0;
}

int kh_inflation_table(const kh_inflation_params * p, double scale, uint8_t * table, int32_t cap, int32_t * n)
{
  if (!p || !n || cap < 0 || (cap > 0 && !table)) {return KH_ERR_INVALID_ARG;}
  *n = 0;
  const int32_t rt = inflation_radius_cells(*p, scale);
  if (rt < 0) {
    set_error("kh_inflation_table: finite radii and factor >= 0, inscribed <= inflation <= 1024 cells, flags 0 / 1 and a scale > 0 are required");
    return KH_ERR_INVALID_ARG;
  }
  *n = rt * rt + 1;
  if (cap == 0) {return KH_OK;}
  if (cap < *n) {return KH_ERR_INVALID_ARG;}
  const std::vector<uint8_t> t = inflation_table(*p, scale, rt);
  std::memcpy(table, t.data(), t.size());
  return KH_OK;
}

int kh_map_field_costs(kh_map_field * f, const kh_inflation_params * p, uint8_t * out)
{
  if (!p || !out) {return KH_ERR_INVALID_ARG;}
  if (!inflation_params_ok(*p)) {               // (the radius in cells is judged once the handle, whose scale it needs, is known)
    set_error("kh_map_field_costs: finite radii and factor >= 0, inscribed <= inflation and flags 0 / 1 are required");
    return KH_ERR_INVALID_ARG;
  }
  int rc = enter(f);
  if (rc) {return rc;}
  int32_t rt = 0;
  std::vector<uint8_t> padded;
  if ((rc = cost_table(f, "kh_map_field_costs", *p, &rt, padded)) != KH_OK) {return rc;}
  Part parts[] = {{nullptr, (f->cells() + 15) / 16 * 16}, {padded.data(), padded.size()}};
  rc = work_stage(f->work, "kh_map_field_costs", "table", false, parts);
  if (rc) {return rc;}
  rc = work_run(f->work, "kh_map_field_costs", [&] {
    field_costs(f->work.stream, f->window(), parts[1].as<const uint8_t>(), static_cast<uint32_t>(rt) * static_cast<uint32_t>(rt), p->track_unknown,
      p->inflate_unknown, parts[0].as<uint8_t>());
  }, nullptr, nullptr, nullptr);
  if (rc) {return rc;}
  // (one plain copy and the rows compacted here: a pitched copy of rows of an odd number of BYTES takes milliseconds)
  const size_t width = static_cast<size_t>(f->view.width), ws = static_cast<size_t>(f->view.width_step), height = static_cast<size_t>(f->view.height);
  std::vector<uint8_t> strided(ws == width ? 0 : f->cells());
  uint8_t * const host = ws == width ? out : strided.data();
  if (hipMemcpyAsync(host, parts[0].d, f->cells(), hipMemcpyDeviceToHost, f->work.stream) != hipSuccess || hipStreamSynchronize(f->work.stream) != hipSuccess) {
    return failed(f, "kh_map_field_costs");
  }
  for (size_t row = 0; ws != width && row < height; ++row) {std::memcpy(out + row * width, host + row * ws, width);}
  return KH_OK;
}

int kh_map_field_clearance(kh_map_field * f, int32_t n, const double * xy, double * metres, int32_t * status, uint32_t * d2)
{
  if (n < 1 || !xy) {return KH_ERR_INVALID_ARG;}
  for (int64_t k = 0; k < 2 * static_cast<int64_t>(n); ++k) {
    if (!std::isfinite(xy[k])) {set_error("kh_map_field_clearance: point " + std::to_string(k / 2) + " is not finite"); return KH_ERR_INVALID_ARG;}
  }
  int rc = enter(f);
  if (rc) {return rc;}
  const size_t np = static_cast<size_t>(n), words = (np + 1) / 2 * 2;                 // every part a multiple of 8 bytes
  Part parts[] = {{nullptr, 2 * words * sizeof(uint32_t)}, {xy, np * 2 * sizeof(double)}};
  rc = work_stage(f->work, "kh_map_field_clearance", "table", true, parts);
  if (rc) {return rc;}
  std::vector<uint32_t> answer(2 * words);
  rc = work_run(f->work, "kh_map_field_clearance", [&] {
    field_lookup(f->work.stream, f->window(), n, parts[1].as<const double>(), parts[0].as<uint32_t>(), parts[0].as<int32_t>() + words);
  }, &parts[0], answer.data(), nullptr);
  if (rc) {return rc;}
  for (size_t k = 0; k < np; ++k) {
    const int32_t code = static_cast<int32_t>(answer[words + k]);
    if (d2) {d2[k] = answer[k];}
    if (status) {status[k] = code;}
    if (metres) {metres[k] = code == KH_CLEAR_OK ? metres_of(answer[k], f->view.scale) : kInf;}
  }
  return KH_OK;
}

int kh_map_field_score(kh_map_field * f, const kh_laser * laser, const double * ranges, int32_t n_poses, const double * sensor_poses,
  int32_t truncate_cells, kh_field_score * out)
{
  if (!out || !score_inputs_ok(laser, ranges, n_poses, sensor_poses, truncate_cells)) {return KH_ERR_INVALID_ARG;}
  int rc = enter(f);
  if (rc) {return rc;}
  if (fit_check("kh_map_field_score", f->view, *laser, n_poses, sensor_poses) != KH_OK) {return KH_ERR_INVALID_ARG;}
  const int32_t t = score_truncation(truncate_cells, f->radius);
  if (t < 0) {set_error("kh_map_field_score: an uncapped field needs truncate_cells > 0"); return KH_ERR_INVALID_ARG;}
  std::vector<uint64_t> sums;
  rc = score_poses(f, "kh_map_field_score", *laser, ranges, n_poses, sensor_poses, t, sums, nullptr);
  if (rc) {return rc;}
  for (size_t k = 0; k < static_cast<size_t>(n_poses); ++k) {out[k] = score_derive(&sums[k * kScoreCounters], t);}
  return KH_OK;
}

void kh_field_refine_params_default(kh_field_refine_params * p, double scale)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  p->step_xy = 2.0 / scale; p->step_heading = 0.02; p->n_halvings = 4; p->max_rounds = 64; p->truncate_cells = 0;
}

int kh_map_field_refine(kh_map_field * f, const kh_laser * laser, const double * ranges, int32_t n, const double * sensor_poses,
  const kh_field_refine_params * params, kh_field_refined * out, double times_ms[2])
{
  if (times_ms) {times_ms[0] = times_ms[1] = 0.0;}
  if (!out || !params || !score_inputs_ok(laser, ranges, n, sensor_poses, params->truncate_cells)) {return KH_ERR_INVALID_ARG;}
  if (!refine_params_ok(*params)) {
    set_error("kh_map_field_refine: a finite step_xy > 0 and step_heading >= 0, 0 <= n_halvings <= 32 and 1 <= max_rounds <= 4096 are required");
    return KH_ERR_INVALID_ARG;
  }
  if (n > INT32_MAX / kRefineCandidates) {set_error("kh_map_field_refine: too many starts"); return KH_ERR_INVALID_ARG;}
  int rc = enter(f);
  if (rc) {return rc;}
  if (fit_check("kh_map_field_refine", f->view, *laser, n, sensor_poses) != KH_OK) {return KH_ERR_INVALID_ARG;}
  const int32_t t = score_truncation(params->truncate_cells, f->radius);
  if (t < 0) {set_error("kh_map_field_refine: an uncapped field needs truncate_cells > 0"); return KH_ERR_INVALID_ARG;}
  const auto t_begin = std::chrono::steady_clock::now();
  double kernel_ms = 0.0;
  std::vector<uint64_t> sums;
  rc = score_poses(f, "kh_map_field_refine", *laser, ranges, n, sensor_poses, t, sums, &kernel_ms);
  if (rc) {return rc;}
  std::vector<RefineStart> starts(static_cast<size_t>(n));
  for (size_t k = 0; k < starts.size(); ++k) {
    const kh_field_score here = score_derive(&sums[k * kScoreCounters], t);
    starts[k].begin(sensor_poses + 3 * k, *params, here.cost, here.n_hit);
  }
  std::vector<double> poses;
  std::vector<size_t> running;
  for (;;) {
    poses.clear(); running.clear();
    for (size_t k = 0; k < starts.size(); ++k) {
      if (!starts[k].running()) {continue;}
      poses.resize(poses.size() + 3 * kRefineCandidates);
      if (starts[k].candidates(f->view.anchor[0], f->view.anchor[1], f->view.scale, poses.data() + poses.size() - 3 * kRefineCandidates)) {
        running.push_back(k);
      } else {
        poses.resize(poses.size() - 3 * kRefineCandidates);
      }
    }
    if (running.empty()) {break;}
    rc = score_poses(f, "kh_map_field_refine", *laser, ranges, static_cast<int32_t>(running.size()) * kRefineCandidates, poses.data(), t, sums, &kernel_ms);
    if (rc) {return rc;}
    for (size_t q = 0; q < running.size(); ++q) {
      uint64_t costs[kRefineCandidates];
      for (int32_t c = 0; c < kRefineCandidates; ++c) {costs[c] = score_derive(&sums[(q * kRefineCandidates + c) * kScoreCounters], t).cost;}
      starts[running[q]].advance(costs, *params);
    }
  }
  for (size_t k = 0; k < starts.size(); ++k) {out[k] = starts[k].result();}
  if (times_ms) {times_ms[0] = kernel_ms; times_ms[1] = ms_since(t_begin);}
  return KH_OK;
}

// The failure rule.  What is refused before the device is used -- a view off the lattice, a window beyond the limits -- and a failed
// allocation leave the field as it was.  After any later failure the field stays usable, holds values that may be stale where the
// change reaches, and its next update recomputes the whole window (RebuildNextUnlessDone).
int kh_map_field_update(kh_map_field * f, const kh_map_view * view, const int32_t rect[4], kh_field_update * out)
{
  if (out) {std::memset(out, 0, sizeof(*out));}
  if (map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (f) {
    static const char * const kOff[] = {"", "anchor x", "anchor y", "scale", "device"};
    const int32_t off = lattice_check(f->view.anchor, f->view.scale, f->view.device, view->anchor, view->scale, view->device);
    if (off != kLatticeSame) {set_error(std::string("kh_map_field_update: the view is not on the field's lattice: its ") + kOff[off] + " differs"); return KH_ERR_INVALID_ARG;}
    if (!f->same_window(*view) && update_window_check(view->width, view->height, f->radius) != kFieldOk) {
      set_error("kh_map_field_update: the view's window is beyond the limits of kh_map_field_create");
      return KH_ERR_INVALID_ARG;
    }
  }
  int rc = enter(f);
  if (rc) {return rc;}
  const auto t_begin = std::chrono::steady_clock::now();
  kh_field_update u;
  std::memset(&u, 0, sizeof(u));
  const int32_t kind = update_kind(f->same_window(*view), f->d_g != nullptr, f->radius, f->rebuild_next);
  if (kind == kUpdateRegion) {
    const Rect clip = update_clip(rect, f->view.ox, f->view.oy, f->view.width, f->view.height);
    if (!clip.empty()) {
      RebuildNextUnlessDone guard{f};
      Rect obstacles;
      if ((rc = compare_stage(f, *view, clip, u, &obstacles)) != KH_OK) {return rc;}
      if (!obstacles.empty()) {
        const UpdateRegions regions = update_regions(obstacles, f->radius, f->view.width, f->view.height);
        box_out(u.values_box, regions.values, f->view);
        if ((rc = region_stage(f, regions.columns, regions.values, u)) != KH_OK) {return rc;}
      }
      guard.done = true;
    }
  } else {
    if (kind == kUpdateRelayout || kind == kUpdateNoColumns) {
      if ((rc = layout_stage(f, *view, kind == kUpdateRelayout)) != KH_OK) {return rc;}
      u.relayout = kind == kUpdateRelayout;
    }
    RebuildNextUnlessDone guard{f};
    if ((rc = rebuild_stage(f, *view, u)) != KH_OK) {return rc;}
    f->rebuild_next = false;
    guard.done = true;
  }
  u.times_ms[3] = ms_since(t_begin);
  if (u.rebuilt) {f->stats.times_ms[0] = u.times_ms[1]; f->stats.times_ms[1] = u.times_ms[2]; f->stats.times_ms[2] = u.times_ms[3];}
  if (out) {*out = u;}
  return KH_OK;
}

int kh_map_field_set_band_rows(kh_map_field * f, int32_t rows)
{
  if (rows < 0) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(f);
  if (rc) {return rc;}
  f->forced_band_rows = rows;
  return KH_OK;
}

int kh_map_field_read_rect(kh_map_field * f, int32_t x, int32_t y, int32_t w, int32_t h, uint32_t * d2)
{
  if (!d2 || w < 1 || h < 1) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(f);
  if (rc) {return rc;}
  const int32_t rect[4] = {x, y, w, h};
  const Rect r = update_clip(rect, f->view.ox, f->view.oy, f->view.width, f->view.height);
  if (r.width() != w || r.height() != h) {set_error("kh_map_field_read_rect: the rectangle does not lie inside the window"); return KH_ERR_INVALID_ARG;}
  const size_t ws = static_cast<size_t>(f->view.width_step), row_bytes = static_cast<size_t>(w) * sizeof(uint32_t);
  if (hipMemcpy2DAsync(d2, row_bytes, f->d_d2 + static_cast<size_t>(r.y0) * ws + static_cast<size_t>(r.x0), ws * sizeof(uint32_t), row_bytes, static_cast<size_t>(h),
      hipMemcpyDeviceToHost, f->work.stream) != hipSuccess || hipStreamSynchronize(f->work.stream) != hipSuccess) {return failed(f, "kh_map_field_read_rect");}
  return KH_OK;
}

int kh_map_field_costs_rect(kh_map_field * f, const kh_inflation_params * p, int32_t x, int32_t y, int32_t w, int32_t h, uint8_t * out)
{
  if (!p || !out || w < 1 || h < 1) {return KH_ERR_INVALID_ARG;}
  if (!inflation_params_ok(*p)) {
    set_error("kh_map_field_costs_rect: finite radii and factor >= 0, inscribed <= inflation and flags 0 / 1 are required");
    return KH_ERR_INVALID_ARG;
  }
  int rc = enter(f);
  if (rc) {return rc;}
  const int32_t rect[4] = {x, y, w, h};
  const Rect r = update_clip(rect, f->view.ox, f->view.oy, f->view.width, f->view.height);
  if (r.width() != w || r.height() != h) {set_error("kh_map_field_costs_rect: the rectangle does not lie inside the window"); return KH_ERR_INVALID_ARG;}
  int32_t rt = 0;
  std::vector<uint8_t> padded;
  if ((rc = cost_table(f, "kh_map_field_costs_rect", *p, &rt, padded)) != KH_OK) {return rc;}
  const size_t width = static_cast<size_t>(w), ws = static_cast<size_t>(field_stride(w)), height = static_cast<size_t>(h);
  std::vector<uint8_t> strided(ws == width ? 0 : ws * height);
  uint8_t * const host = ws == width ? out : strided.data();
  Part parts[] = {{nullptr, (ws * height + 15) / 16 * 16}, {padded.data(), padded.size()}};
  rc = work_stage(f->work, "kh_map_field_costs_rect", "table", false, parts);
  if (rc) {return rc;}
  Part answer{nullptr, ws * height, parts[0].d};
  rc = work_run(f->work, "kh_map_field_costs_rect", [&] {
    field_costs_rect(f->work.stream, f->window(), field_rect(r), parts[1].as<const uint8_t>(), static_cast<uint32_t>(rt) * static_cast<uint32_t>(rt),
      p->track_unknown, p->inflate_unknown, parts[0].as<uint8_t>(), static_cast<int32_t>(ws));
  }, &answer, host, nullptr);
  if (rc) {return rc;}
  for (size_t row = 0; ws != width && row < height; ++row) {std::memcpy(out + row * width, host + row * ws, width);}
  return KH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the live binding's side of the handle (live_map.cpp holds the rest)
namespace kh
{
kh_live_map * map_field_live(const kh_map_field * f) {return f->live;}
void map_field_set_live(kh_map_field * f, kh_live_map * g) {f->live = g;}
FieldWindow map_field_window(const kh_map_field * f) {return f->window();}
int32_t map_field_device(const kh_map_field * f) {return f->view.device;}

// a handle on the view's lattice with no window and no arrays yet: kh_map_field_update on the same view lays it out and builds it
int map_field_create_empty(const kh_map_view & view, const kh_map_field_params & params, const char * who, kh_map_field ** out)
{
  *out = nullptr;
  int32_t radius = 0;
  if (field_check(view.width, view.height, view.scale, params, &radius) != kFieldOk) {
    set_error(std::string(who) + ": the parameters or the window are beyond what kh_map_field_create takes");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(view.device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_map_field * f = new kh_map_field();
  std::memset(&f->stats, 0, sizeof(f->stats));
  f->view = view;
  f->view.device_cells = nullptr;
  f->view.ox = f->view.oy = f->view.width = f->view.height = f->view.width_step = 0;
  f->radius = radius; f->obstacles = params.obstacles;
  f->stats.radius_cells = radius;
  if (!work_open(f->work, view.device)) {
    (void)hipGetLastError();
    set_error(std::string(who) + ": HIP stream / event creation failed");
    kh_map_field_destroy(f);
    return KH_ERR_HIP;
  }
  *out = f;
  return KH_OK;
}
}  // namespace kh
