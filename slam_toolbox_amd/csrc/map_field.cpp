// The distance field of a map (kh_map_field_*): the handle owns a copy of the window's cells -- the field is a
// snapshot -- and the values made from it; costs, clearance, the endpoint score and the refinement read those.  The kernels and
// their launchers are occupancy_field.hip's, the rules that need no device map_field_plan.hpp's.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "map_field_plan.hpp"
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
  size_t cells() const {return static_cast<size_t>(view.width_step) * static_cast<size_t>(view.height);}
  FieldWindow window(uint16_t * g = nullptr) const
  {
    return FieldWindow{d_cells, g, d_d2, view.ox, view.oy, view.width, view.height, view.width_step, view.anchor[0], view.anchor[1], view.scale,
                       radius, obstacles};
  }
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
  (void)hipSetDevice(f->view.device);
  if (f->work.stream) {(void)hipStreamSynchronize(f->work.stream);}
  (void)hipFree(f->d_cells); (void)hipFree(f->d_d2);
  work_close(f->work);
  delete f;
}

int kh_map_field_stats_get(kh_map_field * f, kh_map_field_stats * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(f);
  if (rc) {return rc;}
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
  const int32_t rt = inflation_radius_cells(*p, f->view.scale);
  if (rt < 0) {set_error("kh_map_field_costs: the inflation radius lies above 1024 cells"); return KH_ERR_INVALID_ARG;}
  if (f->radius > 0 && f->radius < rt) {
    set_error("kh_map_field_costs: the field reaches " + std::to_string(f->radius) + " cells, the costs ask for " + std::to_string(rt));
    return KH_ERR_INVALID_ARG;
  }
  const std::vector<uint8_t> table = inflation_table(*p, f->view.scale, rt);
  const size_t table_bytes = (table.size() + 15) / 16 * 16;
  std::vector<uint8_t> padded(table_bytes, 0);
  std::memcpy(padded.data(), table.data(), table.size());
  Part parts[] = {{nullptr, (f->cells() + 15) / 16 * 16}, {padded.data(), table_bytes}};
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

}  // extern "C"
