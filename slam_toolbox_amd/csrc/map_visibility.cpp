// Visibility on a map (kh_map_visibility_*): the handle owns a copy of the view struct (the cells stay
// borrowed), the covered mask over the view's window and the buffer of a call's tables and answers.  The kernels and their launchers
// are occupancy_visibility.hip's, the rules that need no device map_visibility_plan.hpp's.  A call computes the far points of its poses
// on the host (libm stays there, as for kh_map_raycast), uploads them, launches and downloads once: a select enqueues all its rounds --
// gain over the candidates, best, commit of the pick -- and reads nothing between them.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "map_visibility_plan.hpp"
#include "occupancy_device.hpp"

using namespace kh;

struct kh_map_visibility
{
  kh_map_view view;
  kh_laser laser;
  kh_visibility_params params;
  int32_t reach = 0;
  DeviceWork work;                     // the stream, the events around a call's kernels, a call's tables and answers
  uint32_t * d_mask = nullptr;         // vis_mask_words(width, height) words
  bool skip = true;                    // read before the OR (DESIGN.md 7s' leg)
  kh_map_visibility_stats stats;
};

namespace
{
size_t up16(size_t bytes) {return (bytes + 15) / 16 * 16;}

int enter(kh_map_visibility * v)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!v) {return KH_ERR_INVALID_ARG;}
  return hipSetDevice(v->work.device) == hipSuccess ? KH_OK : KH_ERR_HIP;
}

int failed(kh_map_visibility * v, const char * who)
{
  (void)hipStreamSynchronize(v->work.stream);
  set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return KH_ERR_HIP;
}

size_t mask_bytes(const kh_map_visibility * v) {return static_cast<size_t>(vis_mask_words(v->view.width, v->view.height)) * sizeof(uint32_t);}

// the poses' refusals of a call, under `who`; the handle may be NULL (it is looked at after the device): then only what needs no
// handle is checked
int call_check(const char * who, const kh_map_visibility * v, bool nulls, int32_t n, const double * poses, bool select, int32_t k, uint32_t min_gain)
{
  static const char * const kWhy[] = {"", "", "n must lie in 1 .. 65536", "pose # is not finite or lies more than 2^30 cells from the anchor",
    "k must lie in 1 .. min(n, 4096)", "min_gain must be at least 1", "n * n_beams lies above 2^24"};
  int32_t bad_pose = -1;
  const int32_t bad = v ? vis_call_check(nulls, n, poses, v->view.anchor[0], v->view.anchor[1], v->view.scale, v->laser.n_beams, select, k, min_gain, &bad_pose) :
    vis_call_check(nulls, n, poses, 0.0, 0.0, 1.0, 1, select, k, min_gain, &bad_pose);
  if (bad == kVisCallOk) {return KH_OK;}
  std::string words = kWhy[bad];
  const size_t at = words.find('#');
  if (at != std::string::npos) {words.replace(at, 1, std::to_string(bad_pose));}
  if (!words.empty()) {set_error(std::string(who) + ": " + words);}
  return KH_ERR_INVALID_ARG;
}

// the far points and sensor positions of n poses, as k_map_raycast's tables
void tables(const kh_map_visibility * v, int32_t n, const double * poses, std::vector<double> * points, std::vector<double> * sensor_xy)
{
  const size_t nb = static_cast<size_t>(v->laser.n_beams), np = static_cast<size_t>(n);
  const std::vector<double> far(nb, v->laser.range_threshold);
  points->resize(2 * nb * np); sensor_xy->resize(2 * np);
  scan_points_at(far.data(), 0, v->laser.n_beams, v->laser.minimum_angle, v->laser.angular_resolution, np, poses, points->data(), sensor_xy->data());
}

VisJob job_of(const kh_map_visibility * v, const Part & head, const Part & sensors, const Part & points)
{
  VisJob j;
  j.g = window_of(v->view); j.points = points.as<const double>(); j.sensors = sensors.as<const double>();
  j.n_beams = v->laser.n_beams; j.max_unknown = v->params.max_unknown; j.reach = v->reach;
  j.w_unknown = static_cast<uint32_t>(v->params.w_unknown); j.w_free = static_cast<uint32_t>(v->params.w_free);
  j.w_occupied = static_cast<uint32_t>(v->params.w_occupied);
  j.mask = v->d_mask; j.head = head.as<VisHead>(); j.picked = nullptr;
  return j;
}

void begin_stats(kh_map_visibility * v, int32_t n)
{
  v->stats.n_poses = n; v->stats.rounds = 0; v->stats.launches = 0; v->stats.kernel_ms = 0.0; v->stats.call_ms = 0.0;
}

int beyond_reach(const char * who) {set_error(std::string(who) + ": a far cell lies beyond the reach (the bound did not hold)"); return KH_ERR_HIP;}
int no_lds(const char * who) {set_error(std::string(who) + ": the bitmap does not fit the workgroup's LDS"); return KH_ERR_HIP;}
}  // namespace

extern "C" {

void kh_map_visibility_params_default(kh_visibility_params * p)
{
  if (!p) {return;}
  p->max_unknown = 20; p->w_unknown = 1; p->w_free = 0; p->w_occupied = 0;
}

int kh_map_visibility_create(const kh_map_view * view, const kh_laser * laser, const kh_visibility_params * params, kh_map_visibility ** out)
{
  static const char * const who = "kh_map_visibility_create";
  if (out) {*out = nullptr;}
  static const char * const kWhy[] = {"", "", "malformed map view, or one too large or off the int32 lattice", kViewLaserWords, "max_unknown must be at least -1",
    "the weights must lie in 0 .. 255 and not all be zero", "the laser reaches beyond 511 cells: floor(range_threshold * scale) + 2 > 511"};
  int32_t reach = 0;
  const int32_t bad = vis_create_check(view, laser, params, out, &reach);
  if (bad != kVisOk) {
    if (bad != kVisNull) {set_error(std::string(who) + ": " + (bad == kVisBadLaser && laser->n_beams < 1 ? "the laser has no beams" : kWhy[bad]));}
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(0) != KH_OK || require_device(view->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_map_visibility * v = new kh_map_visibility();
  std::memset(&v->stats, 0, sizeof(v->stats));
  v->view = *view; v->laser = *laser; v->params = *params; v->reach = reach;
  v->stats.ox = view->ox; v->stats.oy = view->oy; v->stats.width = view->width; v->stats.height = view->height;
  v->stats.reach = reach; v->stats.bitmap_bytes = vis_bitmap_bytes(reach);
  if (!(work_open(v->work, view->device) && hipMalloc(reinterpret_cast<void **>(&v->d_mask), mask_bytes(v)) == hipSuccess &&
    hipMemsetAsync(v->d_mask, 0, mask_bytes(v), v->work.stream) == hipSuccess && hipStreamSynchronize(v->work.stream) == hipSuccess)) {
    (void)hipGetLastError();
    set_error(std::string(who) + ": HIP stream, event or mask allocation failed");
    kh_map_visibility_destroy(v);
    return KH_ERR_HIP;
  }
  *out = v;
  return KH_OK;
}

void kh_map_visibility_destroy(kh_map_visibility * v)
{
  if (!v) {return;}
  (void)hipSetDevice(v->work.device);
  if (v->work.stream) {(void)hipStreamSynchronize(v->work.stream);}
  (void)hipFree(v->d_mask);
  work_close(v->work);
  delete v;
}

int kh_map_visibility_set_map(kh_map_visibility * v, const kh_map_view * view)
{
  static const char * const who = "kh_map_visibility_set_map";
  if (!view || map_view_refusal(view) != kViewOk) {set_error(std::string(who) + ": malformed map view"); return KH_ERR_INVALID_ARG;}
  if (v && !vis_same_window(v->view, *view)) {
    set_error(std::string(who) + ": the view is not one of the handle's window, lattice and device");
    return KH_ERR_INVALID_ARG;
  }
  const int rc = enter(v);
  if (rc) {return rc;}
  (void)hipStreamSynchronize(v->work.stream);
  v->view = *view;
  return KH_OK;
}

int kh_map_visibility_clear(kh_map_visibility * v)
{
  const int rc = enter(v);
  if (rc) {return rc;}
  if (hipMemsetAsync(v->d_mask, 0, mask_bytes(v), v->work.stream) != hipSuccess || hipStreamSynchronize(v->work.stream) != hipSuccess) {
    return failed(v, "kh_map_visibility_clear");
  }
  return KH_OK;
}

int kh_map_visibility_set_skip(kh_map_visibility * v, int32_t skip)
{
  if (skip < 0 || skip > 1) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(v);
  if (rc) {return rc;}
  v->skip = skip != 0;
  return KH_OK;
}

int kh_map_visibility_commit(kh_map_visibility * v, int32_t n, const double * sensor_poses)
{
  static const char * const who = "kh_map_visibility_commit";
  int rc = call_check(who, v, false, n, sensor_poses, false, 0, 0u);
  if (rc) {return rc;}
  if ((rc = enter(v)) != KH_OK) {return rc;}
  const auto t_begin = std::chrono::steady_clock::now();
  begin_stats(v, n);
  std::vector<double> points, sensor_xy;
  tables(v, n, sensor_poses, &points, &sensor_xy);
  sensor_xy.resize(up16(sensor_xy.size() * sizeof(double)) / sizeof(double));
  Part parts[] = {{kZeros, sizeof(VisHead)}, {sensor_xy.data(), sensor_xy.size() * sizeof(double)}, {points.data(), points.size() * sizeof(double)}};
  rc = work_stage(v->work, who, "table", true, parts);
  if (rc) {return rc;}
  VisHead head;
  bool launched = false;
  rc = work_run(v->work, who, [&] {launched = vis_commit(v->work.stream, job_of(v, parts[0], parts[1], parts[2]), n, v->skip, false);}, &parts[0], &head,
      &v->stats.kernel_ms);
  if (rc) {return rc;}
  if (!launched) {return no_lds(who);}
  v->stats.launches = 1; v->stats.call_ms = ms_since(t_begin);
  return head.error != 0u ? beyond_reach(who) : KH_OK;
}

int kh_map_visibility_gain(kh_map_visibility * v, int32_t n, const double * sensor_poses, kh_visibility_t * out, double * kernel_ms)
{
  static const char * const who = "kh_map_visibility_gain";
  if (kernel_ms) {*kernel_ms = 0.0;}
  int rc = call_check(who, v, !out, n, sensor_poses, false, 0, 0u);
  if (rc) {return rc;}
  if ((rc = enter(v)) != KH_OK) {return rc;}
  const auto t_begin = std::chrono::steady_clock::now();
  begin_stats(v, n);
  std::vector<double> points, sensor_xy;
  tables(v, n, sensor_poses, &points, &sensor_xy);
  const size_t np = static_cast<size_t>(n), record_bytes = up16(np * sizeof(kh_visibility_t));
  sensor_xy.resize(up16(sensor_xy.size() * sizeof(double)) / sizeof(double));
  Part parts[] = {{kZeros, sizeof(VisHead)}, {nullptr, record_bytes}, {sensor_xy.data(), sensor_xy.size() * sizeof(double)},
    {points.data(), points.size() * sizeof(double)}};
  rc = work_stage(v->work, who, "table", true, parts);
  if (rc) {return rc;}
  std::vector<uint8_t> answer(sizeof(VisHead) + record_bytes);
  const Part both{nullptr, answer.size(), parts[0].d};        // the head and the records lie together
  bool launched = false;
  rc = work_run(v->work, who, [&] {
    launched = vis_gain(v->work.stream, job_of(v, parts[0], parts[2], parts[3]), n, v->skip, parts[1].as<kh_visibility_t>());
  }, &both, answer.data(), &v->stats.kernel_ms);
  if (rc) {return rc;}
  if (!launched) {return no_lds(who);}
  VisHead head;
  std::memcpy(&head, answer.data(), sizeof(head));
  if (head.error != 0u) {return beyond_reach(who);}
  std::memcpy(out, answer.data() + sizeof(VisHead), np * sizeof(kh_visibility_t));
  if (kernel_ms) {*kernel_ms = v->stats.kernel_ms;}
  v->stats.launches = 1; v->stats.call_ms = ms_since(t_begin);
  return KH_OK;
}

int kh_map_visibility_select(kh_map_visibility * v, int32_t n, const double * sensor_poses, int32_t k, uint32_t min_gain, int32_t * picks, uint32_t * pick_gains,
  int32_t * n_picked)
{
  static const char * const who = "kh_map_visibility_select";
  if (n_picked) {*n_picked = 0;}
  int rc = call_check(who, v, !picks || !pick_gains || !n_picked, n, sensor_poses, true, k, min_gain);
  if (rc) {return rc;}
  if ((rc = enter(v)) != KH_OK) {return rc;}
  const auto t_begin = std::chrono::steady_clock::now();
  begin_stats(v, n);
  std::vector<double> points, sensor_xy;
  tables(v, n, sensor_poses, &points, &sensor_xy);
  const size_t np = static_cast<size_t>(n), nk = static_cast<size_t>(k), pick_bytes = up16(2 * nk * sizeof(uint32_t));
  sensor_xy.resize(up16(sensor_xy.size() * sizeof(double)) / sizeof(double));
  // the head, the picks and their gains (downloaded together), the picked words, the records, the tables
  Part parts[] = {{kZeros, sizeof(VisHead)}, {kZeros, pick_bytes}, {kZeros, up16(np * sizeof(uint32_t))}, {nullptr, up16(np * sizeof(kh_visibility_t))},
    {sensor_xy.data(), sensor_xy.size() * sizeof(double)}, {points.data(), points.size() * sizeof(double)}};
  rc = work_stage(v->work, who, "table", true, parts);
  if (rc) {return rc;}
  std::vector<uint8_t> answer(sizeof(VisHead) + pick_bytes);
  const Part both{nullptr, answer.size(), parts[0].d};
  VisJob job = job_of(v, parts[0], parts[4], parts[5]);
  bool launched = true;
  rc = work_run(v->work, who, [&] {
    hipStream_t s = v->work.stream;
    for (int32_t r = 0; r < k && launched; ++r) {
      job.picked = parts[2].as<const uint32_t>();
      launched = vis_gain(s, job, n, v->skip, parts[3].as<kh_visibility_t>());
      vis_best(s, parts[3].as<const kh_visibility_t>(), n, min_gain, parts[2].as<uint32_t>(), job.head, parts[1].as<uint32_t>(), parts[1].as<uint32_t>() + nk);
      job.picked = nullptr;
      launched = launched && vis_commit(s, job, 1, v->skip, true);
    }
  }, &both, answer.data(), &v->stats.kernel_ms);
  if (rc) {return rc;}
  if (!launched) {return no_lds(who);}
  VisHead head;
  std::memcpy(&head, answer.data(), sizeof(head));
  if (head.error != 0u || head.n_picked > static_cast<uint32_t>(k)) {return beyond_reach(who);}
  const uint32_t * words = reinterpret_cast<const uint32_t *>(answer.data() + sizeof(VisHead));
  for (size_t i = 0; i < nk; ++i) {
    picks[i] = i < head.n_picked ? static_cast<int32_t>(words[i]) : 0;
    pick_gains[i] = i < head.n_picked ? words[nk + i] : 0u;
  }
  *n_picked = static_cast<int32_t>(head.n_picked);
  v->stats.rounds = head.n_picked; v->stats.launches = 3u * static_cast<uint32_t>(k); v->stats.call_ms = ms_since(t_begin);
  return KH_OK;
}

int kh_map_visibility_read_mask(kh_map_visibility * v, uint8_t * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(v);
  if (rc) {return rc;}
  std::vector<uint32_t> words(static_cast<size_t>(vis_mask_words(v->view.width, v->view.height)));
  if (hipMemcpyAsync(words.data(), v->d_mask, mask_bytes(v), hipMemcpyDeviceToHost, v->work.stream) != hipSuccess ||
    hipStreamSynchronize(v->work.stream) != hipSuccess) {return failed(v, "kh_map_visibility_read_mask");}
  const size_t cells = static_cast<size_t>(v->view.width) * static_cast<size_t>(v->view.height);
  for (size_t i = 0; i < cells; ++i) {out[i] = static_cast<uint8_t>((words[i >> 5] >> (i & 31)) & 1u);}
  return KH_OK;
}

int kh_map_visibility_stats_get(kh_map_visibility * v, kh_map_visibility_stats * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(v);
  if (rc) {return rc;}
  *out = v->stats;
  return KH_OK;
}

}  // extern "C"
