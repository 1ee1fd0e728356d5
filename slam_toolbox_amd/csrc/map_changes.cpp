// The map change layer (kh_map_changes_*): what the scans of a robot that holds only a map say about that map
// -- per beam (explained, novel, through something solid), per cell (confirmed, appeared, vanished, discovered) and as the patched
// map, a kh_map_view of its own.  The handle owns the layer's two counter grids, the codes and patched cells of the last diff and the
// staging of a call; the kernels and their launchers are occupancy_changes.hip's, the rules that need no device map_changes_plan.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "map_changes_plan.hpp"
#include "occupancy_device.hpp"

using namespace kh;

struct kh_map_changes
{
  kh_map_view view;                    // the map: a copy of the struct, the cells borrowed
  DeviceWork work;                     // the stream, the events around a call's first kernel, a call's tables and answers
  hipEvent_t ev[2] = {nullptr, nullptr};       // a diff's third and fourth event
  ChangeLayer layer = {nullptr, nullptr};
  uint8_t * d_codes = nullptr;         // the last diff's codes ...
  uint8_t * d_patched = nullptr;       // ... and patched cells, both on the strided window
  int32_t * d_unit = nullptr;          // the changed-cell list's units: change_units() + 1 words
  unsigned long long * d_counts = nullptr;     // kChangeCodes
  bool has_diff = false;
  uint64_t bound = 0;                  // no cell of the layer holds more (map_changes_plan.hpp)
  int64_t scans = 0, beams = 0;        // observed since the last clear
  double observe_ms = 0.0;
  size_t size() const {return static_cast<size_t>(view.width_step) * static_cast<size_t>(view.height);}
};

namespace
{
int failed(kh_map_changes * c, const char * who)
{
  (void)hipStreamSynchronize(c->work.stream);
  set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return KH_ERR_HIP;
}

double between(hipEvent_t a, hipEvent_t b)
{
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  return ms;
}

// what every call on a handle begins with once its own arguments are judged: the device, then the handle
int enter(kh_map_changes * c)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!c) {return KH_ERR_INVALID_ARG;}
  return hipSetDevice(c->view.device) == hipSuccess ? KH_OK : KH_ERR_HIP;
}

int zero_layer(kh_map_changes * c)
{
  if (hipMemsetAsync(c->layer.pass, 0, c->size() * 4, c->work.stream) != hipSuccess || hipMemsetAsync(c->layer.hits, 0, c->size() * 4, c->work.stream) != hipSuccess ||
    hipStreamSynchronize(c->work.stream) != hipSuccess)
  {
    return failed(c, "kh_map_changes_clear");
  }
  c->bound = 0; c->scans = 0; c->beams = 0; c->observe_ms = 0.0;
  return KH_OK;
}
}  // namespace

extern "C" {

int kh_map_changes_create(const kh_map_view * view, kh_map_changes ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (map_view_check(view) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (view->device < 0) {set_error("kh_map_changes_create: the view names no device"); return KH_ERR_INVALID_ARG;}
  if (require_device(view->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_map_changes * c = new kh_map_changes();
  c->view = *view;
  const size_t size = c->size();
  const size_t unit_bytes = static_cast<size_t>(change_units(view->width, view->height) + 1) * sizeof(int32_t);
  if (!work_open(c->work, view->device) || hipEventCreate(&c->ev[0]) != hipSuccess || hipEventCreate(&c->ev[1]) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&c->layer.pass), size * 4) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&c->layer.hits), size * 4) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&c->d_codes), size) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&c->d_patched), size) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&c->d_unit), unit_bytes) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&c->d_counts), kChangeCodes * sizeof(unsigned long long)) != hipSuccess ||
    hipMemsetAsync(c->d_codes, 0, size, c->work.stream) != hipSuccess || hipMemsetAsync(c->d_patched, 0, size, c->work.stream) != hipSuccess ||
    hipMemsetAsync(c->d_unit, 0, unit_bytes, c->work.stream) != hipSuccess || zero_layer(c) != KH_OK)
  {
    (void)hipGetLastError();
    set_error("kh_map_changes_create: HIP allocation failed");
    kh_map_changes_destroy(c);
    return KH_ERR_HIP;
  }
  *out = c;
  return KH_OK;
}

void kh_map_changes_destroy(kh_map_changes * c)
{
  if (!c) {return;}
  (void)hipSetDevice(c->view.device);
  if (c->work.stream) {(void)hipStreamSynchronize(c->work.stream);}
  (void)hipFree(c->layer.pass); (void)hipFree(c->layer.hits); (void)hipFree(c->d_codes); (void)hipFree(c->d_patched);
  (void)hipFree(c->d_unit); (void)hipFree(c->d_counts);
  for (hipEvent_t e : c->ev) {
    if (e) {(void)hipEventDestroy(e);}
  }
  work_close(c->work);
  delete c;
}

int kh_map_changes_clear(kh_map_changes * c)
{
  const int rc = enter(c);
  return rc ? rc : zero_layer(c);
}

int kh_map_changes_decay(kh_map_changes * c, int32_t shift)
{
  if (!changes_shift_ok(shift)) {set_error("kh_map_changes_decay: 1 <= shift <= 31 is required"); return KH_ERR_INVALID_ARG;}
  const int rc = enter(c);
  if (rc) {return rc;}
  map_decay(c->work.stream, c->view, c->layer, shift);
  if (hipStreamSynchronize(c->work.stream) != hipSuccess) {return failed(c, "kh_map_changes_decay");}
  c->bound = changes_bound_decayed(c->bound, shift);
  return KH_OK;
}

int kh_map_changes_observe(kh_map_changes * c, const kh_laser * laser, int32_t n_scans, const double * ranges, const double * sensor_poses,
  int32_t end_tolerance, int32_t * labels)
{
  if (!changes_observe_args_ok(laser, n_scans, ranges, sensor_poses, end_tolerance)) {
    set_error("kh_map_changes_observe: a laser of numbers, ranges, finite poses, n_scans >= 1 and 0 <= end_tolerance <= 4 are required");
    return KH_ERR_INVALID_ARG;
  }
  int rc = enter(c);
  if (rc) {return rc;}
  const FitInputs walk = changes_observe_walk(*laser, n_scans, sensor_poses, c->view.anchor[0], c->view.anchor[1], c->view.scale);
  if (walk.failed) {
    set_error(fit_inputs_text(walk, "kh_map_changes_observe", "the laser's range_threshold * scale must stay below 2^20 cells of this map",
      "a pose lies more than 2^30 cells from the map's anchor"));
    return KH_ERR_INVALID_ARG;
  }
  const size_t ns = static_cast<size_t>(n_scans), nb = static_cast<size_t>(laser->n_beams);
  uint64_t bound_after = 0;
  if (blocks_per_pose(laser->n_beams, n_scans) == 0 || !changes_bound_after(c->bound, n_scans, laser->n_beams, &bound_after)) {
    set_error("kh_map_changes_observe: a counter of the layer could pass 2^32 - 1 (decay or clear the layer first)");
    return KH_ERR_INVALID_ARG;
  }
  std::vector<double> points(2 * nb * ns), sensor_xy(2 * ns);
  scan_points_at(ranges, nb, laser->n_beams, laser->minimum_angle, laser->angular_resolution, ns, sensor_poses, points.data(), sensor_xy.data());
  // the sensors, the ranges, the points, then the labels: every part a multiple of 8 bytes
  Part parts[] = {{sensor_xy.data(), ns * 2 * sizeof(double)}, {ranges, ns * nb * sizeof(double)}, {points.data(), ns * nb * 2 * sizeof(double)},
    {nullptr, ns * nb * 2 * sizeof(int32_t)}};
  rc = work_stage(c->work, "kh_map_changes_observe", "table", true, parts);
  if (rc) {return rc;}
  double ms = 0.0;
  rc = work_run(c->work, "kh_map_changes_observe", [&] {
    map_observe(c->work.stream, c->view, c->layer, parts[1].as<const double>(), parts[2].as<const double>(), parts[0].as<const double>(), n_scans,
      laser->n_beams, laser->range_threshold, laser->minimum_range, laser->maximum_range, end_tolerance, parts[3].as<int32_t>());
    // (from here on the layer has changed: the bound moves whatever becomes of the download)
    c->bound = bound_after; c->scans += n_scans; c->beams += static_cast<int64_t>(ns * nb);
  }, labels ? &parts[3] : nullptr, labels, &ms);
  if (rc) {return rc;}
  c->observe_ms += ms;
  return KH_OK;
}

int kh_map_changes_diff(kh_map_changes * c, uint32_t min_pass_through, double occupancy_threshold, int32_t * cells, int32_t cap,
  kh_map_changes_summary_t * out)
{
  if (!changes_diff_args_ok(occupancy_threshold, cells, cap, out)) {
    set_error("kh_map_changes_diff: a summary, cap >= 0, room for cap cells and a threshold that is a number are required");
    return KH_ERR_INVALID_ARG;
  }
  std::memset(out, 0, sizeof(*out));
  const int rc = enter(c);
  if (rc) {return rc;}
  const size_t list_bytes = static_cast<size_t>(cap) * 3 * sizeof(int32_t);
  if (!grow_device(c->work.stream, reinterpret_cast<void **>(&c->work.d), &c->work.cap, list_bytes, list_bytes)) {
    set_error("kh_map_changes_diff: list allocation failed");
    return KH_ERR_HIP;
  }
  int32_t * const d_list = reinterpret_cast<int32_t *>(c->work.d);
  const int64_t n_units = change_units(c->view.width, c->view.height);
  unsigned long long counts[kChangeCodes] = {0, 0, 0, 0, 0, 0};
  int32_t total = 0;
  if (hipMemsetAsync(c->d_counts, 0, sizeof(counts), c->work.stream) != hipSuccess) {return failed(c, "kh_map_changes_diff");}
  (void)hipEventRecord(c->work.ev[0], c->work.stream);
  map_diff(c->work.stream, c->view, c->layer, min_pass_through, occupancy_threshold, c->d_codes, c->d_patched, c->d_counts);
  (void)hipEventRecord(c->work.ev[1], c->work.stream);
  map_changed_cells(c->work.stream, c->view, c->d_codes, c->d_unit, d_list, cap);
  (void)hipEventRecord(c->ev[0], c->work.stream);
  c->has_diff = true;
  if (hipMemcpyAsync(counts, c->d_counts, sizeof(counts), hipMemcpyDeviceToHost, c->work.stream) != hipSuccess ||
    hipMemcpyAsync(&total, c->d_unit + n_units, sizeof(total), hipMemcpyDeviceToHost, c->work.stream) != hipSuccess ||
    hipStreamSynchronize(c->work.stream) != hipSuccess)
  {
    return failed(c, "kh_map_changes_diff");
  }
  // (the list's length is known only now: the second copy takes what was written and no more)
  const int32_t listed = std::min(total, cap);
  if (listed > 0 && hipMemcpyAsync(cells, d_list, static_cast<size_t>(listed) * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->work.stream) != hipSuccess) {
    return failed(c, "kh_map_changes_diff");
  }
  (void)hipEventRecord(c->ev[1], c->work.stream);
  if (hipStreamSynchronize(c->work.stream) != hipSuccess) {return failed(c, "kh_map_changes_diff");}
  out->n_unobserved = static_cast<int64_t>(counts[KH_CELL_UNOBSERVED]); out->n_confirmed = static_cast<int64_t>(counts[KH_CELL_CONFIRMED]);
  out->n_appeared = static_cast<int64_t>(counts[KH_CELL_APPEARED]); out->n_vanished = static_cast<int64_t>(counts[KH_CELL_VANISHED]);
  out->n_discovered_occupied = static_cast<int64_t>(counts[KH_CELL_DISCOVERED_OCCUPIED]);
  out->n_discovered_free = static_cast<int64_t>(counts[KH_CELL_DISCOVERED_FREE]);
  out->n_changed = total; out->n_listed = listed;
  out->scans_observed = c->scans; out->beams_observed = c->beams; out->observe_kernel_ms = c->observe_ms;
  out->diff_kernel_ms = between(c->work.ev[0], c->work.ev[1]); out->list_kernel_ms = between(c->work.ev[1], c->ev[0]); out->download_ms = between(c->ev[0], c->ev[1]);
  return KH_OK;
}

int kh_map_changes_read(kh_map_changes * c, uint32_t * pass, uint32_t * hits, uint8_t * codes, uint8_t * patched)
{
  const int rc = enter(c);
  if (rc) {return rc;}
  const size_t size = c->size();
  if ((pass && hipMemcpyAsync(pass, c->layer.pass, size * 4, hipMemcpyDeviceToHost, c->work.stream) != hipSuccess) ||
    (hits && hipMemcpyAsync(hits, c->layer.hits, size * 4, hipMemcpyDeviceToHost, c->work.stream) != hipSuccess) ||
    (codes && hipMemcpyAsync(codes, c->d_codes, size, hipMemcpyDeviceToHost, c->work.stream) != hipSuccess) ||
    (patched && hipMemcpyAsync(patched, c->d_patched, size, hipMemcpyDeviceToHost, c->work.stream) != hipSuccess) ||
    hipStreamSynchronize(c->work.stream) != hipSuccess)
  {
    return failed(c, "kh_map_changes_read");
  }
  return KH_OK;
}

int kh_map_changes_view(kh_map_changes * c, kh_map_view * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(c);
  if (rc) {return rc;}
  if (!c->has_diff) {set_error("kh_map_changes_view: no diff yet"); return KH_ERR_NOT_FOUND;}
  *out = c->view;
  out->device_cells = c->d_patched;
  return KH_OK;
}

int kh_map_changes_read_nav(kh_map_changes * c, int8_t * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  int rc = enter(c);
  if (rc) {return rc;}
  if (!c->has_diff) {set_error("kh_map_changes_read_nav: no diff yet"); return KH_ERR_NOT_FOUND;}
  const size_t total = static_cast<size_t>(c->view.width) * static_cast<size_t>(c->view.height);
  Part parts[] = {{nullptr, (total + 3) / 4 * 4}};           // (whole dwords are written ...
  rc = work_stage(c->work, "kh_map_changes_read_nav", "output", false, parts);
  if (rc) {return rc;}
  parts[0].bytes = total;                                     // ... and the values downloaded)
  return work_run(c->work, "kh_map_changes_read_nav", [&] {
    cells_to_nav(c->work.stream, c->d_patched, c->view.width, c->view.height, c->view.width_step, parts[0].as<uint32_t>());
  }, &parts[0], out, nullptr);
}

}  // extern "C"
