// The live occupancy map of a mapper (kh_live_map_*): pass / hit / cell grids that stay on the mapper's device and are brought up
// to date by the DIFFERENCE between the scans the map holds and the scans the mapper holds now, instead of a fresh
// OccupancyGrid::CreateFromScans over all of them (kh_mapper_build_map) at every map_update_interval.
//
// The counters are integer sums over beams, so a scan leaves the map exactly as it entered it -- provided the same cells are
// walked.  The map therefore keeps a log of what it traced (the end cell and two flags per beam, the sensor cell per scan) on a
// lattice that never moves: a fixed anchor and resolution, with a window of cells that grows in blocks.  DESIGN.md section 7b
// states the lattice, the window rule, the log and the rebuild policy.
//
// The host's rules -- classification of the mapper's scans against the log (new / gone / moved), the window, the log's slots, the
// touched rectangle, the feed's tile job -- are plain functions in live_map_plan.hpp, checked on the CPU by
// tests/test_live_map_plan.py.  This file is what needs the device: kh_live_map_update plans with them and then runs its stages
// (re-layout, log, records, launch, commit), kh_map_feed_poll likewise; each states its failure rule at its top.  The kernels are
// in occupancy_live.hip (k_occ_trace_delta, k_occ_update_rect, k_nav_feed).
//
// The map feed (kh_map_feed_*) is at the end: the published grid of one consumer, the pending region the
// updates leave it, and the poll that hands out the 16 x 16 tiles whose nav values changed.  After it the distance fields that
// follow the live map (kh_live_map_field_*): the same pending region, handed to kh_map_field_update.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "occupancy_device.hpp"
#include "live_map_plan.hpp"
#include "mapper_internal.hpp"

using namespace kh;

namespace
{
constexpr double kDefaultRebuildFraction = 0.5;      // provisional: the crossover has not been measured yet
}

struct kh_live_map
{
  kh_mapper * mapper = nullptr;
  int32_t device = 0;
  kh_laser laser;
  Lattice lat;
  double resolution = 0.05, rebuild_fraction = kDefaultRebuildFraction;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  LiveWindow win = {0, 0, 0, 0, 0, nullptr, nullptr, nullptr};
  int32_t * d_log = nullptr; size_t cap_log = 0;             // capacity in bytes, whole slots
  HostLog log;                               // the host's copy: who is in the map, in which slot, traced at which pose
  DeltaRecord * d_records = nullptr; size_t cap_records = 0;             // capacity in bytes
  unsigned long long * d_counters = nullptr;
  bool have_params = false; uint32_t min_pass = 0; double threshold = 0.0;
  bool all_cells_stale = true;               // the next update runs the cell-state kernel over the whole window
  bool counters_suspect = false;             // an update failed half-way: the next one rebuilds
  kh_live_map_stats_t stats;
  std::vector<kh_map_feed *> feeds;          // the feeds attached (they borrow the live map); none: nothing below looks at them
  // a distance field that follows the map, and its pending region in lattice cells (as a feed's)
  struct Follower {kh_map_field * field; bool pending_whole; Rect pending;};
  std::vector<Follower> fields;
};

struct kh_map_feed
{
  kh_live_map * live = nullptr;              // nullptr once the live map has been destroyed under the feed
  int32_t device = 0;
  Rect window;                               // the window the published grid covers; its row stride is the window's width
  int8_t * d_pub = nullptr;
  // the pending region in lattice cells: the whole window, or the union of what the updates handed over (empty = nothing)
  bool pending_whole = true;
  Rect pending;
  uint32_t * d_count = nullptr;
  int32_t * d_xy = nullptr; size_t cap_xy = 0;               // capacities in bytes
  uint32_t * d_packed = nullptr; size_t cap_packed = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::vector<int32_t> tile_xy, raw_xy;      // the last poll's tiles in ascending (ty, tx) order / as the kernel dealt the slots
  std::vector<int8_t> data, raw_data;
  kh_map_feed_delta_t last;
  kh_map_feed_stats_t stats;
};

namespace
{
void free_window(LiveWindow & w)
{
  (void)hipFree(w.pass); (void)hipFree(w.hits); (void)hipFree(w.cells);
  w.pass = nullptr; w.hits = nullptr; w.cells = nullptr;
}

// A plane for a window that grew: ws x height elements of `elem` bytes filled with byte `fill`, the old plane (old_w x old_h
// elements, row stride old_ws; nullptr = there is none to keep) copied in at column dx, row dy -- all queued on `stream`.  The
// caller synchronises once and swaps only after everything succeeded.  hipErrorOutOfMemory = the allocation failed.
hipError_t new_plane(hipStream_t stream, void ** out, size_t ws, size_t height, size_t elem, int fill, const void * old, size_t old_ws,
  size_t old_w, size_t old_h, size_t dx, size_t dy)
{
  *out = nullptr;
  if (hipMalloc(out, ws * height * elem) != hipSuccess) {(void)hipGetLastError(); *out = nullptr; return hipErrorOutOfMemory;}
  hipError_t err = hipMemsetAsync(*out, fill, ws * height * elem, stream);
  if (err == hipSuccess && old && old_w > 0 && old_h > 0) {
    err = hipMemcpy2DAsync(static_cast<char *>(*out) + (dx + dy * ws) * elem, ws * elem, old, old_ws * elem, old_w * elem, old_h,
        hipMemcpyDeviceToDevice, stream);
  }
  return err;
}

int fail_hip(hipStream_t stream, const char * who, const char * what)
{
  const hipError_t err = hipGetLastError();
  (void)hipStreamSynchronize(stream);
  set_error(std::string(who) + ": " + what + ": " + hipGetErrorString(err));
  return KH_ERR_HIP;
}

// ---------------------------------------------------------------- the stages of kh_live_map_update

// The one statement of "after a failure past the point of no return the next update rebuilds": alive from the first thing queued
// on the map's own arrays to the commit.
struct RebuildNextUnlessCommitted
{
  kh_live_map * g;
  bool committed = false;
  ~RebuildNextUnlessCommitted() {if (!committed) {g->counters_suspect = true;}}
};

// what the device stages leave for the commit
struct Traced
{
  std::vector<DeltaRecord> records;          // the delta table (it outlives the copy that reads it)
  unsigned long long counters[2] = {0, 0};
  float ms = 0.f;
  bool relayout = false, given_whole = false;
  Rect given;                                // the cells handed to the cell-state kernel, window columns and rows
  int64_t cells_given = 0;
};

// classify, window, slots: on the plan alone.  A refusal leaves the map untouched.
int plan_stage(const kh_live_map * g, const std::vector<SensorView> & views, UpdatePlan & plan)
{
  if (!plan_update(g->lat, views, g->log, rect_of(g->win), g->counters_suspect, g->rebuild_fraction, plan)) {
    set_error("kh_live_map_update: scan " + std::to_string(plan.too_far) + " is too far from the anchor for this resolution");
    return KH_ERR_INVALID_ARG;
  }
  if (plan.window != rect_of(g->win) && grid_too_large(plan.window.width(), plan.window.height())) {
    set_error("kh_live_map_update: the window would be " + std::to_string(plan.window.width()) + " x " + std::to_string(plan.window.height()) +
      " cells, beyond the size cap of an occupancy grid");
    return KH_ERR_INVALID_ARG;
  }
  return KH_OK;
}

// The window grew: new arrays, the counters copied to their new place (a rebuild starts from zero, and the cell states are
// computed anew either way).  A failure leaves the map as it was.
int relayout_stage(kh_live_map * g, const UpdatePlan & plan, Traced & t)
{
  if (plan.window == rect_of(g->win)) {return KH_OK;}
  const LiveWindow & old = g->win;
  LiveWindow w;
  w.ox = static_cast<int32_t>(plan.window.x0); w.oy = static_cast<int32_t>(plan.window.y0);
  w.width = static_cast<int32_t>(plan.window.width()); w.height = static_cast<int32_t>(plan.window.height()); w.ws = (w.width + 7) & ~7;
  w.pass = nullptr; w.hits = nullptr; w.cells = nullptr;
  const bool keep = old.width > 0 && !plan.rebuild;
  const size_t ws = static_cast<size_t>(w.ws), height = static_cast<size_t>(w.height), old_ws = static_cast<size_t>(old.ws);
  const size_t old_w = static_cast<size_t>(old.width), old_h = static_cast<size_t>(old.height);
  const size_t dx = static_cast<size_t>(old.ox - w.ox), dy = static_cast<size_t>(old.oy - w.oy);
  hipError_t err = new_plane(g->stream, reinterpret_cast<void **>(&w.pass), ws, height, 4, 0, keep ? old.pass : nullptr, old_ws, old_w, old_h, dx, dy);
  if (err == hipSuccess) {err = new_plane(g->stream, reinterpret_cast<void **>(&w.hits), ws, height, 4, 0, keep ? old.hits : nullptr, old_ws, old_w, old_h, dx, dy);}
  if (err == hipSuccess) {err = new_plane(g->stream, reinterpret_cast<void **>(&w.cells), ws, height, 1, 0, nullptr, 0, 0, 0, 0, 0);}
  if (err == hipSuccess) {err = hipStreamSynchronize(g->stream);}
  if (err != hipSuccess) {
    int rc = KH_ERR_HIP;
    if (err == hipErrorOutOfMemory) {
      (void)hipStreamSynchronize(g->stream);
      set_error("kh_live_map_update: window allocation failed");
    } else {
      rc = fail_hip(g->stream, "kh_live_map_update", "relayout");
    }
    free_window(w);
    return rc;
  }
  free_window(g->win);
  g->win = w;
  g->all_cells_stale = true;
  t.relayout = true;
  return KH_OK;
}

// room in the log for the slots the plan dealt; what the log holds is kept unless a rebuild forgets it
int log_stage(kh_live_map * g, const UpdatePlan & plan)
{
  const size_t slot_bytes = static_cast<size_t>(live_log_slot_words(g->laser.n_beams)) * 4;
  const size_t slots = static_cast<size_t>(plan.next_slot), cap = std::max<size_t>(slots + slots / 2, 64);
  const size_t used = plan.rebuild ? 0 : static_cast<size_t>(g->log.next_slot) * slot_bytes;
  const hipError_t err = grow_device_keeping(reinterpret_cast<void **>(&g->d_log), &g->cap_log, slots * slot_bytes, cap * slot_bytes, used);
  if (err == hipErrorOutOfMemory) {set_error("kh_live_map_update: log allocation failed"); return KH_ERR_HIP;}
  return err == hipSuccess ? KH_OK : fail_hip(g->stream, "kh_live_map_update", "log copy");
}

// residency of what will be read, and the delta table on the device: SUB, MOVE, ADD
int records_stage(kh_live_map * g, const UpdatePlan & plan, Traced & t)
{
  std::vector<int32_t> read_ids;
  for (const Change & c : plan.moved) {read_ids.push_back(c.id);}
  for (const Change & c : plan.added) {read_ids.push_back(c.id);}
  std::vector<ResidentScan> resident;
  int64_t up_points = 0, up_ranges = 0;
  const int rc = mapper_resident_table_of(g->mapper, g->stream, "kh_live_map_update", read_ids.data(), read_ids.size(), resident, &up_points, &up_ranges);
  if (rc) {(void)hipStreamSynchronize(g->stream); return rc;}
  std::vector<DeltaRecord> & records = t.records;
  records.reserve(plan.gone.size() + read_ids.size());
  size_t k = 0;                              // of `resident`: the moved scans, then the added ones
  auto record = [&](int32_t kind, int32_t slot, const Change * c) {
    DeltaRecord r;
    std::memset(&r, 0, sizeof(r));
    r.kind = kind; r.slot = slot;
    if (c) {
      r.points = resident[k].points; r.ranges = resident[k].ranges; ++k;
      r.sx = c->view->sensor[0]; r.sy = c->view->sensor[1];
    }
    records.push_back(r);
  };
  if (!plan.rebuild) {for (int32_t id : plan.gone) {record(kDeltaSub, g->log.entries[static_cast<size_t>(id)].slot, nullptr);}}
  for (const Change & c : plan.moved) {
    const Entry & e = g->log.entries[static_cast<size_t>(c.id)];
    record(kDeltaMove, e.slot, &c);
    records.back().old_cx = e.cx; records.back().old_cy = e.cy;
  }
  for (size_t a = 0; a < plan.added.size(); ++a) {record(kDeltaAdd, plan.new_slots[a], &plan.added[a]);}
  const size_t bytes = records.size() * sizeof(DeltaRecord);
  if (!grow_device(g->stream, reinterpret_cast<void **>(&g->d_records), &g->cap_records, bytes, bytes + bytes / 2)) {
    set_error("kh_live_map_update: delta table allocation failed");
    return KH_ERR_HIP;
  }
  if (bytes > 0 && hipMemcpyAsync(g->d_records, records.data(), bytes, hipMemcpyHostToDevice, g->stream) != hipSuccess) {
    return fail_hip(g->stream, "kh_live_map_update", "delta table upload");
  }
  return KH_OK;
}

// the trace, then the cell states over the whole window or the rectangle the delta can have touched; returns once both have run
int launch_stage(kh_live_map * g, const UpdatePlan & plan, uint32_t min_pass_through, double occupancy_threshold, Traced & t)
{
  const LiveWindow & w = g->win;
  const size_t size = static_cast<size_t>(w.ws) * static_cast<size_t>(w.height);
  if (plan.rebuild && size > 0 && !t.relayout &&
    (hipMemsetAsync(w.pass, 0, size * 4, g->stream) != hipSuccess || hipMemsetAsync(w.hits, 0, size * 4, g->stream) != hipSuccess)) {
    return fail_hip(g->stream, "kh_live_map_update", "clear");
  }
  if (hipMemsetAsync(g->d_counters, 0, 2 * sizeof(unsigned long long), g->stream) != hipSuccess) {return fail_hip(g->stream, "kh_live_map_update", "counters");}
  (void)hipEventRecord(g->ev[0], g->stream);
  live_trace_delta(g->stream, w, g->lat.ax, g->lat.ay, g->lat.scale, g->d_records, static_cast<int32_t>(t.records.size()), g->laser.n_beams,
    g->laser.range_threshold, g->laser.minimum_range, g->laser.maximum_range, g->d_log, g->d_counters);
  (void)hipEventRecord(g->ev[1], g->stream);
  const bool params_changed = !g->have_params || g->min_pass != min_pass_through ||
    std::memcmp(&g->threshold, &occupancy_threshold, sizeof(double)) != 0;
  if (w.width > 0) {
    t.given_whole = g->all_cells_stale || plan.rebuild || params_changed;
    t.given = t.given_whole ? Rect{0, 0, w.ws, w.height} : touched(plan, g->log, g->lat.reach, rect_of(w));
    t.cells_given = t.given.width() * t.given.height();
    live_update_cells(g->stream, w, static_cast<int32_t>(t.given.x0), static_cast<int32_t>(t.given.y0), static_cast<int32_t>(t.given.width()),
      static_cast<int32_t>(t.given.height()), min_pass_through, occupancy_threshold);
  }
  if (hipMemcpyAsync(t.counters, g->d_counters, sizeof(t.counters), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipStreamSynchronize(g->stream) != hipSuccess) {return fail_hip(g->stream, "kh_live_map_update", "trace");}
  (void)hipEventElapsedTime(&t.ms, g->ev[0], g->ev[1]);
  return KH_OK;
}

// the cells an update handed to the cell-state kernel, for everything attached -- feeds and fields: window columns / rows ->
// lattice cells
void followers_pending(kh_live_map * g, const Traced & t)
{
  auto add = [&](bool & whole, Rect & pending) {
    if (t.given_whole) {whole = true; return;}
    pending = pending.join(t.given.moved_by(g->win.ox, g->win.oy));
  };
  for (kh_map_feed * f : g->feeds) {add(f->pending_whole, f->pending);}
  for (kh_live_map::Follower & f : g->fields) {add(f.pending_whole, f.pending);}
}

// the update has happened: the host's copy of the log, the parameters, the feeds and the stats follow
void commit_stage(kh_live_map * g, const std::vector<SensorView> & views, const UpdatePlan & plan, const Traced & t, uint32_t min_pass_through,
  double occupancy_threshold)
{
  commit(g->log, views, plan);
  g->have_params = true; g->min_pass = min_pass_through; g->threshold = occupancy_threshold;
  g->all_cells_stale = false; g->counters_suspect = false;
  if (t.cells_given > 0) {followers_pending(g, t);}
  kh_live_map_counts & last = g->stats.last;
  std::memset(&last, 0, sizeof(last));
  last.scans_added = plan.n_added; last.scans_removed = static_cast<int64_t>(plan.gone.size()); last.scans_moved = plan.n_moved;
  last.beams_traced = static_cast<int64_t>(t.counters[0]); last.beams_skipped = static_cast<int64_t>(t.counters[1]);
  last.cells_updated = t.cells_given; last.relayouts = t.relayout ? 1 : 0; last.rebuilds = plan.rebuild ? 1 : 0;
  last.trace_ms = t.records.size() == 0 ? 0.0 : static_cast<double>(t.ms);
  kh_live_map_counts & total = g->stats.total;
  total.scans_added += last.scans_added; total.scans_removed += last.scans_removed; total.scans_moved += last.scans_moved;
  total.beams_traced += last.beams_traced; total.beams_skipped += last.beams_skipped; total.cells_updated += last.cells_updated;
  total.relayouts += last.relayouts; total.rebuilds += last.rebuilds; total.trace_ms += last.trace_ms;
  g->stats.updates += 1;
  g->stats.scans_in_map = static_cast<int64_t>(g->log.logged.size());
  g->stats.log_bytes = static_cast<int64_t>(g->cap_log);
}
}  // namespace

extern "C" {

int kh_live_map_create(kh_mapper * m, double resolution, const double anchor[2], double rebuild_fraction, kh_live_map ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (!(resolution > 0) || !std::isfinite(resolution) || rebuild_fraction != rebuild_fraction) {
    set_error("kh_live_map_create: the resolution must be positive and finite, the rebuild fraction a number");
    return KH_ERR_INVALID_ARG;
  }
  if (anchor && !(std::isfinite(anchor[0]) && std::isfinite(anchor[1]))) {
    set_error("kh_live_map_create: the anchor must be finite");
    return KH_ERR_INVALID_ARG;
  }
  double ax, ay;
  if (anchor) {
    ax = anchor[0]; ay = anchor[1];
  } else {
    // the offset kh_mapper_build_map would choose now: the minimum of the boxes of the scans still in the map
    std::vector<SensorView> views;
    mapper_sensor_poses(m, views);
    if (views.empty()) {set_error("kh_live_map_create: the default anchor needs a scan in the map"); return KH_ERR_INVALID_ARG;}
    ax = 999999999999999999.99999; ay = 999999999999999999.99999;
    for (const SensorView & v : views) {ax = v.bbox[0] < ax ? v.bbox[0] : ax; ay = v.bbox[1] < ay ? v.bbox[1] : ay;}
  }
  const int32_t device = mapper_device(m);
  if (require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_live_map * g = new kh_live_map();
  g->mapper = m; g->device = device; g->laser = mapper_laser(m);
  g->lat.ax = ax; g->lat.ay = ay; g->resolution = resolution; g->lat.scale = 1.0 / resolution;
  g->rebuild_fraction = rebuild_fraction < 0 ? kDefaultRebuildFraction : rebuild_fraction;
  g->lat.reach = reach_of(g->laser.range_threshold, g->lat.scale);
  std::memset(&g->stats, 0, sizeof(g->stats));
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
    hipEventCreate(&g->ev[0]) != hipSuccess || hipEventCreate(&g->ev[1]) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&g->d_counters), 2 * sizeof(unsigned long long)) != hipSuccess)
  {
    set_error("kh_live_map_create: HIP allocation failed");
    kh_live_map_destroy(g);
    return KH_ERR_HIP;
  }
  *out = g;
  return KH_OK;
}

void kh_live_map_destroy(kh_live_map * g)
{
  if (!g) {return;}
  (void)hipSetDevice(g->device);
  if (g->stream) {(void)hipStreamSynchronize(g->stream);}
  for (kh_map_feed * f : g->feeds) {f->live = nullptr;}         // (feeds are to be destroyed first; one that was not must not follow us)
  for (kh_live_map::Follower & f : g->fields) {map_field_set_live(f.field, nullptr);}      // (a field stays readable)
  free_window(g->win);
  (void)hipFree(g->d_log); (void)hipFree(g->d_records); (void)hipFree(g->d_counters);
  if (g->ev[0]) {(void)hipEventDestroy(g->ev[0]);}
  if (g->ev[1]) {(void)hipEventDestroy(g->ev[1]);}
  if (g->stream) {(void)hipStreamDestroy(g->stream);}
  delete g;
}

// The failure rule.  Up to and including the re-layout a failure -- a scan too far from the anchor, the size cap, hipSetDevice, the
// window's allocation or a re-layout that does not complete -- leaves window, counters, cells, log and stats untouched: the plan is
// worked out beside the map, and the new window is swapped in only once it is complete.  After any later failure the next update
// rebuilds (RebuildNextUnlessCommitted).  The host's copy of the log changes in the commit stage alone.
int kh_live_map_update(kh_live_map * g, uint32_t min_pass_through, double occupancy_threshold)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (g->laser.n_beams <= 0) {set_error("kh_live_map_update: the laser has no beams"); return KH_ERR_INVALID_ARG;}
  std::vector<SensorView> views;
  mapper_sensor_poses(g->mapper, views);
  UpdatePlan plan;
  Traced traced;
  int rc = plan_stage(g, views, plan);
  if (rc != KH_OK) {return rc;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  if ((rc = relayout_stage(g, plan, traced)) != KH_OK) {return rc;}
  RebuildNextUnlessCommitted guard{g};
  if ((rc = log_stage(g, plan)) != KH_OK) {return rc;}
  if ((rc = records_stage(g, plan, traced)) != KH_OK) {return rc;}
  if ((rc = launch_stage(g, plan, min_pass_through, occupancy_threshold, traced)) != KH_OK) {return rc;}
  commit_stage(g, views, plan, traced, min_pass_through, occupancy_threshold);
  guard.committed = true;
  return KH_OK;
}

int kh_live_map_info(const kh_live_map * g, kh_live_map_info_t * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  out->anchor[0] = g->lat.ax; out->anchor[1] = g->lat.ay; out->resolution = g->resolution; out->rebuild_fraction = g->rebuild_fraction;
  out->ox = g->win.ox; out->oy = g->win.oy; out->width = g->win.width; out->height = g->win.height; out->width_step = g->win.ws;
  out->reach = static_cast<int32_t>(std::min<int64_t>(g->lat.reach, INT32_MAX));
  return KH_OK;
}

int kh_live_map_read(kh_live_map * g, uint8_t * cells, uint32_t * pass, uint32_t * hits)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t size = static_cast<size_t>(g->win.ws) * static_cast<size_t>(g->win.height);
  if (size == 0) {return KH_OK;}
  if (cells && hipMemcpy(cells, g->win.cells, size, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  if (pass && hipMemcpy(pass, g->win.pass, size * 4, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  if (hits && hipMemcpy(hits, g->win.hits, size * 4, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  return KH_OK;
}

int kh_live_map_stats(const kh_live_map * g, kh_live_map_stats_t * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  *out = g->stats;
  return KH_OK;
}

int kh_live_map_view(kh_live_map * g, kh_map_view * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  if (!g->win.cells || g->win.width <= 0 || g->win.height <= 0) {set_error("kh_live_map_view: the map has no window yet"); return KH_ERR_NOT_FOUND;}
  out->device_cells = g->win.cells; out->device = g->device;
  out->width = g->win.width; out->height = g->win.height; out->width_step = g->win.ws;
  out->ox = g->win.ox; out->oy = g->win.oy;
  out->anchor[0] = g->lat.ax; out->anchor[1] = g->lat.ay; out->scale = g->lat.scale;
  return KH_OK;
}

// ---------------------------------------------------------------- the map feed

namespace
{
// The one statement of "after a failure the whole window is pending".
struct WholePendingUnlessDone
{
  kh_map_feed * f;
  bool done = false;
  ~WholePendingUnlessDone() {if (!done) {f->pending_whole = true;}}
};

int finish_poll(kh_map_feed * f, kh_map_feed_delta_t * out)
{
  kh_map_feed_delta_t & d = f->last;
  d.ox = static_cast<int32_t>(f->window.x0); d.oy = static_cast<int32_t>(f->window.y0);
  d.width = static_cast<int32_t>(f->window.width()); d.height = static_cast<int32_t>(f->window.height());
  f->stats.polls += 1; f->stats.n_tiles += d.n_tiles; f->stats.tiles_scanned += d.tiles_scanned;
  f->stats.bytes_downloaded += d.bytes_downloaded; f->stats.kernel_ms += d.kernel_ms;
  *out = d;
  return KH_OK;
}

// the published grid follows the window: a new array of -1, the old content at its place
int follow_window_stage(kh_map_feed * f, const LiveWindow & w)
{
  const Rect now = rect_of(w);
  if (now == f->window) {return KH_OK;}
  hipStream_t stream = f->live->stream;
  void * d_new = nullptr;
  hipError_t err = new_plane(stream, &d_new, static_cast<size_t>(w.width), static_cast<size_t>(w.height), 1, 0xFF, f->d_pub,
      static_cast<size_t>(f->window.width()), static_cast<size_t>(f->window.width()), static_cast<size_t>(f->window.height()),
      static_cast<size_t>(f->window.x0 - now.x0), static_cast<size_t>(f->window.y0 - now.y0));
  if (err == hipErrorOutOfMemory) {set_error("kh_map_feed_poll: published grid allocation failed"); return KH_ERR_HIP;}
  if (err == hipSuccess) {err = hipStreamSynchronize(stream);}
  if (err != hipSuccess) {
    const int rc = fail_hip(stream, "kh_map_feed_poll", "relayout");
    (void)hipFree(d_new);
    return rc;
  }
  (void)hipFree(f->d_pub);
  f->d_pub = static_cast<int8_t *>(d_new); f->window = now;
  f->pending_whole = true;                   // (a window that grew was given to the cell-state kernel whole: this restates it)
  return KH_OK;
}

// compare and pack the job's tiles; the count, then that many coordinates and tiles come down as the kernel dealt them
int compare_stage(kh_map_feed * f, const LiveWindow & w, const Rect & tiles, size_t * n, float * ms)
{
  hipStream_t stream = f->live->stream;
  const size_t n_tiles = static_cast<size_t>(tiles.width() * tiles.height());
  if (!grow_device(stream, reinterpret_cast<void **>(&f->d_xy), &f->cap_xy, n_tiles * 2 * sizeof(int32_t), n_tiles * 2 * sizeof(int32_t)) ||
    !grow_device(stream, reinterpret_cast<void **>(&f->d_packed), &f->cap_packed, n_tiles * kTileWords * sizeof(uint32_t), n_tiles * kTileWords * sizeof(uint32_t)))
  {
    set_error("kh_map_feed_poll: tile buffer allocation failed");
    return KH_ERR_HIP;
  }
  NavFeedJob job;
  job.tx0 = static_cast<int32_t>(tiles.x0); job.ty0 = static_cast<int32_t>(tiles.y0);
  job.tx1 = static_cast<int32_t>(tiles.x1); job.ty1 = static_cast<int32_t>(tiles.y1);
  job.cells = w.cells; job.cells_ox = w.ox; job.cells_oy = w.oy; job.cells_ws = w.ws;
  job.published = f->d_pub; job.pub_ox = w.ox; job.pub_oy = w.oy; job.pub_ws = w.width;
  job.count = f->d_count; job.tile_xy = f->d_xy; job.packed = f->d_packed;
  if (hipMemsetAsync(f->d_count, 0, sizeof(uint32_t), stream) != hipSuccess) {return fail_hip(stream, "kh_map_feed_poll", "count");}
  (void)hipEventRecord(f->ev[0], stream);
  nav_feed(stream, job);
  (void)hipEventRecord(f->ev[1], stream);
  uint32_t count = 0;
  if (hipMemcpyAsync(&count, f->d_count, sizeof(count), hipMemcpyDeviceToHost, stream) != hipSuccess ||
    hipStreamSynchronize(stream) != hipSuccess) {return fail_hip(stream, "kh_map_feed_poll", "compare");}
  if (count > n_tiles) {set_error("kh_map_feed_poll: more tiles reported than compared"); return KH_ERR_HIP;}
  (void)hipEventElapsedTime(ms, f->ev[0], f->ev[1]);
  *n = count;
  f->raw_xy.resize(2 * *n); f->raw_data.resize(256 * *n);
  if (*n > 0 && (hipMemcpyAsync(f->raw_xy.data(), f->d_xy, *n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
    hipMemcpyAsync(f->raw_data.data(), f->d_packed, *n * 256, hipMemcpyDeviceToHost, stream) != hipSuccess ||
    hipStreamSynchronize(stream) != hipSuccess)) {return fail_hip(stream, "kh_map_feed_poll", "download");}
  return KH_OK;
}

// the n tiles in ascending (ty, tx) order -- the kernel deals its slots in no order -- and the rectangle of cells that holds them
void sort_stage(kh_map_feed * f, size_t n)
{
  std::vector<uint32_t> order(n);
  for (size_t k = 0; k < n; ++k) {order[k] = static_cast<uint32_t>(k);}
  const int32_t * xy = f->raw_xy.data();
  std::sort(order.begin(), order.end(), [xy](uint32_t a, uint32_t b) {
    return xy[2 * a + 1] != xy[2 * b + 1] ? xy[2 * a + 1] < xy[2 * b + 1] : xy[2 * a] < xy[2 * b];
  });
  f->tile_xy.resize(2 * n); f->data.resize(256 * n);
  Rect box;
  for (size_t k = 0; k < n; ++k) {
    const int32_t tx = xy[2 * order[k]], ty = xy[2 * order[k] + 1];
    f->tile_xy[2 * k] = tx; f->tile_xy[2 * k + 1] = ty;
    std::memcpy(f->data.data() + 256 * k, f->raw_data.data() + 256 * static_cast<size_t>(order[k]), 256);
    box = box.join(Rect{tx, ty, tx + 1, ty + 1});
  }
  kh_map_feed_delta_t & d = f->last;
  d.x = static_cast<int32_t>(box.x0 * kMapTile); d.y = static_cast<int32_t>(box.y0 * kMapTile);
  d.w = static_cast<int32_t>(box.width() * kMapTile); d.h = static_cast<int32_t>(box.height() * kMapTile);
}
}  // namespace

int kh_map_feed_create(kh_live_map * g, kh_map_feed ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!g) {return KH_ERR_INVALID_ARG;}
  kh_map_feed * f = new kh_map_feed();
  f->live = g; f->device = g->device;
  std::memset(&f->last, 0, sizeof(f->last));
  std::memset(&f->stats, 0, sizeof(f->stats));
  if (hipSetDevice(f->device) != hipSuccess || hipEventCreate(&f->ev[0]) != hipSuccess || hipEventCreate(&f->ev[1]) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&f->d_count), sizeof(uint32_t)) != hipSuccess)
  {
    (void)hipGetLastError();
    set_error("kh_map_feed_create: HIP allocation failed");
    kh_map_feed_destroy(f);
    return KH_ERR_HIP;
  }
  g->feeds.push_back(f);
  *out = f;
  return KH_OK;
}

void kh_map_feed_destroy(kh_map_feed * f)
{
  if (!f) {return;}
  (void)hipSetDevice(f->device);
  if (f->live) {
    (void)hipStreamSynchronize(f->live->stream);
    std::vector<kh_map_feed *> & feeds = f->live->feeds;
    feeds.erase(std::remove(feeds.begin(), feeds.end(), f), feeds.end());
  }
  (void)hipFree(f->d_pub); (void)hipFree(f->d_count); (void)hipFree(f->d_xy); (void)hipFree(f->d_packed);
  if (f->ev[0]) {(void)hipEventDestroy(f->ev[0]);}
  if (f->ev[1]) {(void)hipEventDestroy(f->ev[1]);}
  delete f;
}

// The failure rule.  A poll that is refused before it uses the device (a destroyed live map, a window that is not whole blocks or
// that shrank) leaves the feed as it was.  After any later failure the whole window is pending (WholePendingUnlessDone): the next
// poll compares everything, and the consumer misses nothing.
int kh_map_feed_poll(kh_map_feed * f, kh_map_feed_delta_t * out)
{
  if (!f || !out) {return KH_ERR_INVALID_ARG;}
  kh_live_map * g = f->live;
  if (!g) {set_error("kh_map_feed_poll: the feed's live map has been destroyed"); return KH_ERR_INVALID_ARG;}
  std::memset(&f->last, 0, sizeof(f->last));
  f->tile_xy.clear(); f->data.clear();
  const LiveWindow & w = g->win;
  if (w.width == 0 || !(f->pending_whole || !f->pending.empty())) {return finish_poll(f, out);}
  // what the tile rule stands on: no tile straddles the window's edge, and the cells have no row padding
  if (w.ox % kBlock || w.oy % kBlock || w.width % kBlock || w.height % kBlock || w.ws != w.width) {
    set_error("kh_map_feed_poll: the live window is not made of whole 64-cell blocks without row padding");
    return KH_ERR_INVALID_ARG;
  }
  if (!rect_of(w).contains(f->window)) {set_error("kh_map_feed_poll: the live window shrank"); return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(f->device) != hipSuccess) {return KH_ERR_HIP;}
  WholePendingUnlessDone guard{f};
  int rc = follow_window_stage(f, w);
  if (rc != KH_OK) {return rc;}
  const Rect tiles = tile_job(f->pending_whole, f->pending, f->window);
  size_t n = 0;
  float ms = 0.f;
  if (!tiles.empty()) {
    if ((rc = compare_stage(f, w, tiles, &n, &ms)) != KH_OK) {return rc;}
    sort_stage(f, n);
    kh_map_feed_delta_t & d = f->last;
    d.n_tiles = static_cast<int64_t>(n); d.tiles_scanned = tiles.width() * tiles.height();
    d.bytes_downloaded = static_cast<int64_t>(sizeof(uint32_t) + n * (2 * sizeof(int32_t) + 256));
    d.kernel_ms = static_cast<double>(ms);
  }
  f->pending_whole = false; f->pending = Rect{};
  guard.done = true;
  return finish_poll(f, out);
}

int kh_map_feed_tiles(const kh_map_feed * f, int32_t * tile_xy, int8_t * data)
{
  if (!f) {return KH_ERR_INVALID_ARG;}
  if (tile_xy && !f->tile_xy.empty()) {std::memcpy(tile_xy, f->tile_xy.data(), f->tile_xy.size() * sizeof(int32_t));}
  if (data && !f->data.empty()) {std::memcpy(data, f->data.data(), f->data.size());}
  return KH_OK;
}

int kh_map_feed_read(kh_map_feed * f, int32_t x, int32_t y, int32_t w, int32_t h, int8_t * out)
{
  if (!f || w < 0 || h < 0 || static_cast<int64_t>(w) * h > INT32_MAX) {return KH_ERR_INVALID_ARG;}
  if (w == 0 || h == 0) {return KH_OK;}
  if (!out) {return KH_ERR_INVALID_ARG;}
  std::memset(out, 0xFF, static_cast<size_t>(w) * static_cast<size_t>(h));
  const Rect asked{x, y, static_cast<int64_t>(x) + w, static_cast<int64_t>(y) + h}, got = asked.clip(f->window);
  if (got.empty()) {return KH_OK;}
  if (hipSetDevice(f->device) != hipSuccess) {return KH_ERR_HIP;}
  const int8_t * src = f->d_pub + (got.x0 - f->window.x0) + (got.y0 - f->window.y0) * f->window.width();
  int8_t * dst = out + (got.x0 - x) + (got.y0 - y) * static_cast<int64_t>(w);
  if (hipMemcpy2D(dst, static_cast<size_t>(w), src, static_cast<size_t>(f->window.width()), static_cast<size_t>(got.width()),
      static_cast<size_t>(got.height()), hipMemcpyDeviceToHost) != hipSuccess)
  {
    set_error(std::string("kh_map_feed_read: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  return KH_OK;
}

int kh_map_feed_stats(const kh_map_feed * f, kh_map_feed_stats_t * out)
{
  if (!f || !out) {return KH_ERR_INVALID_ARG;}
  *out = f->stats;
  return KH_OK;
}

// ---------------------------------------------------------------- the fields that follow the live map

int kh_live_map_field_create(kh_live_map * g, const kh_map_field_params * params, kh_map_field ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (!params) {return KH_ERR_INVALID_ARG;}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!g) {return KH_ERR_INVALID_ARG;}
  kh_map_view view;
  int rc = kh_live_map_view(g, &view);
  if (rc != KH_OK) {return rc;}
  kh_map_field * f = nullptr;
  if ((rc = map_field_create_empty(view, *params, "kh_live_map_field_create", &f)) != KH_OK) {return rc;}
  if ((rc = kh_map_field_update(f, &view, nullptr, nullptr)) != KH_OK) {kh_map_field_destroy(f); return rc;}
  map_field_set_live(f, g);
  g->fields.push_back(kh_live_map::Follower{f, false, Rect{}});
  *out = f;
  return KH_OK;
}

// A sync that fails leaves the region pending; the field's own failure rule (kh_map_field_update) makes its next update a rebuild.
int kh_live_map_field_sync(kh_map_field * f, kh_field_update * out)
{
  if (out) {std::memset(out, 0, sizeof(*out));}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_live_map * const g = f ? map_field_live(f) : nullptr;
  if (!g) {set_error("kh_live_map_field_sync: the field follows no live map (never attached, or the live map has been destroyed)"); return KH_ERR_INVALID_ARG;}
  auto it = std::find_if(g->fields.begin(), g->fields.end(), [f](const kh_live_map::Follower & o) {return o.field == f;});
  if (it == g->fields.end()) {return KH_ERR_INVALID_ARG;}
  if (!it->pending_whole && it->pending.empty()) {return KH_OK;}
  kh_map_view view;
  int rc = kh_live_map_view(g, &view);
  if (rc != KH_OK) {return rc;}
  const int32_t rect[4] = {static_cast<int32_t>(it->pending.x0), static_cast<int32_t>(it->pending.y0), static_cast<int32_t>(it->pending.width()),
    static_cast<int32_t>(it->pending.height())};
  if ((rc = kh_map_field_update(f, &view, it->pending_whole ? nullptr : rect, out)) != KH_OK) {return rc;}
  it->pending_whole = false; it->pending = Rect{};
  return KH_OK;
}

}  // extern "C"

void kh::live_map_forget_field(kh_live_map * g, kh_map_field * f)
{
  std::vector<kh_live_map::Follower> & fields = g->fields;
  fields.erase(std::remove_if(fields.begin(), fields.end(), [f](const kh_live_map::Follower & o) {return o.field == f;}), fields.end());
}
