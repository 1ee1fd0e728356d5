// The live occupancy map of a mapper (kh_live_map_*): pass / hit / cell grids that stay on the mapper's device and are brought up
// to date by the DIFFERENCE between the scans the map holds and the scans the mapper holds now, instead of a fresh
// OccupancyGrid::CreateFromScans over all of them (kh_mapper_build_map) at every map_update_interval.
//
// The counters are integer sums over beams, so a scan leaves the map exactly as it entered it -- provided the same cells are
// walked.  The map therefore keeps a log of what it traced (the end cell and two flags per beam, the sensor cell per scan) on a
// lattice that never moves: a fixed anchor and resolution, with a window of cells that grows in blocks.  DESIGN.md section 7b
// states the lattice, the window rule, the log and the rebuild policy; tests/live_map_rule.py restates the window rule.
//
// This file is the host side: classification of the mapper's scans against the log (new / gone / moved), the window, the log's
// slots, the delta table.  The kernels are in occupancy.hip (k_occ_trace_delta, k_occ_update_rect).
//
// The map feed (kh_map_feed_*) is at the end: the published grid of one consumer, the pending region the
// updates leave it, and the poll that hands out the 16 x 16 tiles whose nav values changed (k_nav_feed, occupancy.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/karto_hip.h"
#include "occupancy_device.hpp"
#include "mapper_internal.hpp"

namespace kh
{
void set_error(const std::string & s);

namespace
{
constexpr int32_t kBlock = 64;              // the window grows in blocks of kBlock x kBlock lattice cells
constexpr int32_t kMargin = 2;              // cells beyond ceil(range_threshold * scale) the window keeps around a sensor cell
constexpr double kDefaultRebuildFraction = 0.5;      // provisional: the crossover has not been measured yet
constexpr double kCellLimit = 1073741824.0;          // |cell index| a scan may have (2^30): index +- reach stays an int32

int32_t floor_block(int64_t c) {return static_cast<int32_t>((c >= 0 ? c / kBlock : -((-c + kBlock - 1) / kBlock)) * kBlock);}

struct Entry
{
  int32_t slot = -1;         // slot of the log, -1 = the scan is not in the map
  int32_t cx = 0, cy = 0;    // the sensor cell the log holds
  double sensor[3] = {0.0, 0.0, 0.0};      // the sensor pose the scan was traced at
};

struct Window {int64_t ox = 0, oy = 0, width = 0, height = 0;};
}  // namespace
}  // namespace kh

using namespace kh;

struct kh_live_map
{
  kh_mapper * mapper = nullptr;
  int32_t device = 0;
  kh_laser laser;
  double ax = 0.0, ay = 0.0, resolution = 0.05, scale = 20.0, rebuild_fraction = kDefaultRebuildFraction;
  int64_t reach = 0;                         // ceil(range_threshold * scale) + kMargin
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  LiveWindow win = {0, 0, 0, 0, 0, nullptr, nullptr, nullptr};
  int32_t * d_log = nullptr; int64_t cap_slots = 0, next_slot = 0;
  std::vector<int32_t> free_slots;
  std::vector<Entry> entries;                // by scan id
  std::vector<int32_t> logged;               // ids of the scans in the map, ascending
  DeltaRecord * d_records = nullptr; size_t cap_records = 0;
  unsigned long long * d_counters = nullptr;
  bool have_params = false; uint32_t min_pass = 0; double threshold = 0.0;
  bool all_cells_stale = true;               // the next update runs the cell-state kernel over the whole window
  bool counters_suspect = false;             // an update failed half-way: the next one rebuilds
  kh_live_map_stats_t stats;
  std::vector<kh_map_feed *> feeds;          // the feeds attached (they borrow the live map); none: nothing below looks at them
};

struct kh_map_feed
{
  kh_live_map * live = nullptr;              // nullptr once the live map has been destroyed under the feed
  int32_t device = 0;
  int32_t ox = 0, oy = 0, width = 0, height = 0;       // the window the published grid covers; its row stride is width
  int8_t * d_pub = nullptr;
  // the pending region in lattice cells: the whole window, or the union [x0, x1) x [y0, y1) of what the updates handed over
  bool pending_whole = true, pending_rect = false;
  int64_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  uint32_t * d_count = nullptr;
  int32_t * d_xy = nullptr; uint32_t * d_packed = nullptr; int64_t cap_tiles = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::vector<int32_t> tile_xy, raw_xy;      // the last poll's tiles in ascending (ty, tx) order / as the kernel dealt the slots
  std::vector<int8_t> data, raw_data;
  kh_map_feed_delta_t last;
  kh_map_feed_stats_t stats;
};

namespace kh
{
namespace
{
bool cell_of(const kh_live_map * g, const double sensor[3], int32_t * cx, int32_t * cy)
{
  // the operations of occ_cell (occupancy.hip): o_to_int(o_round((x - anchor) * scale))
  const double x = round_half_away((sensor[0] - g->ax) * g->scale), y = round_half_away((sensor[1] - g->ay) * g->scale);
  if (!(std::fabs(x) < kCellLimit && std::fabs(y) < kCellLimit)) {return false;}
  *cx = static_cast<int32_t>(x); *cy = static_cast<int32_t>(y);
  return true;
}

void free_window(LiveWindow & w)
{
  (void)hipFree(w.pass); (void)hipFree(w.hits); (void)hipFree(w.cells);
  w.pass = nullptr; w.hits = nullptr; w.cells = nullptr;
}

// the cells an update handed to the cell-state kernel, for every feed attached: window columns / rows -> lattice cells
void feeds_pending(kh_live_map * g, bool whole, int64_t wx0, int64_t wy0, int64_t wx1, int64_t wy1)
{
  for (kh_map_feed * f : g->feeds) {
    if (whole) {f->pending_whole = true; continue;}
    const int64_t x0 = wx0 + g->win.ox, y0 = wy0 + g->win.oy, x1 = wx1 + g->win.ox, y1 = wy1 + g->win.oy;
    if (!f->pending_rect) {f->x0 = x0; f->y0 = y0; f->x1 = x1; f->y1 = y1; f->pending_rect = true; continue;}
    f->x0 = std::min(f->x0, x0); f->y0 = std::min(f->y0, y0); f->x1 = std::max(f->x1, x1); f->y1 = std::max(f->y1, y1);
  }
}

int64_t floor_div(int64_t a, int64_t b) {return a >= 0 ? a / b : -((-a + b - 1) / b);}

int fail_feed(kh_map_feed * f, const char * what)
{
  const hipError_t err = hipGetLastError();
  if (f->live) {(void)hipStreamSynchronize(f->live->stream);}
  set_error(std::string("kh_map_feed_poll: ") + what + ": " + hipGetErrorString(err));
  f->pending_whole = true;
  return KH_ERR_HIP;
}

int fail_hip(kh_live_map * g, const char * what)
{
  (void)hipStreamSynchronize(g->stream);
  set_error(std::string("kh_live_map_update: ") + what + ": " + hipGetErrorString(hipGetLastError()));
  g->counters_suspect = true;
  return KH_ERR_HIP;
}
}  // namespace
}  // namespace kh

extern "C" {

int kh_live_map_create(kh_mapper * m, double resolution, const double anchor[2], double rebuild_fraction, kh_live_map ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    kh::set_error("no usable HIP device (libkartohip has no CPU fallback)");
    return KH_ERR_NO_DEVICE;
  }
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (!(resolution > 0) || !std::isfinite(resolution) || rebuild_fraction != rebuild_fraction) {
    kh::set_error("kh_live_map_create: the resolution must be positive and finite, the rebuild fraction a number");
    return KH_ERR_INVALID_ARG;
  }
  if (anchor && !(std::isfinite(anchor[0]) && std::isfinite(anchor[1]))) {
    kh::set_error("kh_live_map_create: the anchor must be finite");
    return KH_ERR_INVALID_ARG;
  }
  double ax, ay;
  if (anchor) {
    ax = anchor[0]; ay = anchor[1];
  } else {
    // the offset kh_mapper_build_map would choose now: the minimum of the boxes of the scans still in the map
    std::vector<SensorView> views;
    kh::mapper_sensor_poses(m, views);
    if (views.empty()) {kh::set_error("kh_live_map_create: the default anchor needs a scan in the map"); return KH_ERR_INVALID_ARG;}
    ax = 999999999999999999.99999; ay = 999999999999999999.99999;
    for (const SensorView & v : views) {ax = v.bbox[0] < ax ? v.bbox[0] : ax; ay = v.bbox[1] < ay ? v.bbox[1] : ay;}
  }
  const int32_t device = kh::mapper_device(m);
  if (device < 0 || device >= ndev) {
    kh::set_error("no usable HIP device (libkartohip has no CPU fallback)");
    return KH_ERR_NO_DEVICE;
  }
  kh_live_map * g = new kh_live_map();
  g->mapper = m; g->device = device; g->laser = kh::mapper_laser(m);
  g->ax = ax; g->ay = ay; g->resolution = resolution; g->scale = 1.0 / resolution;
  g->rebuild_fraction = rebuild_fraction < 0 ? kDefaultRebuildFraction : rebuild_fraction;
  const double reach = std::ceil(g->laser.range_threshold * g->scale) + kMargin;
  g->reach = reach < kCellLimit ? static_cast<int64_t>(reach) : static_cast<int64_t>(kCellLimit);
  std::memset(&g->stats, 0, sizeof(g->stats));
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
    hipEventCreate(&g->ev[0]) != hipSuccess || hipEventCreate(&g->ev[1]) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&g->d_counters), 2 * sizeof(unsigned long long)) != hipSuccess)
  {
    kh::set_error("kh_live_map_create: HIP allocation failed");
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
  kh::free_window(g->win);
  (void)hipFree(g->d_log); (void)hipFree(g->d_records); (void)hipFree(g->d_counters);
  if (g->ev[0]) {(void)hipEventDestroy(g->ev[0]);}
  if (g->ev[1]) {(void)hipEventDestroy(g->ev[1]);}
  if (g->stream) {(void)hipStreamDestroy(g->stream);}
  delete g;
}

int kh_live_map_update(kh_live_map * g, uint32_t min_pass_through, double occupancy_threshold)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (g->laser.n_beams <= 0) {kh::set_error("kh_live_map_update: the laser has no beams"); return KH_ERR_INVALID_ARG;}
  // ---- 1. classify the mapper's scans against the log (nothing is touched before the new window is known to fit)
  std::vector<SensorView> views;
  kh::mapper_sensor_poses(g->mapper, views);
  struct Change {int32_t id, cx, cy; const SensorView * view;};
  std::vector<Change> added, moved;
  std::vector<int32_t> gone;
  {
    size_t k = 0;
    for (const SensorView & v : views) {
      while (k < g->logged.size() && g->logged[k] < v.id) {gone.push_back(g->logged[k++]);}
      const bool known = k < g->logged.size() && g->logged[k] == v.id;
      if (known) {++k;}
      if (known && std::memcmp(g->entries[static_cast<size_t>(v.id)].sensor, v.sensor, sizeof(v.sensor)) == 0) {continue;}
      Change c;
      c.id = v.id; c.view = &v;
      if (!kh::cell_of(g, v.sensor, &c.cx, &c.cy)) {
        kh::set_error("kh_live_map_update: scan " + std::to_string(v.id) + " is too far from the anchor for this resolution");
        return KH_ERR_INVALID_ARG;
      }
      (known ? moved : added).push_back(c);
    }
    while (k < g->logged.size()) {gone.push_back(g->logged[k++]);}
  }
  const int64_t n_alive = static_cast<int64_t>(views.size()), n_delta = static_cast<int64_t>(added.size() + moved.size() + gone.size());
  const bool rebuild = g->counters_suspect || g->rebuild_fraction == 0.0 ||
    static_cast<double>(n_delta) > g->rebuild_fraction * static_cast<double>(n_alive);
  // ---- 2. the window: the old one joined with the blocks around every new position
  Window now;
  now.ox = g->win.ox; now.oy = g->win.oy; now.width = g->win.width; now.height = g->win.height;
  auto cover = [&](int32_t cx, int32_t cy) {
    const int64_t x0 = kh::floor_block(cx - g->reach), x1 = static_cast<int64_t>(kh::floor_block(cx + g->reach)) + kBlock;
    const int64_t y0 = kh::floor_block(cy - g->reach), y1 = static_cast<int64_t>(kh::floor_block(cy + g->reach)) + kBlock;
    if (now.width == 0) {now.ox = x0; now.oy = y0; now.width = x1 - x0; now.height = y1 - y0; return;}
    const int64_t ex = std::max(now.ox + now.width, x1), ey = std::max(now.oy + now.height, y1);
    now.ox = std::min(now.ox, x0); now.oy = std::min(now.oy, y0);
    now.width = ex - now.ox; now.height = ey - now.oy;
  };
  for (const Change & c : added) {cover(c.cx, c.cy);}
  for (const Change & c : moved) {cover(c.cx, c.cy);}
  const bool relayout = now.ox != g->win.ox || now.oy != g->win.oy || now.width != g->win.width || now.height != g->win.height;
  if (relayout && (now.width + 7) * now.height > (1ll << 31) - 4096) {
    kh::set_error("kh_live_map_update: the window would be " + std::to_string(now.width) + " x " + std::to_string(now.height) +
      " cells, beyond the size cap of an occupancy grid");
    return KH_ERR_INVALID_ARG;
  }
  if (hipSetDevice(g->device) != hipSuccess) {return KH_ERR_HIP;}
  // ---- 3. relayout: new arrays, the counters copied to their new place
  if (relayout) {
    LiveWindow w;
    w.ox = static_cast<int32_t>(now.ox); w.oy = static_cast<int32_t>(now.oy);
    w.width = static_cast<int32_t>(now.width); w.height = static_cast<int32_t>(now.height); w.ws = (w.width + 7) & ~7;
    w.pass = nullptr; w.hits = nullptr; w.cells = nullptr;
    const size_t size = static_cast<size_t>(w.ws) * static_cast<size_t>(w.height);
    if (hipMalloc(reinterpret_cast<void **>(&w.pass), size * 4) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&w.hits), size * 4) != hipSuccess ||
      hipMalloc(reinterpret_cast<void **>(&w.cells), size) != hipSuccess)
    {
      (void)hipGetLastError();
      kh::free_window(w);
      kh::set_error("kh_live_map_update: window allocation failed");
      return KH_ERR_HIP;                       // (the map is as it was)
    }
    if (hipMemsetAsync(w.pass, 0, size * 4, g->stream) != hipSuccess || hipMemsetAsync(w.hits, 0, size * 4, g->stream) != hipSuccess ||
      hipMemsetAsync(w.cells, 0, size, g->stream) != hipSuccess)
    {
      (void)hipStreamSynchronize(g->stream);
      kh::free_window(w);
      return KH_ERR_HIP;
    }
    if (g->win.width > 0 && !rebuild) {
      const size_t at = static_cast<size_t>(g->win.ox - w.ox) + static_cast<size_t>(g->win.oy - w.oy) * static_cast<size_t>(w.ws);
      const size_t row = static_cast<size_t>(g->win.width) * 4;
      if (hipMemcpy2DAsync(w.pass + at, static_cast<size_t>(w.ws) * 4, g->win.pass, static_cast<size_t>(g->win.ws) * 4, row,
          static_cast<size_t>(g->win.height), hipMemcpyDeviceToDevice, g->stream) != hipSuccess ||
        hipMemcpy2DAsync(w.hits + at, static_cast<size_t>(w.ws) * 4, g->win.hits, static_cast<size_t>(g->win.ws) * 4, row,
          static_cast<size_t>(g->win.height), hipMemcpyDeviceToDevice, g->stream) != hipSuccess)
      {
        (void)hipStreamSynchronize(g->stream);
        kh::free_window(w);
        return KH_ERR_HIP;
      }
    }
    if (hipStreamSynchronize(g->stream) != hipSuccess) {kh::free_window(w); return kh::fail_hip(g, "relayout");}
    kh::free_window(g->win);
    g->win = w;
    g->all_cells_stale = true;
  }
  // ---- 4. the log's slots
  const int64_t n_added = static_cast<int64_t>(added.size()), n_moved = static_cast<int64_t>(moved.size());
  if (rebuild) {
    for (int32_t id : g->logged) {g->entries[static_cast<size_t>(id)].slot = -1;}
    g->logged.clear(); g->free_slots.clear(); g->next_slot = 0;
    g->all_cells_stale = true;
    added.clear(); moved.clear();
    for (const SensorView & v : views) {
      Change c;
      c.id = v.id; c.view = &v;
      (void)kh::cell_of(g, v.sensor, &c.cx, &c.cy);                 // (every scan passed the test above or at an earlier update)
      added.push_back(c);
    }
  }
  const int64_t slots_needed = g->next_slot + std::max<int64_t>(0, static_cast<int64_t>(added.size()) - static_cast<int64_t>(g->free_slots.size()));
  const int64_t slot_words = kh::live_log_slot_words(g->laser.n_beams);
  if (slots_needed > g->cap_slots) {
    const int64_t cap = std::max<int64_t>(slots_needed + slots_needed / 2, 64);
    int32_t * d_new = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d_new), static_cast<size_t>(cap * slot_words) * 4) != hipSuccess) {
      (void)hipGetLastError();
      kh::set_error("kh_live_map_update: log allocation failed");
      g->counters_suspect = g->counters_suspect || rebuild;          // (a rebuild has already forgotten its slots)
      return KH_ERR_HIP;
    }
    if (g->next_slot > 0 && hipMemcpy(d_new, g->d_log, static_cast<size_t>(g->next_slot * slot_words) * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
      (void)hipFree(d_new);
      return kh::fail_hip(g, "log copy");
    }
    (void)hipFree(g->d_log);
    g->d_log = d_new; g->cap_slots = cap;
  }
  // ---- 5. residency of what will be read, and the delta table: SUB, MOVE, ADD
  std::vector<int32_t> read_ids;
  for (const Change & c : moved) {read_ids.push_back(c.id);}
  for (const Change & c : added) {read_ids.push_back(c.id);}
  std::vector<ResidentScan> resident;
  int64_t up_points = 0, up_ranges = 0;
  int rc = kh::mapper_resident_table_of(g->mapper, g->stream, "kh_live_map_update", read_ids.data(), read_ids.size(), resident, &up_points, &up_ranges);
  if (rc) {(void)hipStreamSynchronize(g->stream); g->counters_suspect = g->counters_suspect || rebuild; return rc;}
  std::vector<DeltaRecord> records;
  records.reserve(gone.size() + read_ids.size());
  auto record = [&](int32_t kind, int32_t slot, size_t k, const Change * c) {
    DeltaRecord r;
    std::memset(&r, 0, sizeof(r));
    r.kind = kind; r.slot = slot;
    if (c) {
      r.points = resident[k].points; r.ranges = resident[k].ranges;
      r.sx = c->view->sensor[0]; r.sy = c->view->sensor[1];
      const Entry & e = g->entries[static_cast<size_t>(c->id)];
      r.old_cx = e.cx; r.old_cy = e.cy;
    }
    records.push_back(r);
  };
  if (!rebuild) {for (int32_t id : gone) {record(kDeltaSub, g->entries[static_cast<size_t>(id)].slot, 0, nullptr);}}
  size_t k = 0;
  for (const Change & c : moved) {record(kDeltaMove, g->entries[static_cast<size_t>(c.id)].slot, k++, &c);}
  if (!views.empty() && g->entries.size() <= static_cast<size_t>(views.back().id)) {g->entries.resize(static_cast<size_t>(views.back().id) + 1);}
  std::vector<int32_t> new_slots;
  {
    // (slots are taken from a copy of the free list: the list itself changes only once the update has succeeded)
    size_t free_left = g->free_slots.size();
    int64_t next = g->next_slot;
    for (const Change & c : added) {
      const int32_t slot = free_left > 0 ? g->free_slots[--free_left] : static_cast<int32_t>(next++);
      new_slots.push_back(slot);
      record(kDeltaAdd, slot, k++, &c);
    }
  }
  if (records.size() > g->cap_records) {
    (void)hipStreamSynchronize(g->stream);
    (void)hipFree(g->d_records); g->d_records = nullptr; g->cap_records = 0;
    const size_t cap = records.size() + records.size() / 2;
    if (hipMalloc(reinterpret_cast<void **>(&g->d_records), cap * sizeof(DeltaRecord)) != hipSuccess) {
      (void)hipGetLastError();
      kh::set_error("kh_live_map_update: delta table allocation failed");
      g->counters_suspect = g->counters_suspect || rebuild;
      return KH_ERR_HIP;
    }
    g->cap_records = cap;
  }
  // ---- 6. the trace
  const size_t size = static_cast<size_t>(g->win.ws) * static_cast<size_t>(g->win.height);
  if (rebuild && size > 0 && !relayout &&
    (hipMemsetAsync(g->win.pass, 0, size * 4, g->stream) != hipSuccess || hipMemsetAsync(g->win.hits, 0, size * 4, g->stream) != hipSuccess)) {
    return kh::fail_hip(g, "clear");
  }
  if (hipMemsetAsync(g->d_counters, 0, 2 * sizeof(unsigned long long), g->stream) != hipSuccess) {return kh::fail_hip(g, "counters");}
  if (!records.empty() &&
    hipMemcpyAsync(g->d_records, records.data(), records.size() * sizeof(DeltaRecord), hipMemcpyHostToDevice, g->stream) != hipSuccess) {
    return kh::fail_hip(g, "delta table upload");
  }
  (void)hipEventRecord(g->ev[0], g->stream);
  kh::live_trace_delta(g->stream, g->win, g->ax, g->ay, g->scale, g->d_records, static_cast<int32_t>(records.size()), g->laser.n_beams,
    g->laser.range_threshold, g->laser.minimum_range, g->laser.maximum_range, g->d_log, g->d_counters);
  (void)hipEventRecord(g->ev[1], g->stream);
  // ---- 7. cell states: the whole window, or the rectangle the delta can have touched
  const bool params_changed = !g->have_params || g->min_pass != min_pass_through ||
    std::memcmp(&g->threshold, &occupancy_threshold, sizeof(double)) != 0;
  int64_t cells_given = 0;
  bool given_whole = false;
  int64_t gx0 = 0, gy0 = 0, gx1 = 0, gy1 = 0;                     // the rectangle given, window columns [gx0, gx1) and rows [gy0, gy1)
  if (g->win.width > 0) {
    if (g->all_cells_stale || params_changed) {
      kh::live_update_cells(g->stream, g->win, 0, 0, g->win.ws, g->win.height, min_pass_through, occupancy_threshold);
      cells_given = static_cast<int64_t>(g->win.ws) * g->win.height;
      given_whole = true;
    } else if (!records.empty()) {
      int64_t x0 = std::numeric_limits<int64_t>::max(), y0 = x0, x1 = std::numeric_limits<int64_t>::min(), y1 = x1;
      auto touch = [&](int32_t cx, int32_t cy) {
        x0 = std::min<int64_t>(x0, cx - g->reach); x1 = std::max<int64_t>(x1, cx + g->reach);
        y0 = std::min<int64_t>(y0, cy - g->reach); y1 = std::max<int64_t>(y1, cy + g->reach);
      };
      for (int32_t id : gone) {touch(g->entries[static_cast<size_t>(id)].cx, g->entries[static_cast<size_t>(id)].cy);}
      for (const Change & c : moved) {touch(g->entries[static_cast<size_t>(c.id)].cx, g->entries[static_cast<size_t>(c.id)].cy); touch(c.cx, c.cy);}
      for (const Change & c : added) {touch(c.cx, c.cy);}
      x0 = std::max<int64_t>(x0 - g->win.ox, 0); y0 = std::max<int64_t>(y0 - g->win.oy, 0);
      x1 = std::min<int64_t>(x1 - g->win.ox, g->win.width - 1); y1 = std::min<int64_t>(y1 - g->win.oy, g->win.height - 1);
      if (x1 >= x0 && y1 >= y0) {
        kh::live_update_cells(g->stream, g->win, static_cast<int32_t>(x0), static_cast<int32_t>(y0), static_cast<int32_t>(x1 - x0 + 1),
          static_cast<int32_t>(y1 - y0 + 1), min_pass_through, occupancy_threshold);
        cells_given = (x1 - x0 + 1) * (y1 - y0 + 1);
        gx0 = x0; gy0 = y0; gx1 = x1 + 1; gy1 = y1 + 1;
      }
    }
  }
  unsigned long long counters[2] = {0, 0};
  if (hipMemcpyAsync(counters, g->d_counters, sizeof(counters), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipStreamSynchronize(g->stream) != hipSuccess) {return kh::fail_hip(g, "trace");}
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
  // ---- 8. the update has happened: the host's copy of the log follows
  for (const Change & c : moved) {
    Entry & e = g->entries[static_cast<size_t>(c.id)];
    e.cx = c.cx; e.cy = c.cy; std::memcpy(e.sensor, c.view->sensor, sizeof(e.sensor));
  }
  for (size_t a = 0; a < added.size(); ++a) {
    Entry & e = g->entries[static_cast<size_t>(added[a].id)];
    e.slot = new_slots[a]; e.cx = added[a].cx; e.cy = added[a].cy; std::memcpy(e.sensor, added[a].view->sensor, sizeof(e.sensor));
    if (!g->free_slots.empty() && g->free_slots.back() == e.slot) {g->free_slots.pop_back();} else {g->next_slot = std::max<int64_t>(g->next_slot, e.slot + 1);}
  }
  // (the slots of the scans that left are free from the NEXT update on: this one's ADD records were dealt before)
  if (!rebuild) {
    for (int32_t id : gone) {
      Entry & e = g->entries[static_cast<size_t>(id)];
      g->free_slots.push_back(e.slot);
      e.slot = -1;
    }
  }
  g->logged.clear();
  for (const SensorView & v : views) {g->logged.push_back(v.id);}
  g->have_params = true; g->min_pass = min_pass_through; g->threshold = occupancy_threshold;
  g->all_cells_stale = false; g->counters_suspect = false;
  if (cells_given > 0) {kh::feeds_pending(g, given_whole, gx0, gy0, gx1, gy1);}
  kh_live_map_counts & last = g->stats.last;
  std::memset(&last, 0, sizeof(last));
  last.scans_added = n_added; last.scans_removed = static_cast<int64_t>(gone.size()); last.scans_moved = n_moved;
  last.beams_traced = static_cast<int64_t>(counters[0]); last.beams_skipped = static_cast<int64_t>(counters[1]);
  last.cells_updated = cells_given; last.relayouts = relayout ? 1 : 0; last.rebuilds = rebuild ? 1 : 0;
  last.trace_ms = records.empty() ? 0.0 : static_cast<double>(ms);
  kh_live_map_counts & total = g->stats.total;
  total.scans_added += last.scans_added; total.scans_removed += last.scans_removed; total.scans_moved += last.scans_moved;
  total.beams_traced += last.beams_traced; total.beams_skipped += last.beams_skipped; total.cells_updated += last.cells_updated;
  total.relayouts += last.relayouts; total.rebuilds += last.rebuilds; total.trace_ms += last.trace_ms;
  g->stats.updates += 1;
  g->stats.scans_in_map = static_cast<int64_t>(g->logged.size());
  g->stats.log_bytes = g->cap_slots * slot_words * 4;
  return KH_OK;
}

int kh_live_map_info(const kh_live_map * g, kh_live_map_info_t * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  out->anchor[0] = g->ax; out->anchor[1] = g->ay; out->resolution = g->resolution; out->rebuild_fraction = g->rebuild_fraction;
  out->ox = g->win.ox; out->oy = g->win.oy; out->width = g->win.width; out->height = g->win.height; out->width_step = g->win.ws;
  out->reach = static_cast<int32_t>(std::min<int64_t>(g->reach, INT32_MAX));
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

// ---------------------------------------------------------------- the map feed

int kh_map_feed_create(kh_live_map * g, kh_map_feed ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    kh::set_error("no usable HIP device (libkartohip has no CPU fallback)");
    return KH_ERR_NO_DEVICE;
  }
  if (!g) {return KH_ERR_INVALID_ARG;}
  kh_map_feed * f = new kh_map_feed();
  f->live = g; f->device = g->device;
  std::memset(&f->last, 0, sizeof(f->last));
  std::memset(&f->stats, 0, sizeof(f->stats));
  if (hipSetDevice(f->device) != hipSuccess || hipEventCreate(&f->ev[0]) != hipSuccess || hipEventCreate(&f->ev[1]) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&f->d_count), sizeof(uint32_t)) != hipSuccess)
  {
    (void)hipGetLastError();
    kh::set_error("kh_map_feed_create: HIP allocation failed");
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

int kh_map_feed_poll(kh_map_feed * f, kh_map_feed_delta_t * out)
{
  if (!f || !out) {return KH_ERR_INVALID_ARG;}
  kh_live_map * g = f->live;
  if (!g) {kh::set_error("kh_map_feed_poll: the feed's live map has been destroyed"); return KH_ERR_INVALID_ARG;}
  kh_map_feed_delta_t & d = f->last;
  auto done = [&]() {
    d.ox = f->ox; d.oy = f->oy; d.width = f->width; d.height = f->height;
    f->stats.polls += 1; f->stats.n_tiles += d.n_tiles; f->stats.tiles_scanned += d.tiles_scanned;
    f->stats.bytes_downloaded += d.bytes_downloaded; f->stats.kernel_ms += d.kernel_ms;
    *out = d;
    return KH_OK;
  };
  std::memset(&d, 0, sizeof(d));
  f->tile_xy.clear(); f->data.clear();
  const LiveWindow & w = g->win;
  if (w.width == 0 || !(f->pending_whole || f->pending_rect)) {return done();}
  // what the tile rule stands on: no tile straddles the window's edge, and the cells have no row padding
  if (w.ox % kBlock || w.oy % kBlock || w.width % kBlock || w.height % kBlock || w.ws != w.width) {
    kh::set_error("kh_map_feed_poll: the live window is not made of whole 64-cell blocks without row padding");
    return KH_ERR_INVALID_ARG;
  }
  if (hipSetDevice(f->device) != hipSuccess) {return KH_ERR_HIP;}
  // ---- 1. the published grid follows the window: a new array of -1, the old content at its place
  if (w.ox != f->ox || w.oy != f->oy || w.width != f->width || w.height != f->height) {
    const bool inside = f->width == 0 || (f->ox >= w.ox && f->oy >= w.oy && static_cast<int64_t>(f->ox) + f->width <= static_cast<int64_t>(w.ox) + w.width &&
      static_cast<int64_t>(f->oy) + f->height <= static_cast<int64_t>(w.oy) + w.height);
    if (!inside) {kh::set_error("kh_map_feed_poll: the live window shrank"); return KH_ERR_INVALID_ARG;}
    const size_t size = static_cast<size_t>(w.width) * static_cast<size_t>(w.height);
    int8_t * d_new = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d_new), size) != hipSuccess) {
      (void)hipGetLastError();
      kh::set_error("kh_map_feed_poll: published grid allocation failed");
      return KH_ERR_HIP;                       // (the feed is as it was, its region still pending)
    }
    bool ok = hipMemsetAsync(d_new, 0xFF, size, g->stream) == hipSuccess;
    if (ok && f->width > 0) {
      const size_t at = static_cast<size_t>(f->ox - w.ox) + static_cast<size_t>(f->oy - w.oy) * static_cast<size_t>(w.width);
      ok = hipMemcpy2DAsync(d_new + at, static_cast<size_t>(w.width), f->d_pub, static_cast<size_t>(f->width), static_cast<size_t>(f->width),
          static_cast<size_t>(f->height), hipMemcpyDeviceToDevice, g->stream) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(g->stream) != hipSuccess) {
      const int rc = kh::fail_feed(f, "relayout");
      (void)hipFree(d_new);
      return rc;
    }
    (void)hipFree(f->d_pub);
    f->d_pub = d_new; f->ox = w.ox; f->oy = w.oy; f->width = w.width; f->height = w.height;
    f->pending_whole = true;                   // (a window that grew was given to the cell-state kernel whole: this restates it)
  }
  // ---- 2. the pending region, rounded outward to whole tiles and clipped to the window
  const int64_t wx1 = static_cast<int64_t>(f->ox) + f->width, wy1 = static_cast<int64_t>(f->oy) + f->height;
  int64_t x0 = f->ox, y0 = f->oy, x1 = wx1, y1 = wy1;
  if (!f->pending_whole) {
    x0 = std::max<int64_t>(f->x0, f->ox); y0 = std::max<int64_t>(f->y0, f->oy); x1 = std::min(f->x1, wx1); y1 = std::min(f->y1, wy1);
  }
  if (x1 <= x0 || y1 <= y0) {f->pending_whole = false; f->pending_rect = false; return done();}
  NavFeedJob job;
  job.tx0 = static_cast<int32_t>(kh::floor_div(x0, kMapTile)); job.ty0 = static_cast<int32_t>(kh::floor_div(y0, kMapTile));
  job.tx1 = static_cast<int32_t>(kh::floor_div(x1 - 1, kMapTile) + 1); job.ty1 = static_cast<int32_t>(kh::floor_div(y1 - 1, kMapTile) + 1);
  // (the window is made of whole tiles, so the rounding cannot leave it; the clamp is a guard)
  job.tx0 = std::max<int32_t>(job.tx0, f->ox / kMapTile); job.ty0 = std::max<int32_t>(job.ty0, f->oy / kMapTile);
  job.tx1 = std::min<int32_t>(job.tx1, static_cast<int32_t>(wx1 / kMapTile)); job.ty1 = std::min<int32_t>(job.ty1, static_cast<int32_t>(wy1 / kMapTile));
  const int64_t tiles = static_cast<int64_t>(job.tx1 - job.tx0) * (job.ty1 - job.ty0);
  if (tiles > f->cap_tiles) {
    (void)hipFree(f->d_xy); (void)hipFree(f->d_packed);
    f->d_xy = nullptr; f->d_packed = nullptr; f->cap_tiles = 0;
    if (hipMalloc(reinterpret_cast<void **>(&f->d_xy), static_cast<size_t>(tiles) * 2 * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void **>(&f->d_packed), static_cast<size_t>(tiles) * kTileWords * sizeof(uint32_t)) != hipSuccess)
    {
      (void)hipGetLastError();
      (void)hipFree(f->d_xy); f->d_xy = nullptr;
      kh::set_error("kh_map_feed_poll: tile buffer allocation failed");
      return KH_ERR_HIP;
    }
    f->cap_tiles = tiles;
  }
  job.cells = w.cells; job.cells_ox = w.ox; job.cells_oy = w.oy; job.cells_ws = w.ws;
  job.published = f->d_pub; job.pub_ox = f->ox; job.pub_oy = f->oy; job.pub_ws = f->width;
  job.count = f->d_count; job.tile_xy = f->d_xy; job.packed = f->d_packed;
  // ---- 3. compare and pack
  if (hipMemsetAsync(f->d_count, 0, sizeof(uint32_t), g->stream) != hipSuccess) {return kh::fail_feed(f, "count");}
  (void)hipEventRecord(f->ev[0], g->stream);
  kh::nav_feed(g->stream, job);
  (void)hipEventRecord(f->ev[1], g->stream);
  // ---- 4. the count, then that many coordinates and tiles
  uint32_t count = 0;
  if (hipMemcpyAsync(&count, f->d_count, sizeof(count), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipStreamSynchronize(g->stream) != hipSuccess) {return kh::fail_feed(f, "compare");}
  if (static_cast<int64_t>(count) > tiles) {kh::set_error("kh_map_feed_poll: more tiles reported than compared"); f->pending_whole = true; return KH_ERR_HIP;}
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, f->ev[0], f->ev[1]);
  const size_t n = count;
  f->raw_xy.resize(2 * n); f->raw_data.resize(256 * n);
  if (n > 0 && (hipMemcpyAsync(f->raw_xy.data(), f->d_xy, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipMemcpyAsync(f->raw_data.data(), f->d_packed, n * 256, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
    hipStreamSynchronize(g->stream) != hipSuccess)) {return kh::fail_feed(f, "download");}
  f->pending_whole = false; f->pending_rect = false;
  // ascending (ty, tx): the kernel deals its slots in no order
  std::vector<uint32_t> order(n);
  for (size_t k = 0; k < n; ++k) {order[k] = static_cast<uint32_t>(k);}
  const int32_t * xy = f->raw_xy.data();
  std::sort(order.begin(), order.end(), [xy](uint32_t a, uint32_t b) {
    return xy[2 * a + 1] != xy[2 * b + 1] ? xy[2 * a + 1] < xy[2 * b + 1] : xy[2 * a] < xy[2 * b];
  });
  f->tile_xy.resize(2 * n); f->data.resize(256 * n);
  int32_t bx0 = INT32_MAX, by0 = INT32_MAX, bx1 = INT32_MIN, by1 = INT32_MIN;
  for (size_t k = 0; k < n; ++k) {
    const int32_t tx = xy[2 * order[k]], ty = xy[2 * order[k] + 1];
    f->tile_xy[2 * k] = tx; f->tile_xy[2 * k + 1] = ty;
    std::memcpy(f->data.data() + 256 * k, f->raw_data.data() + 256 * static_cast<size_t>(order[k]), 256);
    bx0 = std::min(bx0, tx); by0 = std::min(by0, ty); bx1 = std::max(bx1, tx); by1 = std::max(by1, ty);
  }
  // ---- 5. the counts
  d.n_tiles = static_cast<int64_t>(n); d.tiles_scanned = tiles;
  d.bytes_downloaded = static_cast<int64_t>(sizeof(count) + n * (2 * sizeof(int32_t) + 256));
  d.kernel_ms = static_cast<double>(ms);
  if (n > 0) {d.x = bx0 * kMapTile; d.y = by0 * kMapTile; d.w = (bx1 - bx0 + 1) * kMapTile; d.h = (by1 - by0 + 1) * kMapTile;}
  return done();
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
  const int64_t x0 = std::max<int64_t>(x, f->ox), y0 = std::max<int64_t>(y, f->oy);
  const int64_t x1 = std::min<int64_t>(static_cast<int64_t>(x) + w, static_cast<int64_t>(f->ox) + f->width);
  const int64_t y1 = std::min<int64_t>(static_cast<int64_t>(y) + h, static_cast<int64_t>(f->oy) + f->height);
  if (x1 <= x0 || y1 <= y0) {return KH_OK;}
  if (hipSetDevice(f->device) != hipSuccess) {return KH_ERR_HIP;}
  const int8_t * src = f->d_pub + (x0 - f->ox) + (y0 - f->oy) * f->width;
  int8_t * dst = out + (x0 - x) + (y0 - y) * static_cast<int64_t>(w);
  if (hipMemcpy2D(dst, static_cast<size_t>(w), src, static_cast<size_t>(f->width), static_cast<size_t>(x1 - x0), static_cast<size_t>(y1 - y0),
      hipMemcpyDeviceToHost) != hipSuccess)
  {
    kh::set_error(std::string("kh_map_feed_read: ") + hipGetErrorString(hipGetLastError()));
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

}  // extern "C"
