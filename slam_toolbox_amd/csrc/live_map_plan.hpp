// The host rules of the live map and its feed (DESIGN.md sections 7b, 7c) as plain functions: floor division, rectangles of
// lattice cells, the classification of the mapper's scans against the log, the window, the log's slots, the touched rectangle and
// the feed's tile job.  Nothing here knows HIP: live_map.cpp plans an update with these before it queues anything on the device,
// and tests/live_map_plan_check.cpp runs them on the CPU (tests/test_live_map_plan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "occupancy_device.hpp"

namespace kh
{
constexpr int32_t kBlock = 64;              // the window grows in blocks of kBlock x kBlock lattice cells
constexpr int32_t kMargin = 2;              // cells beyond ceil(range_threshold * scale) the window keeps around a sensor cell
constexpr double kCellLimit = 1073741824.0;          // |cell index| a scan may have (2^30): index +- reach stays an int32

// the floor quotient, b > 0: cells and tiles left of and below the anchor are negative
inline int64_t floor_div(int64_t a, int64_t b) {return a >= 0 ? a / b : -((-a + b - 1) / b);}

// cells [x0, x1) x [y0, y1); every empty rectangle is "none"
struct Rect
{
  int64_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  bool empty() const {return x1 <= x0 || y1 <= y0;}
  int64_t width() const {return empty() ? 0 : x1 - x0;}
  int64_t height() const {return empty() ? 0 : y1 - y0;}
  bool operator==(const Rect & o) const {return (empty() && o.empty()) || (x0 == o.x0 && y0 == o.y0 && x1 == o.x1 && y1 == o.y1);}
  bool operator!=(const Rect & o) const {return !(*this == o);}
  Rect join(const Rect & o) const         // the smallest rectangle that holds both
  {
    if (empty()) {return o;}
    if (o.empty()) {return *this;}
    return Rect{std::min(x0, o.x0), std::min(y0, o.y0), std::max(x1, o.x1), std::max(y1, o.y1)};
  }
  Rect clip(const Rect & o) const         // what both hold
  {
    const Rect r{std::max(x0, o.x0), std::max(y0, o.y0), std::min(x1, o.x1), std::min(y1, o.y1)};
    return r.empty() ? Rect{} : r;
  }
  bool contains(const Rect & o) const {return o.empty() || (!empty() && o.x0 >= x0 && o.y0 >= y0 && o.x1 <= x1 && o.y1 <= y1);}
  Rect rounded_out(int64_t step) const    // outward to multiples of step
  {
    if (empty()) {return Rect{};}
    return Rect{floor_div(x0, step) * step, floor_div(y0, step) * step, (floor_div(x1 - 1, step) + 1) * step, (floor_div(y1 - 1, step) + 1) * step};
  }
  Rect moved_by(int64_t dx, int64_t dy) const {return empty() ? Rect{} : Rect{x0 + dx, y0 + dy, x1 + dx, y1 + dy};}
};
inline Rect rect_of(const LiveWindow & w) {return Rect{w.ox, w.oy, static_cast<int64_t>(w.ox) + w.width, static_cast<int64_t>(w.oy) + w.height};}

// ---- the lattice ----
struct Lattice
{
  double ax = 0.0, ay = 0.0, scale = 20.0;      // anchor, 1 / resolution
  int64_t reach = 0;                            // ceil(range_threshold * scale) + kMargin
};

inline int64_t reach_of(double range_threshold, double scale)
{
  const double reach = std::ceil(range_threshold * scale) + kMargin;
  return reach < kCellLimit ? static_cast<int64_t>(reach) : static_cast<int64_t>(kCellLimit);
}

// the sensor's cell by the operations of occ_cell (occupancy_walk.hpp): o_to_int(o_round((x - anchor) * scale)); false = too far from the anchor
inline bool cell_of(const Lattice & l, const double sensor[3], int32_t * cx, int32_t * cy)
{
  const double x = round_half_away((sensor[0] - l.ax) * l.scale), y = round_half_away((sensor[1] - l.ay) * l.scale);
  if (!(std::fabs(x) < kCellLimit && std::fabs(y) < kCellLimit)) {return false;}
  *cx = static_cast<int32_t>(x); *cy = static_cast<int32_t>(y);
  return true;
}

// every cell a scan with its sensor in cell (cx, cy) can touch
inline Rect reach_around(int32_t cx, int32_t cy, int64_t reach) {return Rect{cx - reach, cy - reach, cx + reach + 1, cy + reach + 1};}

// ---- the host's copy of the log ----
struct Entry
{
  int32_t slot = -1;         // slot of the log, -1 = the scan is not in the map
  int32_t cx = 0, cy = 0;    // the sensor cell the log holds
  double sensor[3] = {0.0, 0.0, 0.0};      // the sensor pose the scan was traced at
};

struct HostLog
{
  std::vector<Entry> entries;                // by scan id
  std::vector<int32_t> logged;               // ids of the scans in the map, ascending
  std::vector<int32_t> free_slots;           // taken last in, first out
  int64_t next_slot = 0;                     // slots [0, next_slot) have been dealt at some time
};

struct Change {int32_t id, cx, cy; const SensorView * view;};

// What one update is going to do, worked out before anything is queued on the device.  Nothing of it is in the log until commit().
struct UpdatePlan
{
  std::vector<Change> added, moved;          // the ADD and MOVE records (a rebuild: every scan alive is added, none moved)
  std::vector<int32_t> gone;                 // the SUB records (a rebuild writes none, but still counts them)
  int64_t n_added = 0, n_moved = 0;          // as classified, whatever a rebuild makes of them
  int32_t too_far = -1;                      // the id of a scan too far from the anchor for this resolution: the update is refused
  bool rebuild = false;
  Rect window;                               // the window after the update
  std::vector<int32_t> new_slots;            // added[a]'s slot
  size_t free_left = 0;                      // what the deal leaves of the free list ...
  int64_t next_slot = 0;                     // ... and of next_slot: the slots the log must hold
};

// the merge walk of the mapper's scans (ascending id) against the log: new / gone / moved (the bits of the sensor pose differ)
inline void classify(const Lattice & l, const std::vector<SensorView> & views, const HostLog & log, UpdatePlan & p)
{
  size_t k = 0;
  for (const SensorView & v : views) {
    while (k < log.logged.size() && log.logged[k] < v.id) {p.gone.push_back(log.logged[k++]);}
    const bool known = k < log.logged.size() && log.logged[k] == v.id;
    if (known) {++k;}
    if (known && std::memcmp(log.entries[static_cast<size_t>(v.id)].sensor, v.sensor, sizeof(v.sensor)) == 0) {continue;}
    Change c;
    c.id = v.id; c.view = &v;
    if (!cell_of(l, v.sensor, &c.cx, &c.cy)) {p.too_far = v.id; return;}
    (known ? p.moved : p.added).push_back(c);
  }
  while (k < log.logged.size()) {p.gone.push_back(log.logged[k++]);}
  p.n_added = static_cast<int64_t>(p.added.size()); p.n_moved = static_cast<int64_t>(p.moved.size());
}

// the window rule: the old window joined with whole blocks around cell +- reach of every added or moved scan; it never shrinks
inline Rect window_after(const Rect & before, const UpdatePlan & p, int64_t reach)
{
  Rect now = before;
  for (const Change & c : p.added) {now = now.join(reach_around(c.cx, c.cy, reach).rounded_out(kBlock));}
  for (const Change & c : p.moved) {now = now.join(reach_around(c.cx, c.cy, reach).rounded_out(kBlock));}
  return now;
}

// a rebuild forgets the log: every scan alive is added again (each passed cell_of in classify or at an earlier update)
inline void make_rebuild(const Lattice & l, const std::vector<SensorView> & views, UpdatePlan & p)
{
  p.rebuild = true;
  p.added.clear(); p.moved.clear();
  for (const SensorView & v : views) {
    Change c;
    c.id = v.id; c.view = &v;
    (void)cell_of(l, v.sensor, &c.cx, &c.cy);
    p.added.push_back(c);
  }
}

// the slots of the added scans: from a copy of the free list, then from next_slot.  The log itself changes in commit() only, so
// the slot of a scan that leaves in this update is not dealt before the next one.
inline void deal_slots(const HostLog & log, UpdatePlan & p)
{
  p.free_left = p.rebuild ? 0 : log.free_slots.size();
  p.next_slot = p.rebuild ? 0 : log.next_slot;
  p.new_slots.clear();
  for (size_t a = 0; a < p.added.size(); ++a) {
    p.new_slots.push_back(p.free_left > 0 ? log.free_slots[--p.free_left] : static_cast<int32_t>(p.next_slot++));
  }
}

// the whole plan.  false = refused (p.too_far names the scan), and nothing else of p is to be used.
inline bool plan_update(const Lattice & l, const std::vector<SensorView> & views, const HostLog & log, const Rect & window, bool must_rebuild,
  double rebuild_fraction, UpdatePlan & p)
{
  p = UpdatePlan();
  classify(l, views, log, p);
  if (p.too_far >= 0) {return false;}
  p.window = window_after(window, p, l.reach);
  const double n_delta = static_cast<double>(p.added.size() + p.moved.size() + p.gone.size());
  if (must_rebuild || rebuild_fraction == 0.0 || n_delta > rebuild_fraction * static_cast<double>(views.size())) {make_rebuild(l, views, p);}
  deal_slots(log, p);
  return true;
}

// The cells the delta can have touched -- sensor cell +- reach of every record, old and new position -- as columns and rows of
// `window`, clipped to it; empty = none.
inline Rect touched(const UpdatePlan & p, const HostLog & log, int64_t reach, const Rect & window)
{
  Rect r;
  if (!p.rebuild) {
    for (int32_t id : p.gone) {r = r.join(reach_around(log.entries[static_cast<size_t>(id)].cx, log.entries[static_cast<size_t>(id)].cy, reach));}
    for (const Change & c : p.moved) {r = r.join(reach_around(log.entries[static_cast<size_t>(c.id)].cx, log.entries[static_cast<size_t>(c.id)].cy, reach));}
  }
  for (const Change & c : p.moved) {r = r.join(reach_around(c.cx, c.cy, reach));}
  for (const Change & c : p.added) {r = r.join(reach_around(c.cx, c.cy, reach));}
  return r.clip(window).moved_by(-window.x0, -window.y0);
}

// the update has happened: the host's copy of the log follows
inline void commit(HostLog & log, const std::vector<SensorView> & views, const UpdatePlan & p)
{
  if (p.rebuild) {for (int32_t id : log.logged) {log.entries[static_cast<size_t>(id)].slot = -1;}}
  if (!views.empty() && log.entries.size() <= static_cast<size_t>(views.back().id)) {log.entries.resize(static_cast<size_t>(views.back().id) + 1);}
  for (const Change & c : p.moved) {
    Entry & e = log.entries[static_cast<size_t>(c.id)];
    e.cx = c.cx; e.cy = c.cy; std::memcpy(e.sensor, c.view->sensor, sizeof(e.sensor));
  }
  for (size_t a = 0; a < p.added.size(); ++a) {
    Entry & e = log.entries[static_cast<size_t>(p.added[a].id)];
    e.slot = p.new_slots[a]; e.cx = p.added[a].cx; e.cy = p.added[a].cy; std::memcpy(e.sensor, p.added[a].view->sensor, sizeof(e.sensor));
  }
  log.free_slots.resize(p.free_left);
  log.next_slot = p.next_slot;
  // (the slots of the scans that left are free from the NEXT update on: this one's ADD records were dealt before)
  if (!p.rebuild) {
    for (int32_t id : p.gone) {
      Entry & e = log.entries[static_cast<size_t>(id)];
      log.free_slots.push_back(e.slot);
      e.slot = -1;
    }
  }
  log.logged.clear();
  for (const SensorView & v : views) {log.logged.push_back(v.id);}
}

// ---- the feed ----
// the tile columns [x0, x1) and rows [y0, y1) a poll compares: the pending region (the whole window, or the union of what the
// updates handed over) clipped to the window and rounded outward to whole tiles.  The window is made of whole tiles, so the
// rounding cannot leave it; the second clip is a guard.  Empty = nothing to compare.
inline Rect tile_job(bool pending_whole, const Rect & pending, const Rect & window)
{
  const Rect cells = (pending_whole ? window : pending.clip(window)).rounded_out(kMapTile).clip(window);
  if (cells.empty()) {return Rect{};}
  return Rect{floor_div(cells.x0, kMapTile), floor_div(cells.y0, kMapTile), floor_div(cells.x1 - 1, kMapTile) + 1, floor_div(cells.y1 - 1, kMapTile) + 1};
}
}  // namespace kh
