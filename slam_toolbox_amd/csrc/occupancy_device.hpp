// What the occupancy module shares between its kernel files (occupancy.hip, occupancy_live.hip, occupancy_map.hip,
// occupancy_changes.hip, occupancy_field.hip, occupancy_field_update.hip: the kernels and their launchers) and the host files that feed them: mapper_views.cpp (kh_mapper_build_map),
// merge.cpp (kh_merge_build), live_map.cpp (kh_live_map_*), map_localizer.cpp, map_changes.cpp, map_align.cpp, map_merge.cpp, map_field.cpp.  Needs no HIP header:
// the CPU programs of tests/ include it.  Not part of the public ABI (include/karto_hip.h).  The live map's lattice, window and log
// are stated in DESIGN.md section 7b, the map feed's tiles in 7c.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#ifdef __HIP__
#include <hip/hip_runtime.h>
#define KH_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define KH_HOST_DEVICE inline
#endif

#include "../../include/karto_hip.h"
#include "host_common.hpp"

namespace kh
{
// ---- host arithmetic of ComputeDimensions ----
inline double round_half_away(double v) {return v >= 0.0 ? std::floor(v + 0.5) : std::ceil(v - 0.5);}     // math::Round, Math.h:87-90

// BoundingBox2 (Karto.h:2846-2903) as ComputeDimensions uses it
struct Box
{
  double min_x = 999999999999999999.99999, min_y = 999999999999999999.99999;
  double max_x = -999999999999999999.99999, max_y = -999999999999999999.99999;
  void add(double x, double y)
  {
    min_x = x < min_x ? x : min_x; min_y = y < min_y ? y : min_y;
    max_x = x > max_x ? x : max_x; max_y = y > max_y ? y : max_y;
  }
};

// the box of the scans and the resolution -> the grid's width and height in cells (Karto.h:6106-6111); its offset is the box's minimum
inline void grid_dimensions(const Box & box, double resolution, int32_t * width, int32_t * height, double offset[2])
{
  const double scale = 1.0 / resolution;
  *width = static_cast<int32_t>(round_half_away((box.max_x - box.min_x) * scale));
  *height = static_cast<int32_t>(round_half_away((box.max_y - box.min_y) * scale));
  offset[0] = box.min_x; offset[1] = box.min_y;
}

// the size cap of an occupancy grid and of a live window: (width + 7) * height cells stay below 2^31 - 4096, stated without the product
inline bool grid_too_large(int64_t width, int64_t height) {return height > 0 && width + 7 > ((1ll << 31) - 4096) / height;}

// ---- the launch sizes of the kernels that give a wave a run of 64 beams, and a workgroup four waves ----
inline unsigned blocks_of_runs(int32_t n_scans, int32_t runs_per_scan) {return static_cast<unsigned>((static_cast<int64_t>(n_scans) * runs_per_scan + 3) / 4);}
// ... and of those whose workgroups hold waves of ONE pose (scan): the workgroups of a pose of n_beams >= 1 beams, or 0 where those of
// n_poses poses are more than one launch takes
inline int32_t blocks_per_pose(int32_t n_beams, int32_t n_poses)
{
  const int64_t blocks = ((static_cast<int64_t>(n_beams) + 63) / 64 + 3) / 4;
  return blocks * n_poses > INT32_MAX ? 0 : static_cast<int32_t>(blocks);
}

// ---- the records of the trace kernels ----
// one scan whose readings are resident on the grid's device (k_occ_trace_resident)
struct ResidentScan
{
  const double * points;     // 2 * n_beams unfiltered point readings, device memory
  const double * ranges;     // n_beams range readings, device memory
  double sx, sy;             // sensor position
};
static_assert(sizeof(ResidentScan) == 32, "one record = 4 x 8 bytes");

// one scan and one mapper (submap) of a merge (k_occ_trace_merged)
struct MergeScan
{
  const double * points;     // 2 * n_beams UNtransformed unfiltered point readings, device memory
  const double * ranges;     // n_beams range readings, device memory
  double sx, sy;             // transformed sensor position
  int32_t submap, pad;
};
struct MergeSubmap
{
  double c, s, tx, ty;       // the correction: cos / sin of its yaw (host libm), translation
  double range_threshold, min_range, max_range;      // the submap's laser
  int32_t n_beams, pad;
};
static_assert(sizeof(MergeScan) == 40 && sizeof(MergeSubmap) == 64, "records = 5 and 8 words of 8 bytes");

// one candidate correction of the moving submap, and the sensor position of one of its scans under one candidate (k_occ_fit_merged)
struct FitCandidate
{
  double c, s, tx, ty;       // cos / sin of the candidate's yaw (host libm), translation
};
struct FitSensor
{
  double sx, sy;             // GetSensorAt(transformed corrected pose): entry candidate * n_scans + scan
};
static_assert(sizeof(FitCandidate) == 32 && sizeof(FitSensor) == 16, "records = 4 and 2 words of 8 bytes");
// the six counters of one candidate, in this order (kh_merge_fit_t's first six fields)
enum : int32_t {kFitPassUnknown = 0, kFitPassOccupied = 1, kFitPassFree = 2, kFitHitsUnknown = 3, kFitHitsOccupied = 4, kFitHitsFree = 5, kFitCounters = 6};

// the grids of a live map: lattice cells [ox, ox + width) x [oy, oy + height), row stride ws = (width + 7) & ~7
struct LiveWindow
{
  int32_t ox, oy, width, height, ws;
  uint32_t * pass;
  uint32_t * hits;
  uint8_t * cells;
};

// a kh_map_view as k_map_seeds and k_map_fit read it: lattice cells [ox, ox + width) x [oy, oy + height) of cell states, the lattice's
// anchor and scale
struct MapWindow
{
  const uint8_t * cells;
  int32_t ox, oy, width, height, ws;
  double ax, ay, scale;
};
inline MapWindow window_of(const kh_map_view & v)
{
  return MapWindow{static_cast<const uint8_t *>(v.device_cells), v.ox, v.oy, v.width, v.height, v.width_step, v.anchor[0], v.anchor[1], v.scale};
}

// what the live map classifies a scan of its mapper by: the sensor pose; and the scan's box (the default anchor)
struct SensorView
{
  int32_t id;
  double sensor[3];
  double bbox[4];
};

enum : int32_t {kDeltaAdd = 0, kDeltaSub = 1, kDeltaMove = 2};

// one scan of a delta table (k_occ_trace_delta)
struct DeltaRecord
{
  const double * points;     // ADD / MOVE: 2 * n_beams unfiltered point readings, device memory (the mapper's resident copy)
  const double * ranges;     // ADD / MOVE: n_beams range readings, device memory
  double sx, sy;             // ADD / MOVE: sensor position
  int32_t kind;              // kDeltaAdd / kDeltaSub / kDeltaMove
  int32_t slot;              // the scan's slot of the log
  int32_t old_cx, old_cy;    // MOVE: the sensor cell the log holds (the host keeps a copy: the kernel overwrites the log's)
};
static_assert(sizeof(DeltaRecord) == 48, "one record = 6 x 8 bytes");

// The log: one slot per scan of (2 + 2 * n_beams) int32 words.
//   word 0, 1            sensor cell x, y on the lattice
//   word 2 + 2 i         beam i: end cell x on the lattice
//   word 3 + 2 i         beam i: bit 0 = the beam was kept (traced), bit 1 = its end point counts as a hit,
//                                bits 2..31 = end cell y - sensor cell y (two's complement; the size cap of the window bounds it
//                                far below 2^29)
inline int64_t live_log_slot_words(int32_t n_beams) {return 2 + 2 * static_cast<int64_t>(n_beams);}

// ---- the map feed (kh_map_feed_*) ----
constexpr int32_t kMapTile = KH_MAP_TILE;            // a tile: kMapTile x kMapTile lattice cells
constexpr int32_t kStripTiles = 4;                   // k_nav_feed: one wave compares a strip of 4 tiles, 64 cells x 16 rows
constexpr int32_t kTileWords = kMapTile * kMapTile / 4;      // dwords of a packed tile
static_assert(kMapTile == 16 && kStripTiles * kMapTile == 64, "k_nav_feed's lane layout is written for 64 x 16 strips");

// one launch of k_nav_feed: tile columns [tx0, tx1) and tile rows [ty0, ty1) of the lattice, inside both windows
struct NavFeedJob
{
  const uint8_t * cells;     // the live window's cell states, lattice cell (cells_ox, cells_oy) first, row stride cells_ws
  int8_t * published;        // the feed's published grid, lattice cell (pub_ox, pub_oy) first, row stride pub_ws
  int32_t cells_ox, cells_oy, cells_ws;
  int32_t pub_ox, pub_oy, pub_ws;
  int32_t tx0, ty0, tx1, ty1;
  uint32_t * count;          // changed tiles so far: a tile's slot of the two arrays below
  int32_t * tile_xy;         // 2 per slot: tx, ty
  uint32_t * packed;         // kTileWords per slot: the tile's new nav values, row-major
};

// ---- the launchers of a whole grid (occupancy.hip) ----
// the stream the grid's kernels run on: uploads a caller queues there are in place before the next trace reads them
void * occupancy_stream(kh_occupancy * g);
// AddScan for n_scans scans of n_beams beams whose readings are resident on the grid's device.  Returns after the trace (and
// everything queued on the stream before it) has finished.
int occupancy_add_resident(kh_occupancy * g, int32_t n_scans, const ResidentScan * scans, int32_t n_beams, double range_threshold,
  double min_range, double max_range);
// AddScan for the scans of a merge; scans[i].submap indexes submaps.  max_beams = the largest beam count, n_total_beams = the sum
// over the scans (the grid's beam counter).  Returns after the trace has finished.
int occupancy_add_merged(kh_occupancy * g, int32_t n_scans, const MergeScan * scans, int32_t n_submaps, const MergeSubmap * submaps,
  int32_t max_beams, int64_t n_total_beams);
// The fit of n_candidates corrections of ONE submap against the grid's cell states (kh_merge_fit): the submap's n_scans resident
// scans (their sx, sy are not read) of n_beams beams, sensors[candidate * n_scans + scan], the submap's laser gates.  out takes
// kFitCounters sums per candidate; *kernel_ms the kernel's time by events.  The grid is read, never written.  Returns after the
// kernel has finished and the sums are in `out`.
int occupancy_fit_merged(kh_occupancy * g, int32_t n_candidates, const FitCandidate * candidates, const FitSensor * sensors, int32_t n_scans,
  const ResidentScan * scans, int32_t n_beams, double range_threshold, double min_range, double max_range, uint64_t * out, double * kernel_ms);
// k_occ_to_nav of any strided cells on `stream`: d_out takes width * height values, rounded up to a dword
void cells_to_nav(void * stream, const uint8_t * d_cells, int32_t width, int32_t height, int32_t ws, uint32_t * d_out);

// ---- the launchers of a live map (occupancy_live.hip) ----
// n_records records on `stream`; counters[0] += lines walked, counters[1] += kept beams of MOVE records that were left alone
void live_trace_delta(void * stream, const LiveWindow & w, double anchor_x, double anchor_y, double scale, const DeltaRecord * d_records,
  int32_t n_records, int32_t n_beams, double range_threshold, double min_range, double max_range, int32_t * d_log,
  unsigned long long * d_counters);
// k_occ_update's rule over window columns [x0, x0 + w) and rows [y0, y0 + h) (columns may reach into the row padding)
void live_update_cells(void * stream, const LiveWindow & w, int32_t x0, int32_t y0, int32_t rect_w, int32_t rect_h, uint32_t min_pass,
  double threshold);
// k_nav_feed over the job's tiles on `stream`: every tile whose nav values differ from the published grid takes a slot, in no
// particular order.  The caller has set *job.count to 0 and holds room for every tile of the job.
void nav_feed(void * stream, const NavFeedJob & job);

// ---- a map view's kernels (occupancy_map.hip; kh_map_seeds, kh_map_fit, kh_map_localizer_*) ----
// a stream, two events and one growing device buffer on a device: what the launchers below work with.  nullptr = it could not be made.
struct MapWork;
MapWork * map_work_create(int32_t device);
void map_work_destroy(MapWork * w);
// KH_OK for a view the two kernels can read (kh_matcher_add_map's test without the device comparison), else KH_ERR_INVALID_ARG and its text
int map_view_check(const kh_map_view * v);
// ... and the test itself, without the text: 0, or which of its three refusals (what a device-free check can state too)
enum : int32_t {kViewOk = 0, kViewMalformed = 1, kViewTooLarge = 2, kViewLeavesLattice = 3};
inline int32_t map_view_refusal(const kh_map_view * v)
{
  if (!v || !v->device_cells || v->width <= 0 || v->height <= 0 || v->width_step < v->width || !std::isfinite(v->scale) || !(v->scale > 0.0) ||
    !std::isfinite(v->anchor[0]) || !std::isfinite(v->anchor[1])) {return kViewMalformed;}
  if (static_cast<int64_t>(v->width_step) * v->height > (1ll << 31) - 4096) {return kViewTooLarge;}
  if (static_cast<int64_t>(v->ox) + v->width > INT32_MAX || static_cast<int64_t>(v->oy) + v->height > INT32_MAX) {return kViewLeavesLattice;}
  return kViewOk;
}
// k_map_seeds over n_blocks = nbx * nby blocks of `pitch` cells, block column bx0 / block row by0 first: local takes one int32 per
// block, row-major -- the row-major index of the block's seed inside the block, or -1.  *kernel_ms: the kernel by events.
int map_seed_blocks(MapWork * w, const kh_map_view & v, int32_t pitch, int64_t bx0, int64_t by0, int64_t nbx, int64_t nby, int32_t * local,
  double * kernel_ms);
// k_map_fit: n_beams ranges, per pose 2 * n_beams point readings and the sensor's (x, y); counts takes kFitCounters sums per pose.
// The caller has checked the laser and the poses (fit_inputs_check).
int map_fit_counts(MapWork * w, const kh_map_view & v, int32_t n_beams, const double * ranges, int32_t n_poses, const double * points,
  const double * sensor_xy, double range_threshold, double min_range, double max_range, uint64_t * counts, double * kernel_ms);

// ---- the expected scan of a map (occupancy_map.hip; kh_map_raycast) ----
// The cells of TraceLine((x0, y0), (x1, y1)) OUTWARD from (x0, y0), one per step s = 0 .. length.  TraceLine walks its long axis
// upward, so where (x0, y0) has the larger long coordinate it starts at the far end -- and a line traced from the other end is not the
// mirror image: half-way between two rows the walk steps (2 error >= dx), the mirrored walk would step one cell later.  Its error
// at the last cell is k dy - dx floor(k dy / dx + 1 / 2) at k = dx, which is 0: the walk can be run backwards from its own end with no
// division.  With the sign of the error flipped the backward recurrence is the forward one with the comparison made strict, so one
// recurrence serves both directions: error += dy; step when 2 error + bias > dx, bias 1 where TraceLine starts at (x0, y0), else 0.
// (tests/map_align_plan_check.cpp walks every short line against TraceLine on the CPU.)
struct RayWalk
{
  int32_t a, b;              // the current cell: long-axis and short-axis coordinate
  int32_t step_a, step_b;    // +-1: towards (x1, y1)
  int32_t dx, dy, bias, error;
  bool steep;
  KH_HOST_DEVICE RayWalk(int32_t x0, int32_t y0, int32_t x1, int32_t y1)
  {
    const int64_t ex = static_cast<int64_t>(x1) - x0, ey = static_cast<int64_t>(y1) - y0;
    steep = (ey < 0 ? -ey : ey) > (ex < 0 ? -ex : ex);
    a = steep ? y0 : x0; b = steep ? x0 : y0;
    const int64_t ea = steep ? ey : ex, eb = steep ? ex : ey;
    dx = static_cast<int32_t>(ea < 0 ? -ea : ea); dy = static_cast<int32_t>(eb < 0 ? -eb : eb);
    step_a = ea < 0 ? -1 : 1; step_b = eb < 0 ? -1 : 1;
    bias = ea < 0 ? 0 : 1;
    error = 0;
  }
  KH_HOST_DEVICE int32_t length() const {return dx;}
  KH_HOST_DEVICE int32_t x() const {return steep ? b : a;}
  KH_HOST_DEVICE int32_t y() const {return steep ? a : b;}
  KH_HOST_DEVICE void next()
  {
    error += dy;
    if (2 * error + bias > dx) {b += step_b; error -= dx;}
    a += step_a;
  }
};
// one beam's answer of k_map_raycast: the cell the walk ended on, its step, and the KH_RAY_ code
struct alignas(16) RayCell {int32_t i, j, steps, code;};
static_assert(sizeof(RayCell) == 16, "one int4 per beam");
// k_map_raycast: per pose the 2 * n_beams far points (kh_scan_points of a scan whose readings are all range_threshold) and the sensor's
// (x, y); out takes n_poses * n_beams answers, pose-major.  The caller has checked the laser and the poses (fit_inputs_check) and
// max_unknown >= -1.
int map_raycast_cells(MapWork * w, const kh_map_view & v, int32_t n_beams, int32_t n_poses, const double * points, const double * sensor_xy,
  int32_t max_unknown, RayCell * out, double * kernel_ms);
// kh_map_raycast's argument checks but `out` (KH_OK, or KH_ERR_INVALID_ARG and its text), and the call itself on a caller's work
// buffers once they passed: the far points (n_beams libm sincos per pose, on the worker pool), the launch, the ranges
int map_raycast_check(const kh_map_view * view, const kh_laser * laser, int32_t n_poses, const double * sensor_poses, int32_t max_unknown);
int map_raycast(MapWork * w, const kh_map_view & v, const kh_laser & laser, int32_t n_poses, const double * sensor_poses, int32_t max_unknown,
  double no_return, kh_ray_t * out, double * kernel_ms);

// ---- two maps merged into one (occupancy_map.hip; kh_map_merge_*; the handle and its buffers: map_merge.cpp) ----
// one launch of k_map_merge: the output window on the target's lattice, the inverse correction, the samples of a cell
constexpr int32_t kMergeTileWidth = 64, kMergeTileHeight = 16;     // cells of a workgroup's tile: 16 dwords x 16 rows = 256 threads
struct MergeJob
{
  MapWindow target, moving;
  int32_t ox, oy, width, height, ws;      // the output window; ws a multiple of 4
  int32_t footprint, conflict;            // 1 .. 4; KH_MERGE_CONFLICT_
  double c, s, tx, ty;                    // inverse(correction): cos / sin of its yaw (host libm), translation
  double d[4];                            // the sample offsets of one axis (merge_sample_offsets)
};
// k_map_known_box on `stream`: d_box = (i0, j0, i1, j1), set by the caller to (INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN), takes the
// inclusive lattice box of the window cells of state != 0
void map_known_box(void * stream, const kh_map_view & v, int32_t * d_box);
// k_map_merge on `stream`: d_cells and d_codes take one byte per cell of the strided output window (the padding 0), d_counts[6]
// (zeroed by the caller) the window cells by counter (map_merge_plan.hpp's order).  Neither input is written.
void map_merge_cells(void * stream, const MergeJob & job, uint8_t * d_cells, uint8_t * d_codes, unsigned long long * d_counts);

// ---- the distance field of a map (occupancy_field.hip; kh_map_field_*; the handle and its buffers: map_field.cpp) ----
// The field's own arrays on its window, all of row stride ws = field_stride(width), a multiple of 4: the copied cell states (the
// padding 0), the column distances, the values.  As a window of the lattice it is what cell_at() indexes.
struct FieldWindow
{
  const uint8_t * cells;
  uint16_t * g;                // the column pass' answer; only k_field_columns and k_field_rows touch it
  uint32_t * d2;
  int32_t ox, oy, width, height, ws;
  double ax, ay, scale;
  int32_t radius, obstacles;   // R; KH_FIELD_OBSTACLE_
};
// k_field_columns on `stream`: g[row][col] = the distance along the column to the nearest obstacle of that column, kFieldNoColumn where
// there is none (within R, for R > 0).  One launch whatever the map holds.
void field_columns(void * stream, const FieldWindow & f);
// k_field_rows on `stream`: d2 from g; d_counts[kFieldCounters] (zeroed by the caller) takes the cells of value 0, those of
// KH_FIELD_FAR, and the largest other value.  false = the launch could not be prepared (the row's LDS)
bool field_rows(void * stream, const FieldWindow & f, unsigned long long * d_counts);
// k_field_costs on `stream`: d_out (stride ws) from the values through d_table (rt2 + 1 entries) and the unknown policy
void field_costs(void * stream, const FieldWindow & f, const uint8_t * d_table, uint32_t rt2, int32_t track_unknown, int32_t inflate_unknown,
  uint8_t * d_out);
// k_field_lookup on `stream`: n points (x, y) -> their value and KH_CLEAR_ status
void field_lookup(void * stream, const FieldWindow & f, int32_t n, const double * d_xy, uint32_t * d_d2, int32_t * d_status);
// k_field_score on `stream`: k_map_fit's tables and launch shape; d_sums[kScoreCounters] per pose, zeroed by the caller.  The caller
// has checked the laser and the poses (fit_inputs_check) and blocks_per_pose(n_beams, n_poses).
void field_score(void * stream, const FieldWindow & f, const double * d_ranges, const double * d_points, const double * d_sensors, int32_t n_beams,
  int32_t n_poses, double range_threshold, double min_range, double max_range, uint32_t t2, unsigned long long * d_sums);

// ---- a field that follows its map (occupancy_field_update.hip; kh_map_field_update; the rules: map_field_update_plan.hpp) ----
// window columns [x0, x1) and rows [y0, y1)
struct FieldRect {int32_t x0, y0, x1, y1;};
// what k_field_changed leaves: two inclusive boxes (x0, y0, x1, y1) in window columns / rows -- the cells whose state changed, the
// cells whose obstacle-ness changed; the caller sets both to (INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN) -- and, as one uint64 in
// the last two words, the cells compared (set to 0)
enum : int32_t {kChangedStates = 0, kChangedObstacles = 4, kChangedCount = 8, kChangedWords = 10};
// k_field_changed on `stream`: the view's cells (row stride view_ws, first window cell first) against d_snapshot (the field's copy,
// f.cells) over `r`; the copy takes the view's cells
void field_changed(void * stream, const FieldWindow & f, uint8_t * d_snapshot, const uint8_t * d_view_cells, int32_t view_ws, const FieldRect & r,
  int32_t * d_result);
// k_field_columns_band on `stream`, capped fields only: k_field_columns' answer on the whole quads of columns that hold [x0, x1), rows
// [y0, y1), cut into bands of band_rows >= 1 rows
void field_columns_band(void * stream, const FieldWindow & f, const FieldRect & r, int32_t band_rows);
// k_field_rows_region on `stream`, capped fields only: k_field_rows' values for the cells of `r`, no counters.  false = the launch
// could not be prepared
bool field_rows_region(void * stream, const FieldWindow & f, const FieldRect & r);
// k_field_costs_rect on `stream`: k_field_costs' costs of the cells of `r`, row-major of row stride out_ws (a multiple of 4)
void field_costs_rect(void * stream, const FieldWindow & f, const FieldRect & r, const uint8_t * d_table, uint32_t rt2, int32_t track_unknown,
  int32_t inflate_unknown, uint8_t * d_out, int32_t out_ws);
// k_field_count on `stream`: k_field_rows' three counters (zeroed by the caller) from the values as they stand
void field_count(void * stream, const FieldWindow & f, unsigned long long * d_counts);
// the live binding, between map_field.cpp and live_map.cpp: the live map a field follows (nullptr: none, or destroyed under it);
// an empty field on the view's lattice that its first update builds; the live map forgets a field that is being destroyed
kh_live_map * map_field_live(const kh_map_field * f);
void map_field_set_live(kh_map_field * f, kh_live_map * g);
int map_field_create_empty(const kh_map_view & view, const kh_map_field_params & params, const char * who, kh_map_field ** out);
void live_map_forget_field(kh_live_map * g, kh_map_field * f);
// what a reader of another module takes of a field (map_regions.cpp): its arrays as they stand, its device
FieldWindow map_field_window(const kh_map_field * f);
int32_t map_field_device(const kh_map_field * f);

// ---- map regions (occupancy_regions.hip; kh_map_regions_*; the handle and its buffers: map_regions.cpp; the
// rules: map_regions_plan.hpp) ----
// A component's record as the kernels keep it: integers only, the box as inclusive window columns / rows, the anchor as its key
// dist2 << 32 | window index.  k_region_assign writes the first two fields and the neutral elements of the rest.
struct RegionRecord
{
  uint32_t root, n_cells;
  int32_t x0, y0, x1, y1;
  unsigned long long sum_i, sum_j;
  uint32_t max_d2, n_other, link, pad;
  unsigned long long anchor_key;
};
// One of the two sets on the window, every array dense (row stride `width`): label -- a cell's parent, then its root, then its id
// (KH_REGION_NONE off the mask throughout); count -- cells per root, then the root's id; the records of the kept components.
struct RegionSet
{
  uint32_t * label;
  uint32_t * count;
  RegionRecord * records;
  uint32_t minimum, maximum;
};
struct RegionJob
{
  FieldWindow f;               // the field's cells and values: read only
  RegionSet set[2];            // KH_REGIONS, KH_FRONTIERS
  uint32_t rc2;                // Rc * Rc
  int32_t conn8;               // 1: eight neighbours
  int32_t * unit;              // region_grid().units + 1 words: the compaction's counts, then their exclusive prefix
  unsigned long long * counters;   // kRegionCounters words, zeroed by the caller; [kRegionError] != 0: a watchdog ended a walk
};
// k_region_tiles on `stream`: both masks, the labels of both sets inside every 64 x 16 tile, the two mask counters
void region_tiles(void * stream, const RegionJob & job);
// k_region_seams on `stream`, once per set: the unions across tile borders
void region_seams(void * stream, const RegionJob & job);
// k_region_flatten on `stream`, once per set: label = root, count[root] = cells (count zeroed by the caller)
void region_flatten(void * stream, const RegionJob & job);
// k_region_roots (count, fill), the unit scan, k_region_ids on `stream`, per set: the kept roots numbered in row-major order, their
// records begun, label = id
void region_compact(void * stream, const RegionJob & job);
// k_region_records, then k_region_anchor on `stream`: both sets in one launch each
void region_records(void * stream, const RegionJob & job);
void region_anchors(void * stream, const RegionJob & job);
// k_region_lookup on `stream`: n points (x, y) -> the id of their cell in `ids` (dense) and a KH_REGION_AT_ / _OUTSIDE status
void region_lookup(void * stream, const FieldWindow & f, const uint32_t * d_ids, int32_t n, const double * d_xy, uint32_t * d_id, int32_t * d_status);
// k_map_changed_scan on `stream` (occupancy_changes.hip): d_unit[0 .. n_units) -> its exclusive prefix in place, d_unit[n_units] the sum
void unit_scan(void * stream, int32_t * d_unit, int64_t n_units);

// ---- travel costs (occupancy_travel.hip; kh_map_travel_*; the handle and its buffers: map_travel.cpp; the
// rules: map_travel_plan.hpp) ----
// The analysis on the window, both arrays dense (row stride `width`): q -- a cell's weight, 0 where it is not traversable; v -- its
// value.  The lattice is the field's (f.cells, f.g, f.d2 are read by travel_weights only).
struct TravelJob
{
  FieldWindow f;
  uint16_t * q;
  uint32_t * v;
  int32_t conn8, cut_corners;
  uint32_t * flags;            // 2 * tiles words: the tiles to run in launches of even / odd parity
  unsigned long long * counters;   // kTravelCounters words; [kTravelError] != 0: a watchdog ended a loop, or a path found no way on
};
// one answer of k_travel_lookup, one head of k_travel_paths
struct alignas(16) TravelAt {int32_t status; uint32_t value; int32_t x, y;};
struct alignas(16) TravelHead {int32_t status, n_cells; uint32_t cost, start_cell;};
static_assert(sizeof(TravelAt) == 16 && sizeof(TravelHead) == sizeof(kh_travel_path), "one int4 per answer; a head is the ABI's record");
// k_travel_weights on `stream`: q from the field through d_table (rt2 + 1 entries; not read when cost_weight == 0);
// counters[kTravelTraversable] (zeroed by the caller) takes the cells of weight > 0
void travel_weights(void * stream, const TravelJob & job, uint32_t rc2, const uint8_t * d_table, uint32_t rt2, uint32_t neutral_cost, uint32_t cost_weight);
// k_travel_goals on `stream`: n goals (x, y) -> their status and cell (window index, KH_TRAVEL_FAR without one); v = 0 at every goal
// cell; the goal's tile and its neighbours are flagged for the first launch.  The caller has set v to KH_TRAVEL_FAR and the flags to 0.
void travel_goals(void * stream, const TravelJob & job, int32_t n, const double * d_xy, int32_t snap, int32_t * d_status, uint32_t * d_cell);
// k_travel_relax on `stream`: launch number `round` (its parity picks the flags it reads); *d_any (zeroed by the caller) becomes 1
// where a tile flagged a neighbour for the next launch; counters[kTravelRuns] += the tiles that ran
void travel_relax(void * stream, const TravelJob & job, uint32_t round, uint32_t * d_any);
// k_travel_count on `stream`: counters[kTravelReached] and [kTravelMaxValue] (zeroed by the caller) from the values as they stand
void travel_count(void * stream, const TravelJob & job);
// k_travel_lookup on `stream`: n points (x, y) -> one TravelAt each
void travel_lookup(void * stream, const TravelJob & job, int32_t n, const double * d_xy, int32_t snap, TravelAt * d_out);
// k_travel_paths on `stream`: n starts -> one head each and, where d_cells is not null, the cells of path k from 2 * k * max_cells on
void travel_paths(void * stream, const TravelJob & job, int32_t n, const double * d_xy, int32_t snap, int32_t max_cells, TravelHead * d_heads,
  int32_t * d_cells);

// ---- visibility (occupancy_visibility.hip; kh_map_visibility_*; the handle and its buffers: map_visibility.cpp;
// the rules: map_visibility_plan.hpp) ----
// the words the kernels leave for the host, at the head of a call's buffer: a far cell beyond the reach; a select's state
struct alignas(16) VisHead {uint32_t error, done, n_picked, current;};
static_assert(sizeof(VisHead) == 16 && sizeof(kh_visibility_t) == 40, "one int4; a record is the ABI's");
// One launch of k_vis_gain: workgroup p takes pose p of the tables (k_map_raycast's: 2 * n_beams far points and the sensor's (x, y)
// per pose).  head: never null.  picked: null outside a select -- there a pose whose word is set, and every pose once head->done is
// set, leaves at once.
struct VisJob
{
  MapWindow g;
  const double * points;
  const double * sensors;
  int32_t n_beams, max_unknown, reach;
  uint32_t w_unknown, w_free, w_occupied;
  uint32_t * mask;             // the covered mask: read by a gain, ORed into by a commit
  VisHead * head;
  const uint32_t * picked;
};
// k_vis_gain on `stream`, counting: one record per pose into d_out.  skip: read a bitmap word before the OR and leave the OR out where
// the bit is set.  false = the launch could not be prepared (the bitmap's LDS)
bool vis_gain(void * stream, const VisJob & job, int32_t n_poses, bool skip, kh_visibility_t * d_out);
// k_vis_gain on `stream`, committing: Seen(p) of n_poses poses ORed into the mask; from_head: one workgroup, the pose head->current
// (nothing where head->done is set)
bool vis_commit(void * stream, const VisJob & job, int32_t n_poses, bool skip, bool from_head);
// k_vis_best on `stream`: the unpicked candidate of the largest gain, ties to the smallest index -> d_picks / d_gains [head->n_picked],
// its picked word, head->current; head->done where that gain is below min_gain
void vis_best(void * stream, const kh_visibility_t * d_records, int32_t n, uint32_t min_gain, uint32_t * d_picked, VisHead * d_head, uint32_t * d_picks,
  uint32_t * d_gains);

// ---- footprints (occupancy_footprint.hip; kh_map_footprint_*; the handle and its buffers: map_footprint.cpp;
// the rules: map_footprint_plan.hpp) ----
// one pose of k_footprint_poses as the host states it: whether a vertex left the lattice, the pose's own cell, the vertex cells
struct alignas(16) FootPose {int32_t lattice, pad, cx, cy; int32_t v[32];};
static_assert(sizeof(FootPose) == 144 && sizeof(kh_footprint_t) == 32, "nine int4 per pose; a record is the ABI's");
// the handle's snapshot (f.cells and f.d2 are its own copies, f.g is null), the polygon's size, the call's error word
struct FootJob
{
  FieldWindow f;
  int32_t n_vertices, reach;
  uint32_t * error;            // set where a vertex cell lies beyond the reach of its pose's cell
};
// k_footprint_poses on `stream`: one record per pose into d_out
void footprint_poses(void * stream, const FootJob & job, int32_t n, const FootPose * d_poses, kh_footprint_t * d_out);
// k_footprint_layer on `stream`: d_table is foot_layer_table's; d_masks (may be null) takes width * height words, dense; d_counts
// (34 words, zeroed by the caller) the summary's counters in kh_footprint_layer_t's order
void footprint_layer(void * stream, const FootJob & job, int32_t n_headings, int32_t max_status, const int32_t * d_table, uint32_t * d_masks,
  unsigned long long * d_counts);

// ---- a change layer's kernels (occupancy_changes.hip; kh_map_changes_*; the handle and its buffers: map_changes.cpp) ----
// the layer's two counter grids on the window of its view, row stride the view's width_step
struct ChangeLayer
{
  uint32_t * pass;
  uint32_t * hits;
};
enum : int32_t {kChangeCodes = 6};                    // KH_CELL_UNOBSERVED .. KH_CELL_DISCOVERED_FREE
// the units of the changed-cell list: 64 consecutive cells of a row of the window
inline int64_t change_units(int32_t width, int32_t height) {return (static_cast<int64_t>(width) + 63) / 64 * height;}
// k_map_observe on `stream`: n_scans scans of n_beams beams -- d_ranges n_scans * n_beams, d_points 2 per beam (kh_scan_points at the
// scan's pose), d_sensors 2 per scan -- add to the layer; d_labels takes 2 int32 per beam.  The caller has checked the laser and the
// poses (fit_inputs_check), blocks_per_pose(n_beams, n_scans) and 0 <= tolerance <= kMaxEndTolerance.
void map_observe(void * stream, const kh_map_view & v, const ChangeLayer & layer, const double * d_ranges, const double * d_points,
  const double * d_sensors, int32_t n_scans, int32_t n_beams, double range_threshold, double min_range, double max_range, int32_t tolerance,
  int32_t * d_labels);
// k_map_decay on `stream`: both grids >>= shift
void map_decay(void * stream, const kh_map_view & v, const ChangeLayer & layer, int32_t shift);
// k_map_diff on `stream`: d_codes and d_patched take one byte per cell of the strided window (the padding 0), d_counts[kChangeCodes]
// (zeroed by the caller) the window cells by code
void map_diff(void * stream, const kh_map_view & v, const ChangeLayer & layer, uint32_t min_pass, double threshold, uint8_t * d_codes,
  uint8_t * d_patched, unsigned long long * d_counts);
// the cells of code >= 2 in row-major order on `stream`: d_unit holds change_units() + 1 int32 (it ends as the exclusive prefix of the
// units' counts, the total last); d_list takes (lattice i, lattice j, code) of the first `cap` cells
void map_changed_cells(void * stream, const kh_map_view & v, const uint8_t * d_codes, int32_t * d_unit, int32_t * d_list, int32_t cap);

#ifdef __HIP__
// ---- what the module's host files do with the device the same way (absent from a build without HIP: tests/live_map_plan_check.cpp);
// set_error and require_device: host_common.hpp ----
// makes *buf a device buffer of at least `need` bytes once `stream` has drained: one that is too small is replaced by one of `cap`
// bytes (what it held is not kept).  false = the allocation failed, and the buffer is gone.
inline bool grow_device(hipStream_t stream, void ** buf, size_t * have, size_t need, size_t cap)
{
  if (need <= *have) {return true;}
  (void)hipStreamSynchronize(stream);
  if (*buf) {(void)hipFree(*buf); *buf = nullptr;}
  *have = 0;
  if (hipMalloc(buf, cap) != hipSuccess) {(void)hipGetLastError(); return false;}
  *have = cap;
  return true;
}

// the same for a buffer whose first `used` bytes are kept (the live map's log; nothing is in flight on it between two updates).
// hipErrorOutOfMemory = the allocation failed and the buffer is as it was; any other error = the copy failed, likewise.
inline hipError_t grow_device_keeping(void ** buf, size_t * have, size_t need, size_t cap, size_t used)
{
  if (need <= *have) {return hipSuccess;}
  void * d_new = nullptr;
  if (hipMalloc(&d_new, cap) != hipSuccess) {(void)hipGetLastError(); return hipErrorOutOfMemory;}
  const hipError_t err = used > 0 ? hipMemcpy(d_new, *buf, used, hipMemcpyDeviceToDevice) : hipSuccess;
  if (err != hipSuccess) {(void)hipFree(d_new); return err;}
  (void)hipFree(*buf);
  *buf = d_new; *have = cap;
  return hipSuccess;
}

// ---- the launch sequence of the module's timed kernels, stated once (occupancy.hip, occupancy_map.hip, map_changes.cpp): a stream, two events and one
// growing device buffer; the buffer carved into the parts of a launch and the parts uploaded; the kernel between the two events, the
// download, the wait, the elapsed time, a failure reported under the caller's name ----
struct DeviceWork
{
  int32_t device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  uint8_t * d = nullptr; size_t cap = 0;               // a launch's tables and answers (bytes)
};

// false = the stream or an event could not be made (work_close the rest)
inline bool work_open(DeviceWork & w, int32_t device)
{
  w.device = device;
  return hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreate(&w.ev[0]) == hipSuccess && hipEventCreate(&w.ev[1]) == hipSuccess;
}

inline void work_close(DeviceWork & w)
{
  (void)hipSetDevice(w.device);
  if (w.stream) {(void)hipStreamSynchronize(w.stream);}
  (void)hipFree(w.d);
  if (w.ev[0]) {(void)hipEventDestroy(w.ev[0]);}
  if (w.ev[1]) {(void)hipEventDestroy(w.ev[1]);}
  if (w.stream) {(void)hipStreamDestroy(w.stream);}
}

// One part of a launch's buffer: `bytes` bytes that begin as a copy of `host`, as zeros (kZeros), or as they are (nullptr: an answer).
// work_stage fills in `d`.  The parts lie in the order given; every size a multiple of the strictest alignment among them.
struct Part
{
  const void * host;
  size_t bytes;
  uint8_t * d = nullptr;
  template <typename T> T * as() const {return reinterpret_cast<T *>(d);}
};
inline const void * const kZeros = &kZeros;

// Grows the buffer to the parts' sum (to half as much again where `spare`: a caller whose launches creep upward), carves it and
// queues the uploads.  KH_ERR_HIP with "`who`: `what` allocation failed" where the buffer could not be made, with HIP's text for an upload.
template <size_t N>
int work_stage(DeviceWork & w, const char * who, const char * what, bool spare, Part (&parts)[N])
{
  size_t bytes = 0;
  for (const Part & p : parts) {bytes += p.bytes;}
  if (!grow_device(w.stream, reinterpret_cast<void **>(&w.d), &w.cap, bytes, spare ? bytes + bytes / 2 : bytes)) {
    set_error(std::string(who) + ": " + what + " allocation failed");
    return KH_ERR_HIP;
  }
  uint8_t * at = w.d;
  for (Part & p : parts) {
    p.d = at; at += p.bytes;
    const hipError_t err = p.host == kZeros ? hipMemsetAsync(p.d, 0, p.bytes, w.stream) :
      p.host ? hipMemcpyAsync(p.d, p.host, p.bytes, hipMemcpyHostToDevice, w.stream) : hipSuccess;
    if (err != hipSuccess) {
      (void)hipStreamSynchronize(w.stream);
      set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
      return KH_ERR_HIP;
    }
  }
  return KH_OK;
}

// launch() between the two events, the download of `answer` (nullptr: none) into `out`, the wait for all of it; *kernel_ms = the
// time between the events.  A failure is reported under `who`.
template <typename Launch>
int work_run(DeviceWork & w, const char * who, Launch launch, const Part * answer, void * out, double * kernel_ms)
{
  (void)hipEventRecord(w.ev[0], w.stream);
  launch();
  (void)hipEventRecord(w.ev[1], w.stream);
  const bool copied = !answer || hipMemcpyAsync(out, answer->d, answer->bytes, hipMemcpyDeviceToHost, w.stream) == hipSuccess;
  if (hipStreamSynchronize(w.stream) != hipSuccess || !copied) {
    set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
  if (kernel_ms) {*kernel_ms = ms;}
  return KH_OK;
}
#endif
}  // namespace kh
