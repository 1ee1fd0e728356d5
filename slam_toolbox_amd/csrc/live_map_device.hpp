// What live_map.cpp (host side of kh_live_map_*) and occupancy.hip (k_occ_trace_delta, k_occ_update_rect) share.  Not part of the
// public ABI (include/karto_hip.h).  The lattice, the window and the log are stated in DESIGN.md section 7b.
#pragma once
#include <cstdint>

namespace kh
{
// the grids of a live map: lattice cells [ox, ox + width) x [oy, oy + height), row stride ws = (width + 7) & ~7
struct LiveWindow
{
  int32_t ox, oy, width, height, ws;
  uint32_t * pass;
  uint32_t * hits;
  uint8_t * cells;
};

enum : int32_t {kDeltaAdd = 0, kDeltaSub = 1, kDeltaMove = 2};

// one scan of a delta table
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

// n_records records on `stream`; counters[0] += lines walked, counters[1] += kept beams of MOVE records that were left alone
void live_trace_delta(void * stream, const LiveWindow & w, double anchor_x, double anchor_y, double scale, const DeltaRecord * d_records,
  int32_t n_records, int32_t n_beams, double range_threshold, double min_range, double max_range, int32_t * d_log,
  unsigned long long * d_counters);
// k_occ_update's rule over window columns [x0, x0 + w) and rows [y0, y0 + h) (columns may reach into the row padding)
void live_update_cells(void * stream, const LiveWindow & w, int32_t x0, int32_t y0, int32_t rect_w, int32_t rect_h, uint32_t min_pass,
  double threshold);
}  // namespace kh
