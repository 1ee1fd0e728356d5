// The kernels of a live occupancy map (kh_live_map_*, kh_map_feed_*; DESIGN.md sections 7b and 7c) and their launchers: the trace of a
// table of scan deltas into a window of the lattice, UpdateCell over the rectangle a delta can have touched, and the map feed's
// compare-and-pack.  The handle, its window and its log: live_map.cpp; what the kernels share with the other trace kernels:
// occupancy_walk.hpp.
#include "live_map_plan.hpp"
#include "occupancy_walk.hpp"

namespace kh
{
// k_occ_update's rule (UpdateCell) over a rectangle of a live map's window (kh_live_map_update: the cells a delta can have touched)
__global__ __launch_bounds__(256) void k_occ_update_rect(LiveWindow g, int32_t x0, int32_t y0, int32_t rect_w, int32_t rect_h, uint32_t min_pass,
  double threshold)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)rect_w * rect_h) {return;}
  const int64_t y = k / rect_w, x = k - y * rect_w;
  occ_update_cell(g.pass, g.hits, g.cells, (x0 + x) + (y0 + y) * (int64_t)g.ws, min_pass, threshold);
}

// ---- the live map's trace (kh_live_map_update) ----
// The work layout of k_occ_trace_resident -- one wave per run of 64 neighbouring beams of one scan -- over a table of ADD / SUB /
// MOVE records (occupancy_device.hpp).  ADD traces from the resident readings and writes the scan's slot of the log; SUB walks the
// logged lines with -1 and reads nothing else; MOVE compares the beam's new trace record with the logged one and walks (old line
// -1, new line +1) only where something differs.  One scan is one record, so no two waves touch the same log words: a beam's two
// words belong to its lane, and the slot's sensor cell is written by beam 0's lane and read by SUB records only (MOVE gets the old
// cell in its record).
__global__ __launch_bounds__(256) void k_occ_trace_delta(
  LiveWindow g, double ax, double ay, double scale, const DeltaRecord * __restrict__ records, int32_t n_records, int32_t n_beams,
  int32_t runs_per_scan, double range_threshold, double min_range, double max_range, int32_t * __restrict__ log, int64_t slot_words,
  unsigned long long * __restrict__ counters)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int32_t lane = threadIdx.x & 63;
  const int64_t s = wave / runs_per_scan;
  if (s >= n_records) {return;}
  const int32_t i = (int32_t)(wave - s * runs_per_scan) * 64 + lane;
  if (i >= n_beams) {return;}
  const DeltaRecord rec = records[s];
  int32_t * const slot = log + rec.slot * slot_words;
  int2 * const entry = reinterpret_cast<int2 *>(slot + 2) + i;
  // the logged line (SUB, MOVE) and the new one (ADD, MOVE)
  int32_t ocx = rec.old_cx, ocy = rec.old_cy, ncx = 0, ncy = 0;
  int2 was = make_int2(0, 0), now = make_int2(0, 0);
  if (rec.kind != kDeltaAdd) {was = *entry;}
  if (rec.kind == kDeltaSub) {ocx = slot[0]; ocy = slot[1];}
  if (rec.kind != kDeltaSub) {
    const Beam b = occ_gate(rec.ranges[i], rec.points[2 * i], rec.points[2 * i + 1], rec.sx, rec.sy, range_threshold, min_range, max_range);
    ncx = occ_cell(rec.sx, ax, scale); ncy = occ_cell(rec.sy, ay, scale);
    if (b.kept) {now = make_int2(occ_cell(b.px, ax, scale), (int32_t)(((uint32_t)(occ_cell(b.py, ay, scale) - ncy) << 2) | (b.hit ? 3u : 1u)));}
  }
  const bool same = rec.kind == kDeltaMove && was.x == now.x && was.y == now.y && ocx == ncx && ocy == ncy;
  const bool walk_old = rec.kind != kDeltaAdd && !same && (was.y & 1);
  const bool walk_new = rec.kind != kDeltaSub && !same && (now.y & 1);
  if (walk_old) {occ_walk(CountCells<LiveWindow>{g, 0xFFFFFFFFu}, ocx, ocy, was.x, ocy + (was.y >> 2), (was.y & 2) != 0);}
  if (walk_new) {occ_walk(CountCells<LiveWindow>{g, 1u}, ncx, ncy, now.x, ncy + (now.y >> 2), (now.y & 2) != 0);}
  if (rec.kind != kDeltaSub) {
    if (!same) {*entry = now;}
    if (i == 0) {slot[0] = ncx; slot[1] = ncy;}
  }
  // lane 0 holds the run's first beam, so it is here whenever the wave is
  const int walked = __popcll(__ballot(walk_old)) + __popcll(__ballot(walk_new));
  const int skipped = __popcll(__ballot(same && (now.y & 1)));
  if (lane == 0) {
    if (walked) {atomicAdd(&counters[0], (unsigned long long)walked);}
    if (skipped) {atomicAdd(&counters[1], (unsigned long long)skipped);}
  }
}

// The map feed's compare-and-pack (kh_map_feed_poll).  One wave per STRIP of four horizontally adjacent
// tiles, 64 cells x 16 rows: a load instruction of the wave reads four whole 64-byte row segments.  A lane owns the dword column
// lane & 15 of the strip -- so tile (lane & 15) >> 2 -- and the rows lane >> 4, + 4, + 8, + 12.  It turns its four dwords of cell
// states into nav values, compares them with the same four dwords of the published grid, and a ballot masked per tile says which
// of the four tiles changed.  A changed tile takes a slot (one atomic per wave) and its lanes write the new values to the packed
// buffer and to the published grid, and the tile's coordinates; an unchanged tile writes nothing.  Slots are dealt in no order: the
// host sorts the coordinates.  Strips are aligned to 64 lattice cells, as both windows are, so every dword is aligned; the tiles
// of a strip outside [tx0, tx1) are not read.
__global__ __launch_bounds__(256) void k_nav_feed(NavFeedJob j, int32_t strip0, int32_t strips_x, int64_t n_strips)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wave >= n_strips) {return;}
  const int32_t lane = threadIdx.x & 63, col = lane & 15, row0 = lane >> 4, t = col >> 2;
  const int32_t sy = (int32_t)(wave / strips_x), sx = (int32_t)(wave - (int64_t)sy * strips_x);
  const int32_t tx = (strip0 + sx) * kStripTiles + t, ty = j.ty0 + sy;
  const bool active = tx >= j.tx0 && tx < j.tx1;
  const int64_t x = (int64_t)(strip0 + sx) * (kStripTiles * kMapTile) + 4 * col, y = (int64_t)ty * kMapTile + row0;
  const uint8_t * const src = j.cells + (x - j.cells_ox) + (y - j.cells_oy) * j.cells_ws;
  int8_t * const pub = j.published + (x - j.pub_ox) + (y - j.pub_oy) * j.pub_ws;
  uint32_t nav[4] = {0, 0, 0, 0};
  uint32_t differs = 0;                                 // (bitwise, not ||: all eight loads are issued before the first is waited for)
  if (active) {
#pragma unroll
    for (int32_t k = 0; k < 4; ++k) {
      nav[k] = occ_nav4(*reinterpret_cast<const uint32_t *>(src + (int64_t)(4 * k) * j.cells_ws));
      differs |= nav[k] ^ *reinterpret_cast<const uint32_t *>(pub + (int64_t)(4 * k) * j.pub_ws);
    }
  }
  const unsigned long long changed = __ballot(differs != 0);
  uint32_t flags = 0;                                   // bit t: tile t of the strip changed (its lanes: lane & 12 == 4 t)
#pragma unroll
  for (int32_t k = 0; k < kStripTiles; ++k) {flags |= (changed & (0x000F000F000F000Full << (4 * k))) ? 1u << k : 0u;}
  if (flags == 0) {return;}                             // (the whole wave leaves: nothing of the strip is written)
  uint32_t base = 0;
  if (lane == 0) {base = atomicAdd(j.count, (uint32_t)__popc(flags));}
  base = __shfl(base, 0);
  if (!((flags >> t) & 1u)) {return;}
  const int64_t slot = (int64_t)base + __popc(flags & ((1u << t) - 1u));
  uint32_t * const out = j.packed + slot * kTileWords + (col & 3);
#pragma unroll
  for (int32_t k = 0; k < 4; ++k) {
    out[(row0 + 4 * k) * (kMapTile / 4)] = nav[k];
    *reinterpret_cast<uint32_t *>(pub + (int64_t)(4 * k) * j.pub_ws) = nav[k];
  }
  if ((lane & 0x33) == 0) {j.tile_xy[2 * slot] = tx; j.tile_xy[2 * slot + 1] = ty;}
}

void live_trace_delta(void * stream, const LiveWindow & w, double anchor_x, double anchor_y, double scale, const DeltaRecord * d_records,
  int32_t n_records, int32_t n_beams, double range_threshold, double min_range, double max_range, int32_t * d_log,
  unsigned long long * d_counters)
{
  if (n_records <= 0 || n_beams <= 0) {return;}
  const int32_t runs = (n_beams + 63) / 64;
  hipLaunchKernelGGL(k_occ_trace_delta, dim3(blocks_of_runs(n_records, runs)), dim3(256), 0, static_cast<hipStream_t>(stream), w, anchor_x, anchor_y,
    scale, d_records, n_records, n_beams, runs, range_threshold, min_range, max_range, d_log, live_log_slot_words(n_beams), d_counters);
}

void live_update_cells(void * stream, const LiveWindow & w, int32_t x0, int32_t y0, int32_t rect_w, int32_t rect_h, uint32_t min_pass,
  double threshold)
{
  if (rect_w <= 0 || rect_h <= 0) {return;}
  const int64_t size = static_cast<int64_t>(rect_w) * rect_h;
  hipLaunchKernelGGL(k_occ_update_rect, dim3(static_cast<unsigned>((size + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w, x0, y0,
    rect_w, rect_h, min_pass, threshold);
}

void nav_feed(void * stream, const NavFeedJob & job)
{
  if (job.tx1 <= job.tx0 || job.ty1 <= job.ty0) {return;}
  // the strips of 4 tiles that hold tile columns [tx0, tx1): floor quotients, tiles left of the anchor are negative
  const int32_t strip0 = static_cast<int32_t>(floor_div(job.tx0, kStripTiles));
  const int32_t strips_x = static_cast<int32_t>(floor_div(job.tx1 - 1, kStripTiles)) - strip0 + 1;
  const int64_t n_strips = static_cast<int64_t>(strips_x) * (job.ty1 - job.ty0);
  hipLaunchKernelGGL(k_nav_feed, dim3(static_cast<unsigned>((n_strips + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), job, strip0,
    strips_x, n_strips);
}

}  // namespace kh
