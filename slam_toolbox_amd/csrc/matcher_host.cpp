// Host side of the karto correlative scan matcher on MI355X: everything the reference does with
// libm or in inherently sequential order is done here, in the reference's exact IEEE operation
// order (compiled -ffp-contract=off); everything data-parallel is launched on the GPU
// (matcher_kernels.hip).  There is no CPU scoring path.
//
// Reference: lib/karto_sdk/src/Mapper.cpp:477-1208 (ScanMatcher), Mapper.h:1074-1314
// (CorrelationGrid), Karto.h:4393-4563 (CoordinateConverter), :6603-6963 (GridIndexLookup),
// :2946-3041 (Transform), Math.h.
#include "matcher_private.hpp"
#include "matcher_seq.hpp"

namespace kh
{
thread_local std::string g_last_error;
void set_error(const std::string & s) {g_last_error = s;}
}  // namespace kh


namespace kh
{

static int32_t half_kernel_size(double smear, double resolution)   // Mapper.h:1275-1280
{
  return static_cast<int32_t>(round_half_away(2.0 * smear / resolution));
}


// ---- host worker pool: host_pool.hpp ----
void host_parallel_for(size_t n, const std::function<void(size_t)> & fn) {HostPool::instance().run(n, fn);}
void host_parallel_for_wide(size_t n, const std::function<void(size_t)> & fn) {HostPool::wide().run(n, fn);}
void scan_points_at(const double * ranges, size_t ranges_stride, int32_t n_beams, double min_angle, double angular_resolution, size_t n_poses,
  const double * sensor_poses, double * points, double * sensor_xy)
{
  const size_t nb = static_cast<size_t>(n_beams);
  host_parallel_for_wide(n_poses, [&](size_t k) {
    kh_scan_points(ranges + ranges_stride * k, n_beams, sensor_poses + 3 * k, min_angle, angular_resolution, points + 2 * nb * k);
    if (sensor_xy) {sensor_xy[2 * k] = sensor_poses[3 * k]; sensor_xy[2 * k + 1] = sensor_poses[3 * k + 1];}
  });
}

// the geometry and scratch pointers of one slot's rasterisation job (the scan list and the order-dependent rule's tables are the
// caller's)
void fill_raster_job(const kh_matcher * m, const Slot & s, const double * pose, int32_t n_points, size_t npad, RasterJob & j)
{
  std::memset(&j, 0, sizeof(j));
  j.grid = s.d_grid;
  j.view_x = pose[0]; j.view_y = pose[1];
  j.active = s.d_ractive; j.n_points = n_points;
  j.ws = m->ws; j.roi_x = m->roi_x; j.roi_y = m->roi_y; j.roi_w = m->roi_w; j.roi_h = m->roi_h;
  j.kernel_size = m->kernel_size; j.off_x = s.off_x; j.off_y = s.off_y; j.scale = m->scale;
  j.blockmap = s.d_blockmap; j.bm_w = m->bm_w; j.bm_h = m->bm_h; j.bshift = m->bshift;
  const size_t nt = static_cast<size_t>(m->rt_w) * m->rt_h;
  j.tiles_w = m->rt_w; j.tiles_h = m->rt_h; j.height = m->data_size / m->ws;
  j.tile_count = s.d_rtiles; j.tile_cursor = s.d_rtiles + nt; j.n_work = s.d_rtiles + 2 * nt;
  j.tile_start = s.d_rtiles + 2 * nt + 4; j.work = s.d_rtiles + 3 * nt + 4;
  j.cell_xy = s.d_rlists; j.list = s.d_rlists + 2 * npad; j.rank = s.d_rlists + 6 * npad;
  j.grid2 = s.d_grid2; j.copy_kind = s.copy_kind; j.prev_work = s.d_prev_work;
  j.pitch2 = s.copy_kind == 2 ? m->pitch_d : m->pitch2; j.copy_b = s.copy_kind == 2 ? m->copy_q : m->copy_b;
  j.n_foot = static_cast<int32_t>(m->footprint100.size()) - 1;
  int32_t f = 0;
  for (const Cell & c : m->footprint100) {
    if (c.x == 0 && c.y == 0) {continue;}
    j.foot_dx[f] = c.x; j.foot_dy[f] = c.y; ++f;
  }
}

constexpr int kNoFirstPointTable = -1000;      // internal: ensure_seq_tables could not allocate a slot's first-point table
int ensure_seq_tables(kh_matcher * m, Slot & s, int32_t n_points, RasterJob & j)
{
  hipStream_t st = m->stream;
  int rc = ensure_device(s.d_cand, s.cap_cand, static_cast<size_t>(std::max(n_points, 1)) * 8, st); if (rc) {return rc;}
  if (!s.d_seqctl) {KH_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_seqctl), sizeof(int32_t) * 16));}
  const bool fused_tiles = m->kernel_size >= 8;
  if (fused_tiles) {
    rc = ensure_device(s.d_work2, s.cap_work2, 4 * static_cast<size_t>(m->rt_w) * m->rt_h, st); if (rc) {return rc;}
    if (!m->d_tab) {
      std::vector<uint8_t> tab(seq_tile_table_bytes());
      seq_tile_table(m->kernel.data(), m->kernel_size, tab.data());
      KH_HIP(hipMalloc(reinterpret_cast<void **>(&m->d_tab), tab.size()));
      KH_HIP(hipMemcpy(m->d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    }
  }
  const size_t roi_cells = static_cast<size_t>(m->roi_w) * m->roi_h;
  if (roi_cells > s.cap_first) {
    if (s.d_first) {KH_HIP(hipStreamSynchronize(st)); KH_HIP(hipFree(s.d_first)); s.d_first = nullptr;}
    // (the tables were budgeted at create, 4 B x cells of the region of interest per slot, but are allocated here: when the device
    // cannot give one -- other handles, other tenants -- this handle goes back to the hash-table rasteriser for good)
    if (hipMalloc(reinterpret_cast<void **>(&s.d_first), roi_cells * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      s.d_first = nullptr; s.cap_first = 0;
      m->table_raster = false;
      return kNoFirstPointTable;
    }
    s.cap_first = roi_cells; s.first_clean = false;
  }
  if (!s.first_clean) {
    KH_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s.d_first), INT32_MAX, roi_cells, st));
    s.first_clean = true;
  }
  j.first = s.d_first; j.cand = s.d_cand; j.seq_ctl = s.d_seqctl; j.work2 = fused_tiles ? s.d_work2 : nullptr;
  return KH_OK;
}

TablePlan plan_table_raster(const kh_matcher * m, int64_t most_points, int32_t most_readings, int32_t n_scans)
{
  const int32_t tiles = m->rt_w * m->rt_h, bm_words = m->bm_w * m->bm_h;
  const int32_t n_foot = static_cast<int32_t>(m->footprint100.size()) - 1;
  TablePlan p;
  if (most_readings > kSeqMaxReadings) {p.reason = 3; return p;}
  if (n_scans > kSeqMaxScans || most_points > kSeqMaxPoints || tiles > kSeqMaxTiles) {p.reason = 5; return p;}
  // the occupancy block map goes to global memory when the binning kernel's LDS cannot hold it too
  p.bin_lds = seq_bin_lds_bytes(static_cast<int32_t>(most_points), n_foot, tiles, bm_words);
  p.bm_global = p.bin_lds > 150 * 1024;
  if (p.bm_global) {p.bin_lds = seq_bin_lds_bytes(static_cast<int32_t>(most_points), n_foot, tiles, 0);}
  if (p.bin_lds > 150 * 1024) {p.reason = 6; return p;}
  p.ok = true;
  return p;
}

// AddScan's "cell already occupied -> skip" (Mapper.cpp:1093-1096) is order dependent as soon as the smear kernel writes 100
// off-centre: the slot's cell table for k_cell_first / k_active_set, sized for a job of np points, into the job
static int ensure_cell_table(kh_matcher * m, Slot & s, size_t np, RasterJob & j, int32_t & max_cap)
{
  size_t cap = 1024;
  while (cap < 2 * std::max<size_t>(np, 1)) {cap <<= 1;}
  int rc = ensure_device(s.d_hkeys, s.cap_hkeys, cap, m->stream); if (rc) {return rc;}
  rc = ensure_device(s.d_hvals, s.cap_hvals, cap, m->stream); if (rc) {return rc;}
  rc = ensure_device(s.d_hstate, s.cap_hstate, cap, m->stream); if (rc) {return rc;}
  rc = ensure_device(s.d_hnbr, s.cap_hnbr, cap * kMaxFootprint, m->stream); if (rc) {return rc;}
  j.hcap = static_cast<int32_t>(cap);
  max_cap = std::max(max_cap, j.hcap);
  j.hkeys = s.d_hkeys; j.hvals = s.d_hvals; j.hstate = s.d_hstate; j.hnbr = s.d_hnbr;
  return KH_OK;
}

// the per-point scratch of a slot for a job of np points; returns the padded count the lists are laid out by
static int ensure_point_scratch(kh_matcher * m, Slot & s, size_t np, size_t & npad)
{
  int rc = ensure_device(s.d_ractive, s.cap_ractive, std::max<size_t>(np, 1), m->stream); if (rc) {return rc;}
  npad = (std::max<size_t>(np, 1) + 3) & ~static_cast<size_t>(3);      // the rank quadruples are read as int4
  return ensure_device(s.d_rlists, s.cap_rlists, npad * 10, m->stream);
}

// MatchScan steps 1-4, Mapper.cpp:543-569: the slot's grid is centred on the query's sensor pose
static void center_slot(const kh_matcher * m, Slot & s, const double * pose)
{
  const double res = m->grid_resolution();
  s.off_x = pose[0] - (0.5 * (m->roi_w - 1) * res);
  s.off_y = pose[1] - (0.5 * (m->roi_h - 1) * res);
}

// the stamping of the hash-table route (cell table and active set when the rule is order dependent, binning, tiles) and what every
// rasterisation ends with: the re-pitched copies and the slot's tile list brought in step
static void launch_hash_raster(kh_matcher * m, int32_t n_jobs, int32_t most_points, int32_t max_cap, bool any_copies)
{
  const int32_t n_foot = static_cast<int32_t>(m->footprint100.size()) - 1;
  if (n_foot > 0) {launch_active_set(m->d_rjobs, n_jobs, most_points, max_cap, m->stream);}
  launch_raster(m->d_rjobs, n_jobs, most_points, m->rt_w * m->rt_h, m->d_kernel, m->kernel_size, m->stream);
  launch_repitch(m->d_rjobs, n_jobs, m->rt_w * m->rt_h, m->stream, any_copies);
}

// the rasteriser's time by events, between ev[2] and ev[3] (profiling)
static int account_raster(kh_matcher * m)
{
  if (!m->profiling) {return KH_OK;}
  KH_HIP(hipEventRecord(m->ev[3], m->stream));
  KH_HIP(hipEventSynchronize(m->ev[3]));
  float ms = 0;
  KH_HIP(hipEventElapsedTime(&ms, m->ev[2], m->ev[3]));
  m->raster_ms += ms; m->raster_launches += 1;
  return KH_OK;
}

// ---- rasterisation of n jobs from a map view (slots[i] <- the occupied cells of the map in reach of job i) ----

// Map columns (rows) [lo, lo + cnt) whose world coordinate can round into grid cells [0, roi_n) of a grid whose cell 0 lies at `off`:
// WorldToGrid keeps x iff -0.5 <= (x - off) * gscale < roi_n - 0.5.  One cell wide of that either side (the arithmetic here is not
// the kernel's: roi_cell stays the judge); a pose or anchor that is not finite keeps the whole axis.
static void clip_axis(double off, int32_t roi_n, double gscale, double anchor, double mscale, int32_t o, int32_t n, int32_t & lo, int32_t & cnt)
{
  const double w_lo = off - 0.5 / gscale, w_hi = off + (roi_n - 0.5) / gscale;
  double c_lo = std::floor((w_lo - anchor) * mscale) - 1.0 - o, c_hi = std::ceil((w_hi - anchor) * mscale) + 1.0 - o;
  if (!std::isfinite(c_lo) || !std::isfinite(c_hi)) {c_lo = 0.0; c_hi = n - 1.0;}
  c_lo = std::max(c_lo, 0.0); c_hi = std::min(c_hi, n - 1.0);
  if (c_hi < c_lo) {lo = 0; cnt = 0; return;}
  lo = static_cast<int32_t>(c_lo); cnt = static_cast<int32_t>(c_hi - c_lo) + 1;
}

static int raster_map_batch(kh_matcher * m, const std::vector<RasterReq> & reqs)
{
  const size_t n_jobs = reqs.size();
  const int32_t nj = static_cast<int32_t>(n_jobs);
  for (const RasterReq & r : reqs) {
    if (!r.map) {set_error("a batch rasterises from base scans or from a map, not both"); return KH_ERR_INVALID_ARG;}
  }
  int rc = ensure_pinned(m->h_mapjobs, m->cap_hmapjobs, n_jobs, m->stream); if (rc) {return rc;}
  rc = ensure_device(m->d_mapjobs, m->cap_dmapjobs, n_jobs, m->stream); if (rc) {return rc;}
  rc = ensure_pinned(m->h_maptotal, m->cap_hmaptotal, n_jobs, m->stream); if (rc) {return rc;}
  rc = ensure_device(m->d_maptotal, m->cap_dmaptotal, n_jobs, m->stream); if (rc) {return rc;}
  // the pinned mirrors are reused by every call: the previous call's uploads must have left them
  KH_HIP(hipStreamSynchronize(m->stream));
  // 1. the jobs' clip rectangles and units
  size_t units = 0;
  int32_t max_units = 0;
  std::vector<size_t> unit_at(n_jobs);
  for (size_t r = 0; r < n_jobs; ++r) {
    const kh_map_view & v = *reqs[r].map;
    Slot & s = m->slots[reqs[r].slot];
    center_slot(m, s, reqs[r].query->sensor_pose);
    MapJob & j = m->h_mapjobs[r];
    std::memset(&j, 0, sizeof(j));
    j.cells = v.device_cells; j.width_step = v.width_step; j.ox = v.ox; j.oy = v.oy;
    j.ax = v.anchor[0]; j.ay = v.anchor[1]; j.map_scale = v.scale;
    j.off_x = s.off_x; j.off_y = s.off_y; j.scale = m->scale; j.roi_w = m->roi_w; j.roi_h = m->roi_h;
    clip_axis(s.off_x, m->roi_w, m->scale, v.anchor[0], v.scale, v.ox, v.width, j.i0, j.cw);
    clip_axis(s.off_y, m->roi_h, m->scale, v.anchor[1], v.scale, v.oy, v.height, j.j0, j.ch);
    if (j.cw == 0 || j.ch == 0) {j.cw = 0; j.ch = 0;}
    j.units_per_row = (j.cw + 63) / 64;
    j.n_units = j.units_per_row * j.ch;        // (< 2^31 / 64 + height: the view's size was checked)
    unit_at[r] = units;
    units += static_cast<size_t>(j.n_units) + 1;
    max_units = std::max(max_units, j.n_units);
  }
  rc = ensure_device(m->d_mapunits, m->cap_mapunits, units, m->stream); if (rc) {return rc;}
  for (size_t r = 0; r < n_jobs; ++r) {m->h_mapjobs[r].unit = m->d_mapunits + unit_at[r]; m->h_mapjobs[r].total = m->d_maptotal + r;}
  if (m->profiling && !m->ev_map[0]) {
    for (auto & ev : m->ev_map) {KH_HIP(hipEventCreate(&ev));}
  }
  if (m->profiling) {KH_HIP(hipEventRecord(m->ev[2], m->stream));}
  // 2. count and scan; the totals come back once per batch
  KH_HIP(hipMemcpyAsync(m->d_mapjobs, m->h_mapjobs, sizeof(MapJob) * n_jobs, hipMemcpyHostToDevice, m->stream));
  if (m->profiling) {KH_HIP(hipEventRecord(m->ev_map[0], m->stream));}
  launch_map_count(m->d_mapjobs, nj, max_units, m->stream);
  if (m->profiling) {KH_HIP(hipEventRecord(m->ev_map[1], m->stream));}
  KH_HIP(hipMemcpyAsync(m->h_maptotal, m->d_maptotal, sizeof(int32_t) * n_jobs, hipMemcpyDeviceToHost, m->stream));
  KH_HIP(hipStreamSynchronize(m->stream));
  // 3. the per-point scratch from the totals; the job's one pseudo-scan = the collected points, all of them active
  const size_t meta_words = 4 * n_jobs;              // per job: the scan pointer (two words), the prefix {0, n}
  rc = ensure_pinned(m->h_meta, m->cap_hmeta, meta_words, m->stream); if (rc) {return rc;}
  rc = ensure_device(m->d_meta, m->cap_dmeta, meta_words, m->stream); if (rc) {return rc;}
  const int32_t n_foot = static_cast<int32_t>(m->footprint100.size()) - 1;
  int32_t most_points = 0, max_cap = 0;
  bool any_copies = false;
  for (size_t r = 0; r < n_jobs; ++r) {
    Slot & s = m->slots[reqs[r].slot];
    const int32_t total = m->h_maptotal[r];
    if (total < 0 || total > (1 << 30)) {set_error("too many occupied map cells in reach of one match"); return KH_ERR_INVALID_ARG;}
    const size_t np = static_cast<size_t>(total);
    most_points = std::max(most_points, total);
    size_t npad = 0;
    rc = ensure_point_scratch(m, s, np, npad); if (rc) {return rc;}
    rc = ensure_device(s.d_mappts, s.cap_mappts, 2 * std::max<size_t>(np, 1), m->stream); if (rc) {return rc;}
    m->h_mapjobs[r].points = s.d_mappts; m->h_mapjobs[r].active = s.d_ractive;
    int32_t * meta = m->h_meta + 4 * r;
    const double * pts = s.d_mappts;
    std::memcpy(meta, &pts, sizeof(pts));
    meta[2] = 0; meta[3] = total;
    RasterJob & j = m->h_rjobs[r];
    fill_raster_job(m, s, reqs[r].query->sensor_pose, total, npad, j);
    j.scan_ptr = reinterpret_cast<const double * const *>(m->d_meta + 4 * r); j.scan_prefix = m->d_meta + 4 * r + 2;
    j.n_scans = 1; j.uniform_n = total;
    any_copies = any_copies || s.d_grid2 != nullptr;
    if (n_foot > 0) {rc = ensure_cell_table(m, s, np, j, max_cap); if (rc) {return rc;}}
  }
  KH_HIP(hipMemcpyAsync(m->d_meta, m->h_meta, sizeof(int32_t) * meta_words, hipMemcpyHostToDevice, m->stream));
  KH_HIP(hipMemcpyAsync(m->d_rjobs, m->h_rjobs, sizeof(RasterJob) * n_jobs, hipMemcpyHostToDevice, m->stream));
  KH_HIP(hipMemcpyAsync(m->d_mapjobs, m->h_mapjobs, sizeof(MapJob) * n_jobs, hipMemcpyHostToDevice, m->stream));
  // 4. Grid::Clear, the fill phase, and the stamping of the hash-table route as for base scans (k_find_valid* is the one stage
  // a map job has no use for).  The first-point tables of the slots are not touched: they stay as clean as they were.
  launch_raster_clear(m->d_rjobs, nj, m->stream);
  if (m->profiling) {KH_HIP(hipEventRecord(m->ev_map[2], m->stream));}
  launch_map_fill(m->d_mapjobs, nj, max_units, m->stream);
  if (m->profiling) {KH_HIP(hipEventRecord(m->ev_map[3], m->stream));}
  launch_hash_raster(m, nj, most_points, max_cap, any_copies);
  KH_HIP(hipGetLastError());
  rc = account_raster(m); if (rc) {return rc;}
  if (m->profiling) {
    float a = 0, b = 0;
    KH_HIP(hipEventElapsedTime(&a, m->ev_map[0], m->ev_map[1]));
    KH_HIP(hipEventElapsedTime(&b, m->ev_map[2], m->ev_map[3]));
    m->map_collect_ms += a + b; m->map_collects += 1;
  }
  return KH_OK;
}

// ---- rasterisation of n jobs (slots[i] <- base scans of job i) ------------------------------

int raster_batch(kh_matcher * m, const std::vector<RasterReq> & reqs)
{
  if (reqs.empty()) {return KH_OK;}
  if (reqs[0].map) {return raster_map_batch(m, reqs);}
  const size_t n_jobs = reqs.size();
  static const bool timing = std::getenv("KH_MATCH_TIMING") != nullptr;
  const auto t_enter = std::chrono::steady_clock::now();
  // 1. The base scans' unfiltered point readings go to the device ONCE per distinct scan of the batch (loop-closure
  // chains overlap heavily: 256 pairs name ~6400 scans, ~1600 of them distinct); FindValidPoints, WorldToGrid and the
  // order-dependent "cell already occupied" rule all run on the GPU (K0 / K1).  The host only lists who reads what.
  struct Copy {const double * src; size_t dst; int32_t n;};
  std::vector<Copy> copies;
  std::unordered_map<const double *, int32_t> arena_of;        // points_xy -> first point in the arena
  arena_of.reserve(256);
  size_t arena_points = 0, meta_words = 0, n_items = 0;
  std::vector<size_t> meta_at(n_jobs), scans_of(n_jobs, 0);
  std::vector<int32_t> points_of(n_jobs, 0);
  int32_t most_points = 0, most_readings = 0, max_scan_n = 1;
  for (size_t r = 0; r < n_jobs; ++r) {
    int64_t pts = 0;
    for (int32_t b = 0; b < reqs[r].n_base; ++b) {
      const kh_scan & sc = reqs[r].base[b];
      most_readings = std::max(most_readings, sc.n);
      if (sc.points_xy == nullptr || sc.n <= 0) {continue;}      // NULL scan: skipped (Mapper.cpp:1039-1041)
      ++scans_of[r]; pts += sc.n;
      max_scan_n = std::max(max_scan_n, sc.n);
      if (sc.device_points_xy) {continue;}                        // resident on the device: nothing to upload
      auto it = arena_of.find(sc.points_xy);
      if (it == arena_of.end()) {
        arena_of.emplace(sc.points_xy, static_cast<int32_t>(arena_points));
        copies.push_back(Copy{sc.points_xy, arena_points, sc.n});
        arena_points += static_cast<size_t>(sc.n);
      }
    }
    if (pts > (1 << 30) || arena_points > (1u << 30)) {set_error("too many base scan points in one batch"); return KH_ERR_INVALID_ARG;}
    points_of[r] = static_cast<int32_t>(pts);
    most_points = std::max(most_points, points_of[r]);
    meta_at[r] = meta_words;
    meta_words += 3 * scans_of[r] + 1 + ((scans_of[r] + 1) & 1);      // 64-bit scan pointers, then the prefix (kept 8-byte aligned)
    n_items += scans_of[r];
  }
  const size_t items_at = meta_words;
  // The first-point rasteriser (matcher_seq.hip) for the whole batch: no hash tables, the order-dependent rule and the binning of
  // a job in ONE workgroup with its state in LDS.  Needs every job inside its fixed-size tables.
  const TablePlan plan = plan_table_raster(m, most_points, most_readings, 0);
  bool use_table = m->table_raster && plan.ok;
  meta_words += 2 * n_items;
  int rc = ensure_pinned(m->h_arena, m->cap_harena, std::max<size_t>(arena_points, 1) * 2, m->stream); if (rc) {return rc;}
  rc = ensure_device(m->d_arena, m->cap_darena, std::max<size_t>(arena_points, 1) * 2, m->stream); if (rc) {return rc;}
  rc = ensure_pinned(m->h_meta, m->cap_hmeta, std::max<size_t>(meta_words, 1), m->stream); if (rc) {return rc;}
  rc = ensure_device(m->d_meta, m->cap_dmeta, std::max<size_t>(meta_words, 1), m->stream); if (rc) {return rc;}
  // the pinned mirrors are reused by every call: the previous call's uploads must have left them
  KH_HIP(hipStreamSynchronize(m->stream));
  const int32_t n_foot = static_cast<int32_t>(m->footprint100.size()) - 1;
  int32_t max_cap = 0;
  bool any_copies = false;
  ValidItem * items = reinterpret_cast<ValidItem *>(m->h_meta + items_at);
  // the jobs, their scan lists and the (job, scan) items; `table`: the first-point rasteriser's tables instead of the hash tables
  auto fill_jobs = [&](bool table) -> int {
    size_t item = 0;
    for (size_t r = 0; r < n_jobs; ++r) {
      Slot & s = m->slots[reqs[r].slot];
      const double * pose = reqs[r].query->sensor_pose;
      center_slot(m, s, pose);
      const double ** scan_ptr = reinterpret_cast<const double **>(m->h_meta + meta_at[r]);
      int32_t * scan_prefix = m->h_meta + meta_at[r] + 2 * scans_of[r];
      int32_t k = 0, run = 0, uniform_n = -1;
      for (int32_t b = 0; b < reqs[r].n_base; ++b) {
        const kh_scan & sc = reqs[r].base[b];
        if (sc.points_xy == nullptr || sc.n <= 0) {continue;}
        uniform_n = uniform_n < 0 ? sc.n : (uniform_n == sc.n ? uniform_n : 0);
        scan_ptr[k] = sc.device_points_xy ? sc.device_points_xy : m->d_arena + 2 * static_cast<size_t>(arena_of.at(sc.points_xy));
        scan_prefix[k] = run;
        run += sc.n;
        items[item].job = static_cast<int32_t>(r); items[item].scan = k; ++item;
        ++k;
      }
      scan_prefix[k] = run;
      const size_t np = static_cast<size_t>(points_of[r]);
      size_t npad = 0;
      int rc = ensure_point_scratch(m, s, np, npad); if (rc) {return rc;}
      RasterJob & j = m->h_rjobs[r];
      fill_raster_job(m, s, pose, points_of[r], npad, j);
      j.scan_ptr = reinterpret_cast<const double * const *>(m->d_meta + meta_at[r]); j.scan_prefix = m->d_meta + meta_at[r] + 2 * scans_of[r];
      j.n_scans = static_cast<int32_t>(scans_of[r]);
      j.uniform_n = std::max(uniform_n, 0);
      any_copies = any_copies || s.d_grid2 != nullptr;
      if (table) {
        rc = ensure_seq_tables(m, s, points_of[r], j); if (rc) {return rc;}
        s.first_clean = false;                      // until this batch's stamping launch has handed the table back
      } else if (n_foot > 0) {
        rc = ensure_cell_table(m, s, np, j, max_cap); if (rc) {return rc;}
      }
    }
    return KH_OK;
  };
  rc = fill_jobs(use_table);
  // a slot's table could not be allocated: m->table_raster is off for good, and the jobs are filled again for the hash tables
  if (rc == kNoFirstPointTable) {use_table = false; rc = fill_jobs(false);}
  if (rc) {return rc;}
  // 2. upload the jobs and scan lists; Grid::Clear (Karto.h:4612-4615) -- up to 16.8 MB per job -- needs nothing else and
  // runs while the pool gathers the distinct scans' points into the pinned arena
  if (meta_words) {
    KH_HIP(hipMemcpyAsync(m->d_meta, m->h_meta, sizeof(int32_t) * meta_words, hipMemcpyHostToDevice, m->stream));
  }
  KH_HIP(hipMemcpyAsync(m->d_rjobs, m->h_rjobs, sizeof(RasterJob) * n_jobs, hipMemcpyHostToDevice, m->stream));
  if (m->profiling) {KH_HIP(hipEventRecord(m->ev[2], m->stream));}
  if (!use_table) {launch_raster_clear(m->d_rjobs, static_cast<int32_t>(n_jobs), m->stream);}
  HostPool::instance().run(copies.size(), [&](size_t i) {
    std::memcpy(m->h_arena + 2 * copies[i].dst, copies[i].src, sizeof(double) * 2 * static_cast<size_t>(copies[i].n));
  });
  if (arena_points) {
    KH_HIP(hipMemcpyAsync(m->d_arena, m->h_arena, sizeof(double) * 2 * arena_points, hipMemcpyHostToDevice, m->stream));
  }
  // 3. FindValidPoints, stamps
  if (use_table) {
    const int32_t nj = static_cast<int32_t>(n_jobs), tiles = m->rt_w * m->rt_h;
    launch_seq_prep_batch(m->d_rjobs, nj, reinterpret_cast<const ValidItem *>(m->d_meta + items_at), static_cast<int32_t>(n_items), max_scan_n, m->stream);
    launch_seq_links(m->d_rjobs, nj, most_points, m->stream);
    launch_seq_bin(m->d_rjobs, nj, plan.bin_lds, plan.bm_global ? 1 : 0, nullptr, m->stream);
    if (m->kernel_size >= 8) {
      launch_seq_tile(m->d_rjobs, nj, m->d_tab, most_points, tiles, nullptr, m->stream);
    } else {
      launch_raster_tiles(m->d_rjobs, nj, most_points, tiles, m->d_kernel, m->kernel_size, m->stream);
      launch_seq_stage(m->d_rjobs, nj, nullptr, m->stream);
    }
    for (size_t r = 0; r < n_jobs; ++r) {m->slots[reqs[r].slot].first_clean = true;}
    launch_repitch(m->d_rjobs, static_cast<int32_t>(n_jobs), m->rt_w * m->rt_h, m->stream, any_copies);
  } else {
    launch_find_valid(m->d_rjobs, reinterpret_cast<const ValidItem *>(m->d_meta + items_at), static_cast<int32_t>(n_items), max_scan_n, m->stream);
    launch_hash_raster(m, static_cast<int32_t>(n_jobs), most_points, max_cap, any_copies);
  }
  KH_HIP(hipGetLastError());
  if (timing) {
    std::fprintf(stderr, "[kh raster] host %.3f ms: %zu jobs, %zu (job, scan) items, %zu distinct scans, %.1f MB of points uploaded\n",
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enter).count(), n_jobs, n_items, copies.size(),
      arena_points * 16.0 / 1e6);
  }
  return account_raster(m);
}

// ---- CorrelateScan on a set of slots ---------------------------------------------------------

// Re-pitched copies of a slot's grid (CorrJob::grid2): allocated zeroed, filled from the grid as it stands, kept in step by
// raster_batch from then on.
static int allocate_copies(kh_matcher * m, Slot & s, int32_t kind)
{
  const size_t rows = static_cast<size_t>(m->data_size / m->ws);
  const size_t bytes = (kind == 2 ? static_cast<size_t>(m->copy_q) * 4 + 64 : static_cast<size_t>(m->copy_b) * 2 + 64) + 2 * kGridPad;
  s.copy_kind = kind;
  KH_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_grid2_alloc), bytes));
  KH_HIP(hipMemsetAsync(s.d_grid2_alloc, 0, bytes, m->stream));
  s.d_grid2 = s.d_grid2_alloc + kGridPad + static_cast<size_t>(m->pad_rows) * (kind == 2 ? m->pitch_d : m->pitch2);
  const size_t nt = static_cast<size_t>(m->rt_w) * m->rt_h;
  // one-job descriptor for the full copy: only the fields k_repitch_full / k_repitch_keep read
  RasterJob j;
  std::memset(&j, 0, sizeof(j));
  j.grid = s.d_grid; j.ws = m->ws; j.height = static_cast<int32_t>(rows);
  j.grid2 = s.d_grid2; j.copy_kind = kind; j.prev_work = s.d_prev_work;
  j.pitch2 = kind == 2 ? m->pitch_d : m->pitch2; j.copy_b = kind == 2 ? m->copy_q : m->copy_b;
  const size_t nt2 = nt;
  j.n_work = s.d_rtiles + 2 * nt2; j.work = s.d_rtiles + 3 * nt2 + 4;
  RasterJob * d_j = nullptr;
  KH_HIP(hipMalloc(reinterpret_cast<void **>(&d_j), sizeof(RasterJob)));
  KH_HIP(hipMemcpyAsync(d_j, &j, sizeof(RasterJob), hipMemcpyHostToDevice, m->stream));
  launch_repitch_full(d_j, static_cast<int32_t>(rows), m->stream);
  KH_HIP(hipStreamSynchronize(m->stream));       // `j` is on this stack, and the side streams may read the copies next
  KH_HIP(hipFree(d_j));
  return KH_OK;
}

// (the distance penalties -- nx * ny doubles, 30 KB of a config-2 search's 51, 52 KB of a loop-closure search's 70 -- are staged
// by the fused path of one match only, and only for a search that penalises: batches read them from the handle's SearchTable)
StageLayout stage_layout(int32_t P, int32_t nx, int32_t ny, int32_t na, bool stage_penalties)
{
  StageLayout L;
  size_t o = align_up(sizeof(CorrJob), 256);
  L.bx = o; o = align_up(o + sizeof(int32_t) * nx, 16);
  L.by = o; o = align_up(o + sizeof(int32_t) * ny, 16);
  L.dist_pen = o; L.dist_pen_bytes = stage_penalties ? sizeof(double) * nx * ny : 0; o = align_up(o + L.dist_pen_bytes, 16);
  L.ang_pen = o; o = align_up(o + sizeof(double) * na, 16);
  L.cos_sin = o; o = align_up(o + sizeof(double) * 2 * na, 16);
  L.local = o; o = align_up(o + sizeof(double) * 2 * P, 16);
  L.invalid = o; o = align_up(o + P, 16);
  L.total = align_up(o, 256);
  return L;
}

// rows per lane of the scoring kernel (a tile is 4 * ry lattice rows): the variant that loads the fewest rows for ny --
// 81 rows are 3 tiles of 28 (ry 7: 21 row loads per beam and column of tiles) rather than 3 tiles of 32 (ry 8: 24)
int pick_ry(int32_t ny)
{
  if (ny <= 4) {return 1;}
  int best = 8, best_cost = 1 << 30;
  for (int ry : {8, 7, 4}) {
    const int cost = ((ny + 4 * ry - 1) / (4 * ry)) * ry;
    if (cost < best_cost) {best = ry; best_cost = cost;}
  }
  return best;
}

// the accumulation of ComputeAngularCovariance (Mapper.cpp:992-1024) over the raw responses of all angles at the best cell
static double angular_variance(const std::vector<int32_t> & sums, double denom, double center_heading, double ang_off,
  double ang_res, double best_angle, double best_response)
{
  const double startAngle = center_heading - ang_off;
  double norm = 0.0, acc = 0.0;
  for (size_t a = 0; a < sums.size(); ++a) {
    const double angle = startAngle + static_cast<uint32_t>(a) * ang_res;
    const double response = static_cast<double>(sums[a]) / denom;     // GetResponse: no penalty
    if (response >= (best_response - 0.1)) {
      norm += response;
      acc += ((angle - best_angle) * (angle - best_angle) * response);
    }
  }
  if (norm > kTolerance) {
    if (acc < kTolerance) {acc = ang_res * ang_res;}
    acc /= norm;
  } else {
    acc = 1000 * (ang_res * ang_res);
  }
  return acc;
}

static inline double host_response(const CorrHost & c, int32_t sum, int a, int yi, int xi)
{
  double response = static_cast<double>(sum) / c.denom;
  if (c.penalize && !double_equal(response, 0.0)) {
    response *= (c.geo->dist_pen[static_cast<size_t>(yi) * c.nx + xi] * c.ang_pen[a]);
  }
  return response;
}

CorrReq coarse_search(const kh_matcher * m, int32_t slot, const kh_scan * query, double ang_off, bool penalize)
{
  const double res = m->grid_resolution();
  const double cso = 0.5 * (static_cast<double>(m->side) - 1) * res, csr = 2 * res;      // Mapper.cpp:577-585
  const double offset[2] = {cso, cso}, resolution[2] = {csr, csr};
  return CorrReq(slot, query, query->sensor_pose, offset, resolution, ang_off, m->params.coarse_angle_resolution, penalize, false);
}

CorrReq fine_search(const kh_matcher * m, int32_t slot, const kh_scan * query, const double * center, bool penalize)
{
  const double res = m->grid_resolution(), csr = 2 * res;
  const double offset[2] = {csr * 0.5, csr * 0.5}, resolution[2] = {res, res};      // Mapper.cpp:622-624
  return CorrReq(slot, query, center, offset, resolution, 0.5 * m->params.coarse_angle_resolution, m->params.fine_search_angle_offset,
    penalize, true);
}

// the search lattice of one request (Mapper.cpp:736-756)
int init_ctx(const CorrReq & q, CorrHost & c)
{
  c.slot = q.slot;
  c.P = q.scan->n;
  std::copy(q.center, q.center + 3, c.center);
  c.off_x = q.off_x; c.off_y = q.off_y; c.res_x = q.res_x; c.res_y = q.res_y;
  c.ang_off = q.ang_off; c.ang_res = q.ang_res; c.fine = q.fine; c.penalize = q.penalize;
  c.nx = static_cast<int32_t>(static_cast<uint32_t>(round_half_away(q.off_x * 2.0 / q.res_x) + 1));
  c.ny = static_cast<int32_t>(static_cast<uint32_t>(round_half_away(q.off_y * 2.0 / q.res_y) + 1));
  c.na = static_cast<int32_t>(static_cast<uint32_t>(round_half_away(q.ang_off * 2.0 / q.ang_res) + 1));
  if (c.nx <= 0 || c.ny <= 0 || c.na <= 0 || static_cast<int64_t>(c.nx) * c.ny * c.na > (1ll << 28)) {
    set_error("search volume out of range");
    return KH_ERR_INVALID_ARG;
  }
  c.denom = static_cast<double>(static_cast<uint32_t>(c.P) * 100u);     // Mapper.cpp:1204
  return KH_OK;
}

int attach_table(kh_matcher * m, const CorrReq & q, CorrHost & c, bool on_device)
{
  const kh_match_params & mp = m->params;
  uint64_t key[8] = {static_cast<uint64_t>(static_cast<uint32_t>(c.nx)), static_cast<uint64_t>(static_cast<uint32_t>(c.ny)), 0, 0, 0, 0, 0, 0};
  const double reals[6] = {q.off_x, q.off_y, q.res_x, q.res_y, mp.distance_variance_penalty, mp.minimum_distance_penalty};
  std::memcpy(key + 2, reals, sizeof(reals));
  std::shared_ptr<SearchTable> t;
  for (const auto & have : m->tables) {
    if (std::memcmp(have->key, key, sizeof(key)) == 0) {t = have; break;}
  }
  if (!t) {
    t = std::make_shared<SearchTable>();
    std::memcpy(t->key, key, sizeof(key));
    t->nx = c.nx; t->ny = c.ny;
    const double startX = -q.off_x, startY = -q.off_y;
    t->x_poses.resize(c.nx); t->y_poses.resize(c.ny);
    for (int32_t k = 0; k < c.nx; ++k) {t->x_poses[k] = startX + static_cast<uint32_t>(k) * q.res_x;}
    for (int32_t k = 0; k < c.ny; ++k) {t->y_poses[k] = startY + static_cast<uint32_t>(k) * q.res_y;}
    // penalties, Mapper.cpp:673-677
    t->dist_pen.resize(static_cast<size_t>(c.nx) * c.ny);
    for (int32_t yi = 0; yi < c.ny; ++yi) {
      for (int32_t xi = 0; xi < c.nx; ++xi) {
        t->dist_pen[static_cast<size_t>(yi) * c.nx + xi] = distance_penalty(mp, t->x_poses[xi], t->y_poses[yi]);
      }
    }
    m->tables.push_back(t);
  }
  if (on_device && !t->d_dist_pen) {
    const size_t bytes = t->dist_pen.size() * sizeof(double);
    double * d = nullptr;
    KH_HIP(hipMalloc(reinterpret_cast<void **>(&d), bytes));
    // blocking: the table is on the device before any stream of the handle is given a job that reads it
    if (hipMemcpy(d, t->dist_pen.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      set_error("upload of a distance-penalty table failed");
      return KH_ERR_HIP;
    }
    t->d_dist_pen = d;
  }
  t->used = ++m->table_clock;
  c.geo = t;
  return KH_OK;
}

void trim_tables(kh_matcher * m)
{
  while (m->tables.size() > kMaxTables) {
    auto oldest = std::min_element(m->tables.begin(), m->tables.end(),
        [](const std::shared_ptr<SearchTable> & a, const std::shared_ptr<SearchTable> & b) {return a->used < b->used;});
    // (a slot's introspection state may keep the entry's host half alive; the device copy goes now)
    if ((*oldest)->d_dist_pen) {(void)hipFree((*oldest)->d_dist_pen); (*oldest)->d_dist_pen = nullptr;}
    m->tables.erase(oldest);
  }
}

// device scratch of one slot for the search `c` describes (allocation is serial: called before the pool fills the tables)
int ensure_slot_scratch(kh_matcher * m, const CorrReq & q, CorrHost & c, bool allow_copies)
{
  int rc = KH_OK;
  Slot & s = m->slots[c.slot];
  // device scratch for this slot
  const size_t tp = static_cast<size_t>(c.na) * c.P;
  if (tp > s.cap_table) {
    if (s.d_table) {KH_HIP(hipStreamSynchronize(m->stream)); KH_HIP(hipFree(s.d_table)); KH_HIP(hipFree(s.d_slow));}
    const size_t cap = std::max(tp, s.cap_table + s.cap_table / 2);
    KH_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_table), cap * 4));
    KH_HIP(hipMalloc(reinterpret_cast<void **>(&s.d_slow), cap * 4));
    s.cap_table = cap;
  }
  rc = ensure_device(s.d_counts, s.cap_counts, static_cast<size_t>(c.na) * kCountsPerAngle, m->stream); if (rc) {return rc;}
  {
    // one compacted list per (angle, alignment class, scoring tile): bound of the tile count, the job's real
    // one (<= it) is set with the rest of the job below
    size_t lt = static_cast<size_t>((c.nx + 30) / 31) * ((c.ny + 4 * pick_ry(c.ny) - 1) / (4 * pick_ry(c.ny)));
    if (lt > 32) {lt = 1;}
    c.lt_alloc = static_cast<int32_t>(lt);
    // (twice: the second half holds the lists into the re-pitched copies)
    rc = ensure_device(s.d_fast, s.cap_fast, 2 * tp * kClasses * lt, m->stream); if (rc) {return rc;}
    rc = ensure_device(s.d_tcounts, s.cap_tcounts, 2 * static_cast<size_t>(c.na) * kClasses * lt, m->stream); if (rc) {return rc;}
    // dual-copy layout: worth its memory (2 x the grid) and upkeep for full-resolution searches with many angles whose
    // window is one tile wide -- the config-2 CorrelateScan; decided from the request alone, allocated once per slot
    const double work = static_cast<double>(c.nx) * c.ny * c.na * c.P;
    // (the copy is picked per beam and scoring tile, so the lattice is one tile wide or has per-tile lists)
    const double cells_per_step = q.res_x * m->scale;
    const bool full_res = c.nx > 1 && std::fabs(cells_per_step - 1.0) < 1e-9 && c.nx <= kTileSpan;
    const bool tiled_lists = lt > 1 && (std::fabs(cells_per_step - 1.0) < 1e-9 || std::fabs(cells_per_step - 2.0) < 1e-9);
    if (allow_copies && m->dual_copy && !s.d_grid2 && (full_res || tiled_lists) && work >= 1e8) {
      // a search that steps two cells (MatchScan's coarse pass) gets the column-decimated copies
      const bool two_cells = std::fabs(cells_per_step - 2.0) < 1e-9 && m->copy_q > 0 && (m->ws % 8) == 0;
      rc = allocate_copies(m, s, two_cells ? 2 : 1); if (rc) {return rc;}
    }
  }
  {
    // chunk descriptors of the LDS-staged path: at most one per beam, kept per (angle pair, beam range)
    const size_t groups = (static_cast<size_t>(c.na) + kGroupAngles - 1) / kGroupAngles;
    const size_t range_len = static_cast<size_t>(lds_desc_capacity(c.P));
    rc = ensure_device(s.d_chunks, s.cap_chunks, groups * kLdsRanges * range_len * kChunkWords, m->stream); if (rc) {return rc;}
    rc = ensure_device(s.d_chunk_counts, s.cap_chunk_counts, groups * kLdsRanges, m->stream); if (rc) {return rc;}
  }
  const size_t vol = static_cast<size_t>(c.nx) * c.ny * c.na;
  rc = ensure_device(s.d_sums, s.cap_volume, vol, m->stream); if (rc) {return rc;}
  // best response per scoring tile: at most ceil(nx / 31) x ceil(ny / 4) tiles per angle
  rc = ensure_device(s.d_tile_best, s.cap_tile_best,
      static_cast<size_t>(c.na) * ((c.nx + 30) / 31) * ((c.ny + 3) / 4), m->stream); if (rc) {return rc;}
  if (m->keep_responses) {rc = ensure_device(s.d_resp, s.cap_resp, vol, m->stream); if (rc) {return rc;}}

  return KH_OK;
}

// Host half of one CorrelateScan job: the exact-arithmetic tables into the staging block `hb` (device address `db`) and the job
// descriptor at its head.  Independent between the jobs of a batch (runs on the pool).
void prepare_job(kh_matcher * m, const CorrReq & q, CorrHost & c, const StageLayout & L, uint8_t * hb, uint8_t * db,
  unsigned long long * d_out, size_t out_words, size_t n_launch, bool lds_always, bool lds_never, JobShape & shape)
{
  const kh_match_params & mp = m->params;
  Slot & s = m->slots[c.slot];
  CorrJob * job = reinterpret_cast<CorrJob *>(hb);
  int32_t * bx = reinterpret_cast<int32_t *>(hb + L.bx);
  int32_t * by = reinterpret_cast<int32_t *>(hb + L.by);
  double * ang_pen = reinterpret_cast<double *>(hb + L.ang_pen);
  double * cos_sin = reinterpret_cast<double *>(hb + L.cos_sin);
  double * local = reinterpret_cast<double *>(hb + L.local);
  uint8_t * invalid = hb + L.invalid;

  // lattice base indices: operator()(y), Mapper.cpp:649-662
  c.bx.resize(c.nx); c.by.resize(c.ny);
  for (int32_t k = 0; k < c.nx; ++k) {
    const double newPositionX = c.center[0] + c.geo->x_poses[k];
    const double gx = (newPositionX - s.off_x) * m->scale;
    c.bx[k] = to_int32(round_half_away(gx)) + m->roi_x;
    bx[k] = c.bx[k];
  }
  for (int32_t k = 0; k < c.ny; ++k) {
    const double newPositionY = c.center[1] + c.geo->y_poses[k];
    const double gy = (newPositionY - s.off_y) * m->scale;
    c.by[k] = (to_int32(round_half_away(gy)) + m->roi_y) * m->ws;
    by[k] = c.by[k];
  }
  int32_t sx = c.nx > 1 ? c.bx[1] - c.bx[0] : 1;
  int32_t sy_ws = c.ny > 1 ? c.by[1] - c.by[0] : m->ws;
  bool linear = (sx == 1 || sx == 2) && sy_ws > 0;
  for (int32_t k = 1; k < c.nx && linear; ++k) {linear = (c.bx[k] - c.bx[k - 1]) == sx;}
  for (int32_t k = 1; k < c.ny && linear; ++k) {linear = (c.by[k] - c.by[k - 1]) == sy_ws;}
  // every window row read by a tile must stay inside the (padded) allocation
  if (linear) {
    const int64_t bmax = static_cast<int64_t>(c.bx[0]) + c.by[0] + static_cast<int64_t>(c.ny - 1) * sy_ws;
    if (c.bx[0] + c.by[0] < 0 || bmax >= m->data_size) {linear = false;}
  }
  if (!linear) {sx = 1; sy_ws = m->ws;}

  // penalties, Mapper.cpp:671-685 (the distance penalties are the SearchTable's)
  c.ang_pen.assign(c.na, 1.0);
  c.angles.resize(c.na);
  const double startAngle = c.center[2] - c.ang_off;
  for (int32_t a = 0; a < c.na; ++a) {
    const double angle = startAngle + static_cast<uint32_t>(a) * c.ang_res;
    c.angles[a] = angle;
    ref_sincos(angle, &cos_sin[2 * a + 1], &cos_sin[2 * a]);          // Karto.h:6857-6858
    c.ang_pen[a] = angle_penalty(mp, angle, c.center[2]);
    ang_pen[a] = c.ang_pen[a];
  }
  if (L.dist_pen_bytes) {std::memcpy(hb + L.dist_pen, c.geo->dist_pen.data(), L.dist_pen_bytes);}

  // scan points in the sensor frame: Transform(sensorPose).InverseTransformPose, Karto.h:6813-6824,
  // 2987-2994, 3003-3024, 2482-2511, 2654-2666
  {
    const double tx = q.scan->sensor_pose[0], ty = q.scan->sensor_pose[1], th = q.scan->sensor_pose[2];
    double r00, r01, r02, r10, r11, r12;
    if (tx == 0.0 && ty == 0.0 && th == 0.0) {
      r00 = 1; r01 = 0; r02 = 0; r10 = 0; r11 = 1; r12 = 0;
    } else {
      const double radians = 0.0 - th;
      double cosR, sinR;
      ref_sincos(radians, &sinR, &cosR);
      const double omc = 1.0 - cosR;
      r00 = 0.0 * omc + cosR;
      r01 = 0.0 * 0.0 * omc - 1.0 * sinR;
      r02 = 0.0 * 1.0 * omc + 0.0 * sinR;
      r10 = 0.0 * 0.0 * omc + 1.0 * sinR;
      r11 = 0.0 * omc + cosR;
      r12 = 0.0 * 1.0 * omc - 0.0 * sinR;
    }
    for (int32_t k = 0; k < c.P; ++k) {
      const double sxp = q.scan->points_xy[2 * k] - tx, syp = q.scan->points_xy[2 * k + 1] - ty, sh = 0.0 - th;
      local[2 * k] = r00 * sxp + r01 * syp + r02 * sh;
      local[2 * k + 1] = r10 * sxp + r11 * syp + r12 * sh;
      const double rr = q.scan->ranges[k];
      invalid[k] = (std::isnan(rr) || std::isinf(rr)) ? 1 : 0;     // Karto.h:6869-6875
    }
  }

  std::memset(job, 0, sizeof(CorrJob));
  job->grid = s.d_grid; job->data_size = m->data_size; job->ws = m->ws;
  job->n_points = c.P; job->nx = c.nx; job->ny = c.ny; job->na = c.na;
  job->linear = linear ? 1 : 0; job->sx = sx; job->sy_ws = sy_ws; job->base0 = c.bx[0] + c.by[0];
  const int this_sx = (linear && sx == 2) ? 2 : 1;
  const int this_ry = pick_ry(c.ny);
  job->tiles_y = (c.ny + 4 * this_ry - 1) / (4 * this_ry);
  // column-decimated copies of the slot: the two-cell search is scored as a one-cell search on them (CorrJob::dec), as long
  // as the copy can be picked per beam and tile (one tile column, or lists per tile)
  bool dec = s.copy_kind == 2 && m->dual_copy && this_sx == 2 && sy_ws % m->ws == 0;
  if (dec) {
    const int32_t tiles = ((c.nx + kTileSpan - 1) / kTileSpan) * job->tiles_y;
    dec = c.nx <= kTileSpan || (tiles >= 4 && tiles <= c.lt_alloc);
  }
  const int px = dec ? kTileSpan : score_tile_poses(this_sx);
  job->tiles_x = (c.nx + px - 1) / px;
  job->ry = this_ry; job->tile_px = px; job->dec = dec ? 1 : 0;
  shape.sx = dec ? 1 : this_sx; shape.lds_sx = this_sx; shape.ry = this_ry; shape.tiles = job->tiles_x * job->tiles_y;
  // LDS-staged scoring: linear lattice whose window fits 64 bytes x 64 rows
  // ... and a launch of at least two workgroups (angle pairs) per compute unit: one config-2 search alone is 41 workgroups that
  // walk their 25 chunks one after the other -- 0.26 ms against the windowed kernel's 0.14
  const bool lds_wanted = lds_always || (!lds_never && static_cast<double>(c.nx) * c.ny * c.na * c.P >= 1e8 &&
    static_cast<double>(n_launch) * c.na >= 1024.0);      // (workgroup = kGroupAngles angles)
  const bool lds_ok = lds_wanted && linear && (c.nx - 1) * sx + 1 <= kTileSpan && c.ny <= 64 && c.P <= 2048 &&
    sy_ws % m->ws == 0 && sy_ws / m->ws == sx && (m->ws % 4) == 0 && 63 * sx + 1 <= kLdsRows;
  shape.lds = lds_ok ? 1 : 0;
  job->lds_path = shape.lds; job->sy_cells = sy_ws / m->ws;
  job->rel = s.d_fast; job->chunks = s.d_chunks; job->chunk_counts = s.d_chunk_counts;
  job->do_penalize = q.penalize ? 1 : 0; job->coarse = q.fine ? 0 : 1;
  job->write_resp = m->keep_responses ? 1 : 0;
  job->denom = c.denom;
  job->grid_off_x = s.off_x; job->grid_off_y = s.off_y; job->scale = m->scale;
  job->bx = reinterpret_cast<const int32_t *>(db + L.bx);
  job->by = reinterpret_cast<const int32_t *>(db + L.by);
  job->dist_pen = L.dist_pen_bytes ? reinterpret_cast<const double *>(db + L.dist_pen) : c.geo->d_dist_pen;
  job->ang_pen = reinterpret_cast<const double *>(db + L.ang_pen);
  job->cos_sin = reinterpret_cast<const double *>(db + L.cos_sin);
  job->local = reinterpret_cast<const double *>(db + L.local);
  job->invalid = db + L.invalid;
  job->table = s.d_table; job->fast = s.d_fast; job->slow = s.d_slow; job->counts = s.d_counts;
  job->tcounts = s.d_tcounts; {
    // tile lists pay for themselves when the window is several tiles large (the tests cost K2 time per tile)
    const int32_t tiles = job->tiles_x * job->tiles_y;
    job->list_tiles = (tiles >= 4 && tiles <= c.lt_alloc) ? tiles : 1;
  }
  job->sums = s.d_sums; job->resp = s.d_resp; job->out = d_out; job->out_words = static_cast<int32_t>(out_words);
  job->blockmap = m->dense_score ? nullptr : s.d_blockmap; job->bm_w = m->bm_w; job->bm_h = m->bm_h; job->bshift = m->bshift;
  job->tile_best = s.d_tile_best;
  // re-pitched copies: linear full-resolution lattice one tile wide (the copy is picked per beam for the tile at x0 = 0)
  {
    const bool use2 = dec || (s.copy_kind == 1 && m->dual_copy && linear && (job->tiles_x == 1 || job->list_tiles > 1));
    const size_t lists = static_cast<size_t>(c.na) * kClasses * static_cast<size_t>(c.lt_alloc);
    job->grid2 = use2 ? s.d_grid2 : nullptr;
    job->pitch2 = dec ? m->pitch_d : m->pitch2; job->copy_b = dec ? m->copy_q : m->copy_b;
    job->fast2 = s.d_fast + lists * static_cast<size_t>(c.P);
    job->tcounts2 = s.d_tcounts + lists;
  }
  job->pad = std::max(0, m->pad_rows * m->ws - 512); job->pad_rows = m->pad_rows;
  job->load_counter = m->profiling ? m->d_load_counter : nullptr;
}

// Finalisation of one CorrelateScan (Mapper.cpp:775-862) from its downloaded result block: tie average, covariance, the slot's
// introspection state.  q.status carries the reference's "unable to find best position".
int finalize_job(kh_matcher * m, CorrReq & q, CorrHost & c, const ResultView & v)
{
  int rc = KH_OK;
  Slot & s = m->slots[c.slot];
  s.volume_stale = false;
  const unsigned long long * out = v.out;
  double best;
  std::memcpy(&best, &out[0], 8);
  const uint64_t tie_count = out[1];
  const size_t plane = static_cast<size_t>(c.nx) * c.ny;
  std::vector<uint32_t> ties;
  std::vector<int32_t> host_sums;     // full volume, only when needed
  auto fetch_volume = [&]() -> int {
    if (!host_sums.empty()) {return KH_OK;}
    if (!v.device_work) {return kNeedGeneric;}
    host_sums.resize(plane * c.na);
    KH_HIP(hipMemcpy(host_sums.data(), s.d_sums, host_sums.size() * 4, hipMemcpyDeviceToHost));
    return KH_OK;
  };
  if (tie_count <= static_cast<uint64_t>(kTieCap)) {
    const uint32_t * idx = reinterpret_cast<const uint32_t *>(out + 2);
    ties.assign(idx, idx + tie_count);
    std::sort(ties.begin(), ties.end());
  } else {
    // degenerate search (e.g. nothing rasterised: every pose ties at 0): walk the whole volume
    // on the host in the reference's order
    rc = fetch_volume(); if (rc) {return rc;}
    for (int32_t yi = 0; yi < c.ny; ++yi) {
      for (int32_t xi = 0; xi < c.nx; ++xi) {
        for (int32_t a = 0; a < c.na; ++a) {
          const double r = host_response(c, host_sums[static_cast<size_t>(a) * plane + static_cast<size_t>(yi) * c.nx + xi], a, yi, xi);
          if (double_equal(r, best)) {ties.push_back(static_cast<uint32_t>((static_cast<size_t>(yi) * c.nx + xi) * c.na + a));}
        }
      }
    }
  }
  if (ties.empty()) {q.status = KH_ERR_SEARCH; return KH_OK;}     // Mapper.cpp:828
  // average all poses with the same highest response, Mapper.cpp:802-829
  double ax = 0.0, ay = 0.0, thetaX = 0.0, thetaY = 0.0;
  for (uint32_t t : ties) {
    const int32_t a = static_cast<int32_t>(t % static_cast<uint32_t>(c.na));
    const uint32_t xy = t / static_cast<uint32_t>(c.na);
    const int32_t xi = static_cast<int32_t>(xy % static_cast<uint32_t>(c.nx)), yi = static_cast<int32_t>(xy / static_cast<uint32_t>(c.nx));
    ax += c.center[0] + c.geo->x_poses[xi];
    ay += c.center[1] + c.geo->y_poses[yi];
    const double heading = normalize_angle(c.angles[a]);
    double sin_h, cos_h;
    ref_sincos(heading, &sin_h, &cos_h);
    thetaX += cos_h;
    thetaY += sin_h;
  }
  const int32_t count = static_cast<int32_t>(ties.size());
  ax /= count; ay /= count; thetaX /= count; thetaY /= count;
  const double avg[3] = {ax, ay, std::atan2(thetaY, thetaX)};

  if (!c.fine) {
    const double * lattice = reinterpret_cast<const double *>(out + kOutHeaderWords);
    WalkLattice wl;
    wl.center[0] = c.center[0]; wl.center[1] = c.center[1]; wl.off_x = c.off_x; wl.off_y = c.off_y;
    wl.nx = c.nx; wl.ny = c.ny; wl.x_poses = c.geo->x_poses.data(); wl.y_poses = c.geo->y_poses.data();
    WalkGeometry wg;
    std::copy(c.center, c.center + 3, wg.center);
    wg.off_x = c.off_x; wg.off_y = c.off_y; wg.res_x = c.res_x; wg.res_y = c.res_y; wg.ang_res = c.ang_res;
    const int prc = positional_covariance(m->side, m->resolution, wl, lattice, wg, avg, best, q.cov);
    if (prc != KH_OK) {q.status = prc; return KH_OK;}
    // m_pSearchSpaceProbs of this matcher slot
    s.last_coarse = wl; s.last_coarse_geo = c.geo; s.last_lattice.assign(lattice, lattice + plane); s.has_last_coarse = true;
  } else {
    // ComputeAngularCovariance, Mapper.cpp:977-1025
    const double bestAngle = normalize_angle_difference(avg[2], c.center[2]);
    const Cell g = world_to_grid(m->scale, s.off_x, s.off_y, avg[0], avg[1]);
    const int32_t gridIndex = (g.x + m->roi_x) + (g.y + m->roi_y) * m->ws;
    // the raw responses of all angles at that cell: it is a lattice point unless the tie average
    // left the lattice, in which case the sums are recomputed by a 1x1 search at that cell
    int32_t fx = -1, fy = -1;
    for (int32_t yi = 0; yi < c.ny && fx < 0; ++yi) {
      for (int32_t xi = 0; xi < c.nx; ++xi) {
        if (c.bx[xi] + c.by[yi] == gridIndex) {fx = xi; fy = yi; break;}
      }
    }
    std::vector<int32_t> col(c.na, 0);
    if (fx >= 0 && v.small != nullptr) {
      const int32_t * vol = v.small;
      for (int32_t a = 0; a < c.na; ++a) {col[a] = vol[static_cast<size_t>(a) * plane + static_cast<size_t>(fy) * c.nx + fx];}
    } else if (!v.device_work) {
      return kNeedGeneric;
    } else if (fx >= 0) {
      KH_HIP(hipMemcpy2D(col.data(), 4, s.d_sums + static_cast<size_t>(fy) * c.nx + fx, plane * 4, 4, c.na, hipMemcpyDeviceToHost));
    } else {
      // off-lattice best pose: score the single cell through the generic (per-pose checked) path.  Finalisation may
      // run on pool threads: one of them at a time talks to the stream
      static std::mutex rescore_mutex;
      std::lock_guard<std::mutex> rescore_lock(rescore_mutex);
      s.volume_stale = true;
      CorrJob * job = v.h_job;
      CorrJob one = *job;
      one.nx = 1; one.ny = 1; one.linear = 0; one.sx = 1; one.sy_ws = m->ws; one.base0 = gridIndex;
      one.tiles_x = 1; one.tiles_y = 1; one.ry = 1; one.do_penalize = 0; one.coarse = 0; one.write_resp = 0;
      // bx/by of the single pose: reuse the first entries of the staged arrays
      int32_t one_bx = gridIndex, one_by = 0;
      KH_HIP(hipMemcpy(const_cast<int32_t *>(job->bx), &one_bx, 4, hipMemcpyHostToDevice));
      KH_HIP(hipMemcpy(const_cast<int32_t *>(job->by), &one_by, 4, hipMemcpyHostToDevice));
      KH_HIP(hipMemcpy(v.d_job, &one, sizeof(CorrJob), hipMemcpyHostToDevice));
      launch_offsets(v.d_job, v.stride, 1, one.na, m->stream);
      launch_score(v.d_job, v.stride, 1, 1, one.na, 1, 1, m->stream);
      KH_HIP(hipStreamSynchronize(m->stream));
      KH_HIP(hipMemcpy(col.data(), s.d_sums, sizeof(int32_t) * c.na, hipMemcpyDeviceToHost));
      // (the slot's stored volume now holds this 1 x 1 search: kh_matcher_read_volume reports KH_ERR_NOT_FOUND)
    }
    q.cov[8] = angular_variance(col, c.denom, c.center[2], c.ang_off, c.ang_res, bestAngle, best);
  }
  q.mean[0] = avg[0]; q.mean[1] = avg[1]; q.mean[2] = avg[2];
  q.response = best > 1.0 ? 1.0 : best;
  s.last.P = c.P; s.last.nx = c.nx; s.last.ny = c.ny; s.last.na = c.na; s.last.denom = c.denom; s.has_last = true;
  return KH_OK;
}

// A chunk of CorrelateScan jobs goes through in two calls so that two chunks can be pipelined: enqueue_chunk = host preparation
// + upload + kernels + download, all enqueued, ending with B.done; finish_chunk = wait for B.done + finalisation.  Everything the
// second needs lives in the CorrBatch.

// fine passes with volumes up to this many poses have them downloaded with the results (ComputeAngularCovariance reads them)
constexpr size_t kSmallVolume = 4096;

// KH_MATCH_TIMING=1: wall split of the stages, printed every 64 calls (diagnostics only)
struct StageTiming
{
  bool on = std::getenv("KH_MATCH_TIMING") != nullptr;
  double acc[4] = {0, 0, 0, 0};     // prepare, enqueue, wait, finalise
  long calls = 0;
  void lap(int slot, std::chrono::steady_clock::time_point from)
  {
    if (on) {acc[slot] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - from).count();}
  }
};
static StageTiming & stage_timing()
{
  static StageTiming t;
  return t;
}

static int enqueue_chunk(kh_matcher * m, CorrReq * reqs, size_t n, CorrBatch & B, bool overlap)
{
  if (n == 0) {return KH_OK;}
  StageTiming & timing = stage_timing();
  const auto t_enter = std::chrono::steady_clock::now();
  int rc = KH_OK;
  B.ctx.assign(n, CorrHost()); B.lay.assign(n, StageLayout());
  B.stride = 0; B.out_words = 0;
  int32_t max_na = 0, max_poses = 0;

  // ---- 1. host preparation (exact reference arithmetic) ----
  for (size_t i = 0; i < n; ++i) {
    CorrReq & q = reqs[i];
    CorrHost & c = B.ctx[i];
    q.status = KH_OK;
    rc = init_ctx(q, c);
    if (rc) {return rc;}
    // (a chunk's jobs share their geometry: after the first this is a look-up)
    rc = attach_table(m, q, c, q.penalize);
    if (rc) {return rc;}
    B.lay[i] = stage_layout(c.P, c.nx, c.ny, c.na, false);
    B.stride = std::max(B.stride, B.lay[i].total);
    B.out_words = std::max(B.out_words, kOutHeaderWords + static_cast<size_t>(c.nx) * c.ny);
    max_na = std::max(max_na, c.na);
    max_poses = std::max(max_poses, c.nx * c.ny * c.na);
  }
  B.out_words = align_up(B.out_words, 32);
  const size_t stride = B.stride, out_words = B.out_words;
  rc = ensure_pinned(B.h_stage, B.cap_stage, stride * n, m->stream);
  if (rc) {return rc;}
  rc = ensure_device(B.d_stage, B.cap_dstage, B.cap_stage, m->stream);
  if (rc) {return rc;}
  rc = ensure_pinned(B.h_out, B.cap_hout, out_words * n, m->stream);
  if (rc) {return rc;}
  rc = ensure_device(B.d_out, B.cap_dout, out_words * n, m->stream);
  if (rc) {return rc;}

  // device scratch of every slot first (allocation is serial); the tables themselves are filled by
  // the host pool
  for (size_t i = 0; i < n; ++i) {
    rc = ensure_slot_scratch(m, reqs[i], B.ctx[i]);
    if (rc) {return rc;}
  }
  // LDS-staged scoring (k_offsets_lds / k_score_lds): by default for the searches it was measured faster on -- windows of at most
  // 61 bytes x 64 rows with >= 1e8 lookups per search, in launches of >= 512 angle pairs (the config-2 CorrelateScan in batches:
  // 0.48 against 0.60 ms per 51 matches); smaller searches and small launches keep the windowed kernel, whose fixed costs are lower.  kh_matcher_set_debug bit 1:
  // every search the path can take; bit 6: none.
  const bool lds_never = m->windowed_score;
  const bool lds_always = !lds_never && m->lds_score;
  std::vector<JobShape> shapes(n);
  HostPool::instance().run(n, [&](size_t i) {
    prepare_job(m, reqs[i], B.ctx[i], B.lay[i], B.h_stage + stride * i, B.d_stage + stride * i, B.d_out + out_words * i, out_words, n,
      lds_always, lds_never, shapes[i]);
  });
  if (timing.on) {
    const CorrJob * j0 = reinterpret_cast<const CorrJob *>(B.h_stage);
    std::fprintf(stderr, "[kh corr] job 0: %d x %d x %d poses, sx %d, tiles %d x %d of %d x %d poses, lists per tile %d, copies %d (slot kind %d), "
      "dec %d, ws %d\n", j0->nx, j0->ny, j0->na, j0->sx, j0->tiles_x, j0->tiles_y, j0->tile_px, 4 * j0->ry, j0->list_tiles,
      j0->grid2 ? 1 : 0, m->slots[B.ctx[0].slot].copy_kind, j0->dec, m->ws);
  }
  // one scoring launch for the chunk if every job takes the same kernel instance
  int32_t max_tiles = 0, sx_variant = shapes[0].sx, ry = shapes[0].ry;
  // (the LDS-staged kernels score the grid itself with the lattice's own step: a two-cell search on a slot that holds column-decimated
  // copies is a one-cell search for the windowed kernel only)
  const int32_t lds_sx = shapes[0].lds_sx;
  bool uniform_kernel = true, all_lds = true;
  for (size_t i = 0; i < n; ++i) {
    if (sx_variant != shapes[i].sx || ry != shapes[i].ry) {uniform_kernel = false;}
    all_lds = all_lds && shapes[i].lds_sx == lds_sx;
    max_tiles = std::max(max_tiles, shapes[i].tiles);
    all_lds = all_lds && shapes[i].lds != 0;
  }
  B.use_lds = all_lds && uniform_kernel;
  int32_t tile_pairs = 0;
  for (size_t i = 0; i < n; ++i) {
    CorrJob * job = reinterpret_cast<CorrJob *>(B.h_stage + stride * i);
    if (B.use_lds) {
      // the LDS-staged kernel scores an angle's whole lattice in one workgroup: one scoring tile per angle for K4
      job->tiles_x = 1; job->tiles_y = 1; job->ry = 16; job->tile_px = kTileSpan;
      // ... and keeps the search-space probabilities in its epilogue: K4 is the tie scan alone
      job->cells_in_score = 1;
    }
    tile_pairs = std::max(tile_pairs, job->na * job->tiles_x * job->tiles_y);
  }

  // ---- 2. upload, launch, download ----
  timing.lap(0, t_enter);
  const auto t_enqueue = std::chrono::steady_clock::now();
  // overlap (chunked batches): everything of a chunk -- uploads, the table / list kernel K2, the scoring kernel K3, the tie scan K4
  // and the downloads -- goes on its staging set's side stream, and happens under the scoring of its neighbours
  hipStream_t cs = overlap ? B.side : m->stream;
  KH_HIP(hipMemcpyAsync(B.d_stage, B.h_stage, stride * n, hipMemcpyHostToDevice, cs));
  // (the result blocks are zeroed by K2)
  if (m->profiling) {KH_HIP(hipEventRecord(B.evs[0], cs));}
  if (B.use_lds) {
    launch_offsets_lds(B.d_stage, stride, static_cast<int32_t>(n), max_na, cs);
  } else {
    launch_offsets(B.d_stage, stride, static_cast<int32_t>(n), max_na, cs);
  }
  if (m->profiling) {KH_HIP(hipEventRecord(B.evs[1], cs));}
  // The scoring kernel of a chunk goes on the chunk's own side stream as well: the two staging sets then are two independent
  // in-order queues, and the workgroups of chunk i + 1 fill the compute units the tail of chunk i leaves idle (2099 workgroups on
  // 512 slots are 4.1 rounds: a fifth of the kernel's time ran at a tenth of the occupancy).
  if (m->profiling) {KH_HIP(hipEventRecord(B.ev[0], cs));}
  if (B.use_lds) {
    bool full_rows = true;
    for (size_t i = 0; i < n; ++i) {full_rows = full_rows && lds_row_waves(B.ctx[i].ny) == 4;}
    launch_score_lds(B.d_stage, stride, static_cast<int32_t>(n), max_na, lds_sx, full_rows, cs);
  } else if (uniform_kernel) {
    launch_score(B.d_stage, stride, static_cast<int32_t>(n), max_tiles, max_na, sx_variant, ry, cs);
  } else {
    for (size_t i = 0; i < n; ++i) {
      const CorrJob * job = reinterpret_cast<const CorrJob *>(B.h_stage + stride * i);
      launch_score(B.d_stage + stride * i, stride, 1, job->tiles_x * job->tiles_y, job->na,
        (job->linear && job->sx == 2 && !job->dec) ? 2 : 1, job->ry, cs);
    }
  }
  if (m->profiling) {KH_HIP(hipEventRecord(B.ev[1], cs)); KH_HIP(hipEventRecord(B.evs[2], cs));}
  launch_ties(B.d_stage, stride, static_cast<int32_t>(n), max_poses, tile_pairs, B.use_lds, cs);
  if (m->profiling) {KH_HIP(hipEventRecord(B.evs[3], cs));}
  KH_HIP(hipGetLastError());
  KH_HIP(hipMemcpyAsync(B.h_out, B.d_out, out_words * 8 * n, hipMemcpyDeviceToHost, cs));
  // fine passes need the raw sums of every angle at the best cell (ComputeAngularCovariance): their
  // volumes are tiny (3 x 3 x nA), so they ride along with the batch download instead of costing one
  // synchronous copy per match afterwards
  size_t max_small = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t vol = static_cast<size_t>(B.ctx[i].nx) * B.ctx[i].ny * B.ctx[i].na;
    if (B.ctx[i].fine && vol <= kSmallVolume) {max_small = std::max(max_small, vol);}
  }
  B.small_stride = align_up(max_small, 32);
  if (max_small) {
    rc = ensure_pinned(B.h_sums, B.cap_hsums, B.small_stride * n, m->stream); if (rc) {return rc;}
    rc = ensure_device(B.d_small, B.cap_dsmall, B.small_stride * n, m->stream); if (rc) {return rc;}
    launch_gather_small(B.d_stage, stride, static_cast<int32_t>(n), B.d_small, static_cast<int32_t>(B.small_stride), cs);
    KH_HIP(hipMemcpyAsync(B.h_sums, B.d_small, B.small_stride * n * 4, hipMemcpyDeviceToHost, cs));
  }
  KH_HIP(hipEventRecord(B.done, cs));
  timing.lap(1, t_enqueue);
  return KH_OK;
}

// KH_LDS_DEBUG: what the LDS-staged path made of job 0 of a finished chunk (its chunk descriptors), on stderr
static int dump_lds_chunks(const kh_matcher * m, const CorrBatch & B)
{
  const CorrHost & c0 = B.ctx[0];
  const Slot & s0 = m->slots[c0.slot];
  const size_t groups = (static_cast<size_t>(c0.na) + kGroupAngles - 1) / kGroupAngles;
  const size_t range_len = static_cast<size_t>(lds_desc_capacity(c0.P));
  std::vector<int32_t> cc(groups * kLdsRanges), dd(groups * kLdsRanges * range_len * kChunkWords);
  KH_HIP(hipMemcpy(cc.data(), s0.d_chunk_counts, cc.size() * 4, hipMemcpyDeviceToHost));
  KH_HIP(hipMemcpy(dd.data(), s0.d_chunks, dd.size() * 4, hipMemcpyDeviceToHost));
  long total = 0, bytes = 0, windows = 0, maxb = 0, small = 0;
  for (size_t g = 0; g < groups * kLdsRanges; ++g) {
    for (int32_t k = 0; k < cc[g]; ++k) {
      const int32_t * d = dd.data() + (g * range_len + k) * kChunkWords;
      ++total; bytes += static_cast<long>(d[2]) * kLdsPitch; windows += d[3];
      maxb = std::max<long>(maxb, static_cast<long>(d[2]) * kLdsPitch);
      if (d[3] < 16) {++small;}
    }
  }
  std::fprintf(stderr, "[kh lds] job 0: %zu angle pairs, %ld chunks (%.1f per pair, %ld with < 16 windows), mean region %.1f KB, max %.1f KB, "
    "%.1f windows per chunk, %.0f staged bytes per window\n",
    groups, total, static_cast<double>(total) / groups, small, bytes / 1024.0 / std::max(1l, total), maxb / 1024.0,
    static_cast<double>(windows) / std::max(1l, total), static_cast<double>(bytes) / std::max(1l, windows));
  return KH_OK;
}

// last_of_call (the last chunk of a chunked call): nothing hides the host's work any more -- the worker pool is woken while this
// thread still waits for the chunk's results, and stays awake behind the finalisation for the first chunk of the caller's next call.
static int finish_chunk(kh_matcher * m, CorrReq * reqs, size_t n, CorrBatch & B, bool last_of_call)
{
  if (n == 0) {return KH_OK;}
  StageTiming & timing = stage_timing();
  const auto t_enter = std::chrono::steady_clock::now();
  // (what a wake-up costs -- a futex wake and the scheduler, ~50 us -- is hidden under the scoring kernels for every chunk but the
  // last, and for every preparation but the first of the next call)
  constexpr uint64_t kAwaitResults = 200 * HostPool::kTicksPerMicrosecond, kAwaitNextCall = 120 * HostPool::kTicksPerMicrosecond;
  if (last_of_call) {HostPool::instance().run(2, [](size_t) {}, kAwaitResults);}
  KH_HIP(hipEventSynchronize(B.done));
  timing.lap(2, t_enter);
  const auto t_final = std::chrono::steady_clock::now();
  if (B.use_lds && std::getenv("KH_LDS_DEBUG")) {
    const int rc = dump_lds_chunks(m, B); if (rc) {return rc;}
  }
  if (m->profiling) {
    float ms = 0;
    KH_HIP(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
    m->score_ms += ms; m->score_launches += 1; m->score_jobs += static_cast<int64_t>(n);
    KH_HIP(hipEventElapsedTime(&ms, B.evs[0], B.evs[1])); m->offsets_ms += ms;
    KH_HIP(hipEventElapsedTime(&ms, B.evs[2], B.evs[3])); m->ties_ms += ms;
  }

  // ---- 3. finalisation (Mapper.cpp:775-862) ----
  std::vector<int> final_rc(n, KH_OK);
  auto finalize = [&](size_t i) -> int {
    const CorrHost & c = B.ctx[i];
    ResultView v;
    v.out = B.h_out + B.out_words * i;
    const size_t vol = static_cast<size_t>(c.nx) * c.ny * c.na;
    v.small = (c.fine && vol <= kSmallVolume && B.h_sums) ? B.h_sums + B.small_stride * i : nullptr;
    v.h_job = reinterpret_cast<CorrJob *>(B.h_stage + B.stride * i); v.d_job = B.d_stage + B.stride * i; v.stride = B.stride;
    return finalize_job(m, reqs[i], B.ctx[i], v);
  };
  // big fine volumes and the off-lattice re-score path issue their own copies / launches on the
  // stream: keep such batches off the pool
  bool serial_final = false;
  for (const CorrHost & c : B.ctx) {
    serial_final = serial_final || (c.fine && static_cast<size_t>(c.nx) * c.ny * c.na > kSmallVolume);
  }
  if (serial_final) {
    for (size_t i = 0; i < n; ++i) {final_rc[i] = finalize(i);}
  } else {
    HostPool::instance().run(n, [&](size_t i) {
      (void)hipSetDevice(m->device);
      final_rc[i] = finalize(i);
    }, last_of_call ? kAwaitNextCall : 0);
  }
  timing.lap(3, t_final);
  static const long period = (std::getenv("KH_MATCH_TIMING") && std::atoi(std::getenv("KH_MATCH_TIMING")) > 1) ? 1 : 64;
  if (timing.on && ++timing.calls % period == 0) {
    std::fprintf(stderr, "[kh match] per call: prepare %.3f ms, enqueue %.3f ms, wait %.3f ms, finalize %.3f ms (n = %zu, stage %zu B/job)\n",
      timing.acc[0] / period, timing.acc[1] / period, timing.acc[2] / period, timing.acc[3] / period, n, B.stride);
    timing.acc[0] = timing.acc[1] = timing.acc[2] = timing.acc[3] = 0;
  }
  for (size_t i = 0; i < n; ++i) {if (final_rc[i] != KH_OK) {return final_rc[i];}}
  return KH_OK;
}

int correlate_batch(kh_matcher * m, std::vector<CorrReq> & reqs)
{
  const size_t n = reqs.size();
  if (n == 0) {return KH_OK;}
  trim_tables(m);
  // Large batches go through in chunks of kChunk jobs on the two staging sets of the handle: while the kernels of
  // chunk i run, the host prepares chunk i + 1 and finalises chunk i - 1 (the exact host half costs ~5 us per match
  // on the worker pool, the scoring kernel ~13 us).  Chunks of 64 keep the scoring launches at full efficiency;
  // splitting a batch of 32 into halves was measured slower than not splitting (0.85 against 0.76 ms), so batches
  // below 2 * kChunk are not split.
  constexpr size_t kChunk = 64;
  // ... and only searches whose scoring kernel dwarfs the hand-overs between the streams: a chunk of 64 config-2
  // searches scores for 0.85 ms, a chunk of loop-closure coarse searches (half the lookups, a quarter of the loads)
  // for 0.2 ms, and batches of those were measured 25 % slower chunked than whole
  const CorrReq & r0 = reqs[0];
  const double work0 = (round_half_away(r0.off_x * 2.0 / r0.res_x) + 1) * (round_half_away(r0.off_y * 2.0 / r0.res_y) + 1) *
    (round_half_away(r0.ang_off * 2.0 / r0.ang_res) + 1) * static_cast<double>(r0.scan->n);
  if (n < 2 * kChunk || (work0 < 2.5e8 && !m->force_chunks)) {
    int rc = enqueue_chunk(m, reqs.data(), n, m->batch[0], false);
    if (rc) {return rc;}
    return finish_chunk(m, reqs.data(), n, m->batch[0], false);
  }
  // the side streams start behind everything already queued on the main stream (the rasteriser writes the grids
  // and the occupancy block maps K2 reads); they are drained before this call returns (every chunk's `done` is
  // waited for), so later main-stream work needs no edge back
  KH_HIP(hipEventRecord(m->batch[0].kdone, m->stream));
  for (auto & b : m->batch) {KH_HIP(hipStreamWaitEvent(b.side, m->batch[0].kdone, 0));}
  // a shorter first chunk: the pipeline fills on it (its preparation, upload and K2 are exposed) and drains on the last (its
  // K4, download and finalisation are).  256 config-2 matches as 24 + 64 + 64 + 64 + 40 measured 79.9 k and 81.4 k matches/s
  // on two boxes where 32 + 64 + 64 + 64 + 32 (the split of rounds 2-3) gave 78.4 k and 76.5 k, a first chunk of 16 74.4 k,
  // uniform chunks of 64 less again; splits sized to whole rounds of workgroups (24 + 62 + 62 + 62 + 46) measured no better
  // than the plain one.
  constexpr size_t kEdgeChunk = 24;
  std::vector<size_t> bounds{0};
  for (size_t at = kEdgeChunk; at + kEdgeChunk < n; at += kChunk) {bounds.push_back(at);}
  if (n - bounds.back() > kChunk) {bounds.push_back(n - kEdgeChunk);}
  bounds.push_back(n);
  const size_t chunks = bounds.size() - 1;
  auto begin_of = [&](size_t c) {return bounds[c];};
  auto size_of = [&](size_t c) {return bounds[c + 1] - bounds[c];};
  int first_rc = KH_OK;
  int rc = enqueue_chunk(m, reqs.data(), size_of(0), m->batch[0], true);
  if (rc) {return rc;}
  for (size_t c = 1; c < chunks; ++c) {
    rc = enqueue_chunk(m, reqs.data() + begin_of(c), size_of(c), m->batch[c & 1], true);
    if (rc) {(void)hipStreamSynchronize(m->stream); for (auto & b : m->batch) {(void)hipStreamSynchronize(b.side);} return rc;}
    rc = finish_chunk(m, reqs.data() + begin_of(c - 1), size_of(c - 1), m->batch[(c - 1) & 1], false);
    if (rc && !first_rc) {first_rc = rc;}
  }
  rc = finish_chunk(m, reqs.data() + begin_of(chunks - 1), size_of(chunks - 1), m->batch[(chunks - 1) & 1], true);
  return first_rc ? first_rc : rc;
}

}  // namespace kh

namespace kh
{
// for the other translation units of the library (kh_matcher is private to this one)
int32_t matcher_max_batch(const kh_matcher * m) {return m ? m->max_batch : 0;}
}

// =============================================================================================
//                                         C ABI
// =============================================================================================
extern "C" {

const char * kh_last_error(void) {return kh::g_last_error.c_str();}

int kh_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {return 0;}
  return n;
}

const char * kh_version(void) {return "karto-hip 0.1 (gfx950)";}

int kh_scan_points(const double * ranges, int32_t n, const double sensor_pose[3], double min_angle,
  double angular_resolution, double * out)
{
  if (!ranges || !out || n < 0) {return KH_ERR_INVALID_ARG;}
  for (int32_t i = 0; i < n; ++i) {          // Karto.h:5663-5682
    const double angle = sensor_pose[2] + min_angle + static_cast<uint32_t>(i) * angular_resolution;
    double sin_a, cos_a;
    ref_sincos(angle, &sin_a, &cos_a);
    out[2 * i] = sensor_pose[0] + (ranges[i] * cos_a);
    out[2 * i + 1] = sensor_pose[1] + (ranges[i] * sin_a);
  }
  return KH_OK;
}

void kh_match_params_default(kh_match_params * p)
{
  // Mapper.cpp:2250-2293
  p->coarse_search_angle_offset = 20 * kPi180;
  p->coarse_angle_resolution = 2 * kPi180;
  p->fine_search_angle_offset = 0.2 * kPi180;
  p->use_response_expansion = 0;
  p->distance_variance_penalty = 0.3 * 0.3;
  p->minimum_distance_penalty = 0.5;
  p->angle_variance_penalty = (20 * kPi180) * (20 * kPi180);
  p->minimum_angle_penalty = 0.9;
}

int kh_matcher_create(double search_size, double resolution, double smear, double range_threshold,
  int32_t device, int32_t max_batch, kh_matcher ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  // Mapper.cpp:481-493
  if (resolution <= 0 || search_size <= 0 || smear < 0 || range_threshold <= 0 || max_batch < 1) {
    set_error("ScanMatcher::Create: invalid parameters");
    return KH_ERR_INVALID_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    set_error("no usable HIP device (libkartohip has no CPU fallback)");
    return KH_ERR_NO_DEVICE;
  }
  kh_matcher * m = new kh_matcher();
  m->search_size = search_size; m->resolution = resolution; m->smear = smear; m->range_threshold = range_threshold;
  m->device = device; m->max_batch = max_batch;
  kh_match_params_default(&m->params);
  // Mapper.cpp:498-505
  const uint32_t side = static_cast<uint32_t>(round_half_away(search_size / resolution) + 1);
  const uint32_t margin = static_cast<uint32_t>(std::ceil(range_threshold / resolution));
  const int32_t grid_size = static_cast<int32_t>(side + 2 * margin);
  // CorrelationGrid::CreateGrid / ctor, Mapper.h:1099-1114, 1194-1208; Grid::Resize Karto.h:4636-4664
  const uint32_t border = static_cast<uint32_t>(half_kernel_size(smear, resolution)) + 1;
  m->width = grid_size + 2 * static_cast<int32_t>(border);
  m->height = m->width;
  m->ws = static_cast<int32_t>((static_cast<size_t>(m->width) + 7) & ~static_cast<size_t>(7));
  const int64_t ds = static_cast<int64_t>(m->ws) * m->height;
  if (ds <= 0 || ds > (1ll << 31) - 4096) {delete m; set_error("grid too large"); return KH_ERR_INVALID_ARG;}
  m->data_size = static_cast<int32_t>(ds);
  m->scale = 1.0 / resolution;
  m->roi_x = m->roi_y = static_cast<int32_t>(border);
  m->roi_w = m->roi_h = grid_size;
  m->side = static_cast<int32_t>(side);
  // CalculateKernel, Mapper.h:1213-1266
  const double res = m->grid_resolution();
  const double min_dev = 0.5 * res, max_dev = 10 * res;
  if (!(smear >= min_dev && smear <= max_dev)) {
    delete m;
    set_error("Mapper Error:  Smear deviation too small / too large");
    return KH_ERR_INVALID_ARG;
  }
  m->kernel_size = 2 * half_kernel_size(smear, res) + 1;
  const int32_t k = m->kernel_size, hk = k / 2;
  m->kernel.resize(static_cast<size_t>(k) * k);
  for (int32_t i = -hk; i <= hk; ++i) {
    for (int32_t j = -hk; j <= hk; ++j) {
      const double distance_from_mean = hypot(i * res, j * res);
      const double z = exp(-0.5 * pow(distance_from_mean / smear, 2));
      const uint32_t v = static_cast<uint32_t>(round_half_away(z * 100));
      m->kernel[(i + hk) + k * (j + hk)] = static_cast<uint8_t>(v);
      if (v == 100) {m->footprint100.push_back(Cell{i, j});}
    }
  }

  if (m->footprint100.size() > static_cast<size_t>(kMaxFootprint) + 1) {
    // cannot happen inside [0.5, 10] x resolution: the diagonal neighbours reach 99 at sigma / res = 10
    delete m; set_error("smear kernel with more than five cells of 100"); return KH_ERR_INVALID_ARG;
  }
  auto fail = [&](hipError_t e, const char * what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    kh_matcher_destroy(m);
    return KH_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) {return fail(e, "hipSetDevice");}
  if ((e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking)) != hipSuccess) {return fail(e, "hipStreamCreate");}
  for (auto & ev : m->ev) {
    if ((e = hipEventCreate(&ev)) != hipSuccess) {return fail(e, "hipEventCreate");}
  }
  for (auto & b : m->batch) {
    for (auto & ev : b.ev) {
      if ((e = hipEventCreate(&ev)) != hipSuccess) {return fail(e, "hipEventCreate");}
    }
    for (auto & ev : b.evs) {
      if ((e = hipEventCreate(&ev)) != hipSuccess) {return fail(e, "hipEventCreate");}
    }
    if ((e = hipEventCreateWithFlags(&b.done, hipEventDisableTiming)) != hipSuccess) {return fail(e, "hipEventCreate");}
    if ((e = hipEventCreateWithFlags(&b.kdone, hipEventDisableTiming)) != hipSuccess) {return fail(e, "hipEventCreate");}
    if ((e = hipStreamCreateWithFlags(&b.side, hipStreamNonBlocking)) != hipSuccess) {return fail(e, "hipStreamCreate");}
  }
  if ((e = hipMalloc(reinterpret_cast<void **>(&m->d_kernel), m->kernel.size())) != hipSuccess) {return fail(e, "hipMalloc kernel");}
  // (word 0 = the tally; the words behind it are used by measurement builds of the kernels only)
  if ((e = hipMalloc(reinterpret_cast<void **>(&m->d_load_counter), 512)) != hipSuccess) {return fail(e, "hipMalloc counter");}
  if ((e = hipMemset(m->d_load_counter, 0, 512)) != hipSuccess) {return fail(e, "hipMemset counter");}
  if ((e = hipMemcpy(m->d_kernel, m->kernel.data(), m->kernel.size(), hipMemcpyHostToDevice)) != hipSuccess) {return fail(e, "hipMemcpy kernel");}
  // zero rows either side: as many as the SEARCH SPACE is high (m->side cells: 61 / 161 / 51 for the C2 / L / S presets -- not the
  // grid's region of interest, which also spans the range threshold), so that any search window that touches the array is inside
  m->pad_rows = m->side + 8;
  m->grid_pad = align_up(static_cast<size_t>(m->pad_rows) * m->ws, 256) + kGridPad;
  m->pitch2 = static_cast<int32_t>(align_up(static_cast<size_t>(m->ws), 128));
  {
    const size_t copy = align_up(static_cast<size_t>(m->pitch2) * (m->data_size / m->ws + 2 * m->pad_rows) + 256, 256);
    if (2 * copy + 256 > (1ull << 31) - 4096) {m->dual_copy = false;}        // offsets into the copies are int32
    m->copy_b = static_cast<int32_t>(std::min<size_t>(copy, (1ull << 30)));
  }
  {
    m->pitch_d = static_cast<int32_t>(align_up(static_cast<size_t>(m->ws) / 2 + 64, 128));
    const size_t quarter = align_up(static_cast<size_t>(m->pitch_d) * (m->data_size / m->ws + 2 * m->pad_rows) + 256, 256);
    m->copy_q = 4 * quarter + 4096 < (1ull << 31) ? static_cast<int32_t>(quarter) : 0;
  }
  m->rt_w = (m->ws + kRasterTile - 1) / kRasterTile;
  m->rt_h = (m->data_size / m->ws + kRasterTile - 1) / kRasterTile;
  // occupancy block map: 8 x 8-cell blocks where the searches are small, a stamp is, and the handle is made for batches (a stamp marks every block its footprint
  // overlaps: 41 x 41 cells are 49 blocks of 8 x 8), 32 x 32-cell blocks otherwise.  On the config-2 search the finer map leaves
  // out 9 % more windows.
  // (handles made for batches: one match at a time builds its map inside one workgroup, where the coarse map is the cheaper one)
  m->bshift = (m->kernel_size <= 25 && m->side <= 64 && max_batch >= 8) ? 3 : kBlockShift;
  m->bm_w = (((m->ws >> m->bshift) + 1) + 31) / 32 + 1;     // words per block row (+1 padding word)
  m->bm_h = (m->data_size / m->ws >> m->bshift) + 2;
  // Batches take the first-point rasteriser (matcher_seq.hip) where every slot can have its table over the region of interest --
  // 4 bytes per cell: 66 MB for the sequential preset, 260 MB for the config-2 geometry -- within 24 GB per handle
  {
    const double table_bytes = 4.0 * static_cast<double>(m->roi_w) * m->roi_h * max_batch;
    m->table_raster = table_bytes <= 24e9 && m->rt_w * m->rt_h <= 16384;
  }
  m->slots.resize(max_batch);
  for (auto & s : m->slots) {
    if ((e = hipMalloc(reinterpret_cast<void **>(&s.d_grid_alloc), static_cast<size_t>(m->data_size) + 2 * m->grid_pad)) != hipSuccess) {return fail(e, "hipMalloc grid");}
    if ((e = hipMemset(s.d_grid_alloc, 0, static_cast<size_t>(m->data_size) + 2 * m->grid_pad)) != hipSuccess) {return fail(e, "hipMemset grid");}
    s.d_grid = s.d_grid_alloc + m->grid_pad;
    if ((e = hipMalloc(reinterpret_cast<void **>(&s.d_blockmap), static_cast<size_t>(m->bm_w) * m->bm_h * 4)) != hipSuccess) {return fail(e, "hipMalloc block map");}
    if ((e = hipMemset(s.d_blockmap, 0, static_cast<size_t>(m->bm_w) * m->bm_h * 4)) != hipSuccess) {return fail(e, "hipMemset block map");}
    if ((e = hipMalloc(reinterpret_cast<void **>(&s.d_rtiles), (4 * static_cast<size_t>(m->rt_w) * m->rt_h + 8) * sizeof(int32_t))) != hipSuccess) {return fail(e, "hipMalloc raster tiles");}
    // tiles the slot's previous rasterisation wrote ([0] = how many): none yet, the grid is all zero
    const size_t prev_bytes = (static_cast<size_t>(m->rt_w) * m->rt_h + 4) * sizeof(int32_t);
    if ((e = hipMalloc(reinterpret_cast<void **>(&s.d_prev_work), prev_bytes)) != hipSuccess) {return fail(e, "hipMalloc tile list");}
    if ((e = hipMemset(s.d_prev_work, 0, prev_bytes)) != hipSuccess) {return fail(e, "hipMemset tile list");}
  }
  if ((e = hipHostMalloc(reinterpret_cast<void **>(&m->h_rjobs), sizeof(RasterJob) * max_batch, hipHostMallocDefault)) != hipSuccess) {return fail(e, "hipHostMalloc");}
  if ((e = hipMalloc(reinterpret_cast<void **>(&m->d_rjobs), sizeof(RasterJob) * max_batch)) != hipSuccess) {return fail(e, "hipMalloc");}
  // (the fills above run on the null stream, which the handle's own non-blocking streams do not wait for: a rasterisation that
  // starts with little host work in front of it -- from a map -- must not be overtaken by the zeroing of its grid)
  if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) {return fail(e, "hipStreamSynchronize");}
  *out = m;
  return KH_OK;
}

void kh_matcher_destroy(kh_matcher * m)
{
  if (!m) {return;}
  hipSetDevice(m->device);
  if (m->stream) {hipStreamSynchronize(m->stream);}
  seq_destroy(m);
  for (auto & s : m->slots) {
    hipFree(s.d_grid_alloc); hipFree(s.d_grid2_alloc); hipFree(s.d_prev_work); hipFree(s.d_blockmap); hipFree(s.d_rtiles); hipFree(s.d_rlists); hipFree(s.d_tile_best); hipFree(s.d_table); hipFree(s.d_fast); hipFree(s.d_tcounts); hipFree(s.d_slow); hipFree(s.d_counts);
    hipFree(s.d_chunks); hipFree(s.d_chunk_counts);
    hipFree(s.d_sums); hipFree(s.d_resp); hipFree(s.d_ractive);
    hipFree(s.d_hkeys); hipFree(s.d_hvals); hipFree(s.d_hstate); hipFree(s.d_hnbr);
    hipFree(s.d_first); hipFree(s.d_cand); hipFree(s.d_seqctl); hipFree(s.d_work2); hipFree(s.d_mappts);
  }
  hipFree(m->d_kernel); hipFree(m->d_rjobs); hipFree(m->d_load_counter); hipFree(m->d_tab);
  for (auto & b : m->batch) {
    hipFree(b.d_stage); hipFree(b.d_out); hipFree(b.d_small);
    if (b.h_stage) {hipHostFree(b.h_stage);}
    if (b.h_out) {hipHostFree(b.h_out);}
    if (b.h_sums) {hipHostFree(b.h_sums);}
    for (auto & ev : b.ev) {if (ev) {hipEventDestroy(ev);}}
    for (auto & ev : b.evs) {if (ev) {hipEventDestroy(ev);}}
    if (b.done) {hipEventDestroy(b.done);}
    if (b.kdone) {hipEventDestroy(b.kdone);}
    if (b.side) {hipStreamSynchronize(b.side); hipStreamDestroy(b.side);}
  }
  for (auto & t : m->tables) {hipFree(t->d_dist_pen); t->d_dist_pen = nullptr;}
  hipFree(m->d_arena); hipFree(m->d_meta);
  hipFree(m->d_mapjobs); hipFree(m->d_maptotal); hipFree(m->d_mapunits);
  if (m->h_mapjobs) {hipHostFree(m->h_mapjobs);}
  if (m->h_maptotal) {hipHostFree(m->h_maptotal);}
  for (auto & ev : m->ev_map) {if (ev) {hipEventDestroy(ev);}}
  if (m->h_arena) {hipHostFree(m->h_arena);}
  if (m->h_meta) {hipHostFree(m->h_meta);}
  if (m->h_rjobs) {hipHostFree(m->h_rjobs);}
  for (auto & ev : m->ev) {if (ev) {hipEventDestroy(ev);}}
  if (m->stream) {hipStreamDestroy(m->stream);}
  delete m;
}

int kh_matcher_set_params(kh_matcher * m, const kh_match_params * p)
{
  if (!m || !p) {return KH_ERR_INVALID_ARG;}
  if (!(p->coarse_angle_resolution != 0.0) || !(p->fine_search_angle_offset != 0.0) ||
    p->minimum_distance_penalty < 0.0 || p->minimum_angle_penalty < 0.0)
  {
    set_error("invalid match parameters");
    return KH_ERR_INVALID_ARG;
  }
  m->params = *p;
  return KH_OK;
}

int kh_matcher_set_debug(kh_matcher * m, int32_t keep_response_volume)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  m->keep_responses = (keep_response_volume & 1) != 0;
  m->lds_score = (keep_response_volume & 2) != 0;
  m->windowed_score = (keep_response_volume & 64) != 0;
  m->no_seq = (keep_response_volume & 128) != 0;
  m->dense_score = (keep_response_volume & 4) != 0;
  m->force_chunks = (keep_response_volume & 8) != 0;
  m->dual_copy = (keep_response_volume & 16) == 0;
  return KH_OK;
}

static int check_scan(const kh_scan * s)
{
  if (!s || s->n < 0 || (s->n > 0 && (!s->ranges || !s->points_xy))) {return KH_ERR_INVALID_ARG;}
  return KH_OK;
}

int kh_matcher_add_scans(kh_matcher * m, int32_t slot, const kh_scan * query, const kh_scan * base, int32_t n_base)
{
  if (!m || slot < 0 || slot >= m->max_batch || !query || n_base < 0 || (n_base > 0 && !base)) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  std::vector<RasterReq> reqs{RasterReq{slot, query, base, n_base}};
  int rc = raster_batch(m, reqs);
  if (rc) {return rc;}
  KH_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}

// a view the map entry points can read on the matcher's device
static int check_view(const kh_matcher * m, const kh_map_view * v)
{
  if (!v || !v->device_cells || v->width <= 0 || v->height <= 0 || v->width_step < v->width || !std::isfinite(v->scale) || !(v->scale > 0.0)) {
    set_error("malformed map view");
    return KH_ERR_INVALID_ARG;
  }
  if (static_cast<int64_t>(v->width_step) * v->height > (1ll << 31) - 4096) {set_error("map view too large"); return KH_ERR_INVALID_ARG;}
  if (v->device != m->device) {set_error("the map view lies on another device than the matcher"); return KH_ERR_INVALID_ARG;}
  return KH_OK;
}

int kh_matcher_add_map(kh_matcher * m, int32_t slot, const kh_scan * query, const kh_map_view * map)
{
  if (!m || slot < 0 || slot >= m->max_batch || !query || check_view(m, map) != KH_OK) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  std::vector<RasterReq> reqs{RasterReq{slot, query, nullptr, 0, map}};
  int rc = raster_batch(m, reqs);
  if (rc) {return rc;}
  KH_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}

int kh_matcher_correlate_batch(kh_matcher * m, int32_t n, const kh_scan * queries, const double * centers,
  const double search_offset[2], const double search_resolution[2], double angle_offset,
  double angle_resolution, int32_t do_penalize, int32_t fine, double * means, double * covs,
  double * responses, int32_t * status)
{
  if (!m || n < 0 || n > m->max_batch || !queries || !centers || !means || !covs || !responses) {return KH_ERR_INVALID_ARG;}
  if (!(search_resolution[0] > 0.0) || !(search_resolution[1] > 0.0) || angle_resolution == 0.0) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  std::vector<CorrReq> reqs;
  reqs.reserve(n);
  for (int32_t i = 0; i < n; ++i) {
    if (check_scan(&queries[i]) != KH_OK || queries[i].n == 0) {return KH_ERR_INVALID_ARG;}
    reqs.emplace_back(i, &queries[i], centers + 3 * i, search_offset, search_resolution, angle_offset, angle_resolution,
      do_penalize != 0, fine != 0);
    std::copy(covs + 9 * i, covs + 9 * i + 9, reqs.back().cov);
  }
  int rc = correlate_batch(m, reqs);
  if (rc) {return rc;}
  int worst = KH_OK;
  for (int32_t i = 0; i < n; ++i) {
    std::copy(reqs[i].mean, reqs[i].mean + 3, means + 3 * i);
    std::copy(reqs[i].cov, reqs[i].cov + 9, covs + 9 * i);
    responses[i] = reqs[i].response;
    if (status) {status[i] = reqs[i].status;}
    if (reqs[i].status != KH_OK) {worst = reqs[i].status;}
  }
  return status ? KH_OK : worst;
}

int kh_matcher_correlate(kh_matcher * m, int32_t slot, const kh_scan * query, const double center[3],
  const double search_offset[2], const double search_resolution[2], double angle_offset,
  double angle_resolution, int32_t do_penalize, int32_t fine, double mean[3], double cov[9], double * response)
{
  if (!m || slot < 0 || slot >= m->max_batch || check_scan(query) != KH_OK || query->n == 0 || !mean || !cov || !response) {
    return KH_ERR_INVALID_ARG;
  }
  if (!(search_resolution[0] > 0.0) || !(search_resolution[1] > 0.0) || angle_resolution == 0.0) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  std::vector<CorrReq> reqs{CorrReq(slot, query, center, search_offset, search_resolution, angle_offset, angle_resolution,
    do_penalize != 0, fine != 0)};
  CorrReq & q = reqs[0];
  std::copy(cov, cov + 9, q.cov);
  int rc = correlate_batch(m, reqs);
  if (rc) {return rc;}
  if (q.status != KH_OK) {return q.status;}
  std::copy(q.mean, q.mean + 3, mean);
  std::copy(q.cov, q.cov + 9, cov);
  *response = q.response;
  return KH_OK;
}

}  // extern "C"

// MatchScan for n independent queries, stage by stage over the whole batch: against (query, base chain) pairs, or -- map != nullptr,
// base and base_begin unused -- all of them against one map view
static int match_batch(kh_matcher * m, int32_t n, const kh_scan * queries, const kh_scan * base,
  const int32_t * base_begin, const kh_map_view * map, int32_t do_penalize, int32_t do_refine, double * means, double * covs,
  double * responses, int32_t * status)
{
  KH_HIP(hipSetDevice(m->device));
  static const bool batch_timing = std::getenv("KH_MATCH_TIMING") != nullptr;
  const auto t_batch = std::chrono::steady_clock::now();
  struct Report {
    bool on; std::chrono::steady_clock::time_point t0; int32_t n;
    ~Report() {
      if (on) {std::fprintf(stderr, "[kh match_batch] %d matches, %.3f ms inside the call\n", n,
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());}
    }
  } report{batch_timing, t_batch, n};
  const kh_match_params & mp = m->params;
  // (a query whose readings the caller finishes later -- QueryHook, matcher_private.hpp: whatever way this call takes, they are
  // complete before it reads them, and when it returns)
  struct HookGuard {~HookGuard() {pending_query_hook().run();}} hook_guard;
  std::vector<int> st(n, KH_OK);
  std::vector<int32_t> active;
  std::vector<RasterReq> rreqs;
  for (int32_t i = 0; i < n; ++i) {
    if (check_scan(&queries[i]) != KH_OK) {return KH_ERR_INVALID_ARG;}
    const int32_t nb = map ? 0 : base_begin[i + 1] - base_begin[i];
    if (nb < 0 || (nb > 0 && !base)) {return KH_ERR_INVALID_ARG;}
    for (int32_t b = 0; b < nb; ++b) {
      if (check_scan(&base[base_begin[i] + b]) != KH_OK) {return KH_ERR_INVALID_ARG;}
    }
    double * mean = means + 3 * i; double * cov = covs + 9 * i;
    std::fill(cov, cov + 9, 0.0);
    if (queries[i].n == 0) {
      // Mapper.cpp:547-557
      std::copy(queries[i].sensor_pose, queries[i].sensor_pose + 3, mean);
      cov[0] = kMaxVariance; cov[4] = kMaxVariance;
      cov[8] = 4 * (mp.coarse_angle_resolution * mp.coarse_angle_resolution);
      responses[i] = 0.0;
      continue;
    }
    active.push_back(i);
    rreqs.push_back(RasterReq{i, &queries[i], (base && !map) ? base + base_begin[i] : nullptr, nb, map});
  }
  // ONE MatchScan -- what the reference's API issues (Mapper.cpp:2714-2717) -- takes the fused path (matcher_seq.cpp); it hands
  // back, pass by pass, whatever it could not finish
  int rc = KH_OK;
  bool coarse_done = false, fine_done = false;
  if (n == 1 && active.size() == 1 && !map) {
    int seq_status = KH_OK;
    rc = seq_match(m, &queries[0], base ? base + base_begin[0] : nullptr, base_begin[1] - base_begin[0], do_penalize != 0, do_refine != 0,
      means, covs, responses, &seq_status, &coarse_done, &fine_done);
    if (rc) {return rc;}
    if (coarse_done) {st[0] = seq_status;}
  }
  if (!coarse_done) {
    rc = raster_batch(m, rreqs);
    // (the rasteriser reads the queries' sensor poses only: readings a caller left to a QueryHook are made now, behind its launches)
    pending_query_hook().run();
    if (rc) {return rc;}
  }

  // the searches search(i) of the matches `which`, one batch
  auto run = [&](const std::vector<int32_t> & which, auto search) -> int {
    std::vector<CorrReq> reqs;
    reqs.reserve(which.size());
    for (int32_t i : which) {
      reqs.push_back(search(i));
      std::copy(covs + 9 * i, covs + 9 * i + 9, reqs.back().cov);
    }
    int r = correlate_batch(m, reqs);
    if (r) {return r;}
    for (size_t k = 0; k < which.size(); ++k) {
      const int32_t i = which[k];
      st[i] = reqs[k].status;
      if (reqs[k].status != KH_OK) {continue;}
      std::copy(reqs[k].mean, reqs[k].mean + 3, means + 3 * i);
      std::copy(reqs[k].cov, reqs[k].cov + 9, covs + 9 * i);
      responses[i] = reqs[k].response;
    }
    return KH_OK;
  };
  auto coarse = [&](double ang_off) {
    return [&, ang_off](int32_t i) {return coarse_search(m, i, &queries[i], ang_off, do_penalize != 0);};
  };
  auto fine = [&](int32_t i) {return fine_search(m, i, &queries[i], means + 3 * i, do_penalize != 0);};     // centre = rMean
  auto alive = [&](const std::vector<int32_t> & v) {
    std::vector<int32_t> o;
    for (int32_t i : v) {if (st[i] == KH_OK) {o.push_back(i);}}
    return o;
  };

  // coarse search, Mapper.cpp:588-592
  if (!coarse_done) {
    rc = run(active, coarse(mp.coarse_search_angle_offset));
    if (rc) {return rc;}
  }
  // response expansion, Mapper.cpp:594-619
  if (mp.use_response_expansion) {
    std::vector<int32_t> zero;
    for (int32_t i : alive(active)) {if (double_equal(responses[i], 0.0)) {zero.push_back(i);}}
    double newSearchAngleOffset = mp.coarse_search_angle_offset;
    for (uint32_t k = 0; k < 3 && !zero.empty(); ++k) {
      newSearchAngleOffset += 20 * kPi180;
      rc = run(zero, coarse(newSearchAngleOffset));
      if (rc) {return rc;}
      std::vector<int32_t> still;
      for (int32_t i : alive(zero)) {if (double_equal(responses[i], 0.0)) {still.push_back(i);}}
      zero.swap(still);
    }
  }
  // fine search, Mapper.cpp:621-629
  if (do_refine && !fine_done) {
    rc = run(alive(active), fine);
    if (rc) {return rc;}
  }
  int worst = KH_OK;
  for (int32_t i = 0; i < n; ++i) {
    if (status) {status[i] = st[i];}
    if (st[i] != KH_OK) {worst = st[i];}
  }
  return status ? KH_OK : worst;
}

extern "C" {

int kh_matcher_match_batch(kh_matcher * m, int32_t n, const kh_scan * queries, const kh_scan * base,
  const int32_t * base_begin, int32_t do_penalize, int32_t do_refine, double * means, double * covs,
  double * responses, int32_t * status)
{
  if (!m || n < 0 || n > m->max_batch || !queries || !base_begin || !means || !covs || !responses) {return KH_ERR_INVALID_ARG;}
  return match_batch(m, n, queries, base, base_begin, nullptr, do_penalize, do_refine, means, covs, responses, status);
}

int kh_matcher_match_map_batch(kh_matcher * m, int32_t n, const kh_scan * queries, const kh_map_view * map,
  int32_t do_penalize, int32_t do_refine, double * means, double * covs, double * responses, int32_t * status)
{
  if (!m || n < 0 || n > m->max_batch || !queries || !means || !covs || !responses || check_view(m, map) != KH_OK) {return KH_ERR_INVALID_ARG;}
  return match_batch(m, n, queries, nullptr, nullptr, map, do_penalize, do_refine, means, covs, responses, status);
}

int kh_matcher_match_map(kh_matcher * m, const kh_scan * query, const kh_map_view * map, int32_t do_penalize, int32_t do_refine,
  double mean[3], double cov[9], double * response)
{
  if (!m || !query || !mean || !cov || !response) {return KH_ERR_INVALID_ARG;}
  int32_t status = KH_OK;
  int rc = kh_matcher_match_map_batch(m, 1, query, map, do_penalize, do_refine, mean, cov, response, &status);
  if (rc) {return rc;}
  return status;
}

int kh_matcher_profile_map(kh_matcher * m, double * collect_ms, int64_t * collects)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (collect_ms) {*collect_ms = m->map_collect_ms;}
  if (collects) {*collects = m->map_collects;}
  m->map_collect_ms = 0; m->map_collects = 0;
  return KH_OK;
}

int kh_matcher_match(kh_matcher * m, const kh_scan * query, const kh_scan * base, int32_t n_base,
  int32_t do_penalize, int32_t do_refine, double mean[3], double cov[9], double * response)
{
  if (!m || !query || !mean || !cov || !response || n_base < 0) {return KH_ERR_INVALID_ARG;}
  const int32_t begin[2] = {0, n_base};
  int32_t status = KH_OK;
  int rc = kh_matcher_match_batch(m, 1, query, base, begin, do_penalize, do_refine, mean, cov, response, &status);
  if (rc) {return rc;}
  return status;
}

int kh_matcher_grid_info(kh_matcher * m, int32_t slot, kh_grid_info * out)
{
  if (!m || !out || slot < 0 || slot >= m->max_batch) {return KH_ERR_INVALID_ARG;}
  out->width = m->width; out->height = m->height; out->width_step = m->ws; out->data_size = m->data_size;
  out->roi_x = m->roi_x; out->roi_y = m->roi_y; out->roi_w = m->roi_w; out->roi_h = m->roi_h;
  out->kernel_size = m->kernel_size; out->search_side = m->side;
  out->offset_x = m->slots[slot].off_x; out->offset_y = m->slots[slot].off_y; out->scale = m->scale;
  return KH_OK;
}

int kh_matcher_read_grid(kh_matcher * m, int32_t slot, uint8_t * out)
{
  if (!m || !out || slot < 0 || slot >= m->max_batch) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  KH_HIP(hipStreamSynchronize(m->stream));
  KH_HIP(hipMemcpy(out, m->slots[slot].d_grid, static_cast<size_t>(m->data_size), hipMemcpyDeviceToHost));
  return KH_OK;
}

int kh_matcher_read_kernel(kh_matcher * m, uint8_t * out)
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  KH_HIP(hipMemcpy(out, m->d_kernel, m->kernel.size(), hipMemcpyDeviceToHost));
  return KH_OK;
}

int kh_matcher_read_lookup(kh_matcher * m, int32_t slot, int32_t * n_angles, int32_t * n_points, int32_t * out)
{
  if (!m || slot < 0 || slot >= m->max_batch || !n_angles || !n_points) {return KH_ERR_INVALID_ARG;}
  Slot & s = m->slots[slot];
  if (!s.has_last) {return KH_ERR_NOT_FOUND;}
  *n_angles = s.last.na; *n_points = s.last.P;
  if (out) {
    KH_HIP(hipSetDevice(m->device));
    KH_HIP(hipStreamSynchronize(m->stream));
    KH_HIP(hipMemcpy(out, s.d_table, sizeof(int32_t) * s.last.na * s.last.P, hipMemcpyDeviceToHost));
  }
  return KH_OK;
}

int kh_matcher_read_volume(kh_matcher * m, int32_t slot, int32_t * nx, int32_t * ny, int32_t * na,
  int32_t * out_sums, double * out_responses)
{
  if (!m || slot < 0 || slot >= m->max_batch || !nx || !ny || !na) {return KH_ERR_INVALID_ARG;}
  Slot & s = m->slots[slot];
  if (!s.has_last) {return KH_ERR_NOT_FOUND;}
  if (s.volume_stale) {set_error("the last search re-scored an off-lattice best pose: its volume was not kept"); return KH_ERR_NOT_FOUND;}
  const auto & c = s.last;
  *nx = c.nx; *ny = c.ny; *na = c.na;
  if (!out_sums && !out_responses) {return KH_OK;}
  KH_HIP(hipSetDevice(m->device));
  KH_HIP(hipStreamSynchronize(m->stream));
  const size_t plane = static_cast<size_t>(c.nx) * c.ny, vol = plane * c.na;
  if (out_sums) {
    std::vector<int32_t> tmp(vol);
    KH_HIP(hipMemcpy(tmp.data(), s.d_sums, vol * 4, hipMemcpyDeviceToHost));
    for (int32_t a = 0; a < c.na; ++a) {
      for (size_t p = 0; p < plane; ++p) {out_sums[p * c.na + a] = tmp[static_cast<size_t>(a) * plane + p];}
    }
  }
  if (out_responses) {
    if (!m->keep_responses || !s.d_resp) {set_error("response volume not kept: call kh_matcher_set_debug(m, 1) first"); return KH_ERR_NOT_FOUND;}
    std::vector<double> tmp(vol);
    KH_HIP(hipMemcpy(tmp.data(), s.d_resp, vol * 8, hipMemcpyDeviceToHost));
    for (int32_t a = 0; a < c.na; ++a) {
      for (size_t p = 0; p < plane; ++p) {out_responses[p * c.na + a] = tmp[static_cast<size_t>(a) * plane + p];}
    }
  }
  return KH_OK;
}

// m_pSearchSpaceProbs as the last COARSE CorrelateScan of `slot` left it: the lattice's cells only (ny rows of nx), from the host's
// copy -- no GPU work
int kh_matcher_read_search_probabilities(kh_matcher * m, int32_t slot, int32_t * nx, int32_t * ny, double * out)
{
  if (!m || slot < 0 || slot >= m->max_batch || !nx || !ny) {return KH_ERR_INVALID_ARG;}
  const Slot & s = m->slots[slot];
  if (!s.has_last_coarse) {set_error("no coarse search has run in this slot"); return KH_ERR_NOT_FOUND;}
  *nx = s.last_coarse.nx; *ny = s.last_coarse.ny;
  if (out) {std::copy(s.last_lattice.begin(), s.last_lattice.end(), out);}
  return KH_OK;
}

// ScanMatcher::ComputePositionalCovariance (Mapper.cpp:874-966) on the search-space probabilities the last COARSE
// CorrelateScan of `slot` left behind
int kh_matcher_positional_covariance(kh_matcher * m, int32_t slot, const double best_pose[3], double best_response,
  const double center[3], const double search_offset[2], const double search_resolution[2], double angle_resolution,
  double cov[9])
{
  if (!m || slot < 0 || slot >= m->max_batch || !best_pose || !center || !search_offset || !search_resolution || !cov) {return KH_ERR_INVALID_ARG;}
  if (!(search_resolution[0] > 0.0) || !(search_resolution[1] > 0.0)) {return KH_ERR_INVALID_ARG;}
  Slot & s = m->slots[slot];
  if (!s.has_last_coarse) {set_error("no coarse search has run in this slot"); return KH_ERR_NOT_FOUND;}
  WalkGeometry wg;
  std::copy(center, center + 3, wg.center);
  wg.off_x = search_offset[0]; wg.off_y = search_offset[1]; wg.res_x = search_resolution[0]; wg.res_y = search_resolution[1];
  wg.ang_res = angle_resolution;
  return positional_covariance(m->side, m->resolution, s.last_coarse, s.last_lattice.data(), wg, best_pose, best_response, cov);
}

// ScanMatcher::ComputeAngularCovariance (Mapper.cpp:977-1025): GetResponse of every search angle at the best pose's cell
// (one 1 x 1 search on the GPU against the grid currently in `slot`), then the reference's accumulation.  Only cov[8]
// (theta-theta) is written.
int kh_matcher_angular_covariance(kh_matcher * m, int32_t slot, const kh_scan * query, const double best_pose[3],
  double best_response, const double center[3], double angle_offset, double angle_resolution, double cov[9])
{
  if (!m || slot < 0 || slot >= m->max_batch || check_scan(query) != KH_OK || query->n == 0 || !best_pose || !center || !cov ||
    angle_resolution == 0.0) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  const double at[3] = {best_pose[0], best_pose[1], center[2]}, zero[2] = {0.0, 0.0};
  const double resolution[2] = {m->grid_resolution(), m->grid_resolution()};
  std::vector<CorrReq> reqs{CorrReq(slot, query, at, zero, resolution, angle_offset, angle_resolution, false, true)};
  int rc = correlate_batch(m, reqs);
  if (rc) {return rc;}
  Slot & s = m->slots[slot];
  const int32_t na = s.last.na;
  std::vector<int32_t> col(static_cast<size_t>(na));
  KH_HIP(hipMemcpy(col.data(), s.d_sums, sizeof(int32_t) * na, hipMemcpyDeviceToHost));
  const double bestAngle = normalize_angle_difference(best_pose[2], center[2]);
  cov[8] = angular_variance(col, s.last.denom, center[2], angle_offset, angle_resolution, bestAngle, best_response);
  return KH_OK;
}

int kh_matcher_seq_stats(kh_matcher * m, int64_t out[8])
{
  if (!m || !out) {return KH_ERR_INVALID_ARG;}
  const int64_t * v = seq_stats(m);
  std::copy(v, v + kSeqStatWords, out);
  return KH_OK;
}

void * kh_matcher_stream(kh_matcher * m) {return m ? reinterpret_cast<void *>(m->stream) : nullptr;}

int kh_matcher_profile(kh_matcher * m, int32_t enable, double * score_ms, int64_t * score_launches,
  double * raster_ms, int64_t * raster_launches)
{
  if (!m) {return KH_ERR_INVALID_ARG;}
  if (score_ms) {*score_ms = m->score_ms;}
  if (score_launches) {*score_launches = m->score_launches;}
  if (raster_ms) {*raster_ms = m->raster_ms;}
  if (raster_launches) {*raster_launches = m->raster_launches;}
  m->profiling = enable != 0;
  m->score_ms = 0; m->raster_ms = 0; m->score_launches = 0; m->raster_launches = 0; m->score_jobs = 0;
  return KH_OK;
}

int kh_matcher_profile_side(kh_matcher * m, double * offsets_ms, double * ties_ms)
{
  if (!m || !offsets_ms || !ties_ms) {return KH_ERR_INVALID_ARG;}
  *offsets_ms = m->offsets_ms; *ties_ms = m->ties_ms;
  m->offsets_ms = 0; m->ties_ms = 0;
  return KH_OK;
}

int kh_matcher_score_loads(kh_matcher * m, int64_t * wave_loads, int32_t reset)
{
  if (!m || !wave_loads) {return KH_ERR_INVALID_ARG;}
  KH_HIP(hipSetDevice(m->device));
  KH_HIP(hipStreamSynchronize(m->stream));
  for (auto & b : m->batch) {KH_HIP(hipStreamSynchronize(b.side));}
  unsigned long long v = 0;
  KH_HIP(hipMemcpy(&v, m->d_load_counter, 8, hipMemcpyDeviceToHost));
  *wave_loads = static_cast<int64_t>(v);
  if (reset) {KH_HIP(hipMemset(m->d_load_counter, 0, 512));}
  return KH_OK;
}

}  // extern "C"
