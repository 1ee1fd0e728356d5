// Map regions (kh_map_regions_*): the handle owns the label, count and record arrays of the two sets -- the
// traversable regions and the frontier clusters of a distance field's window -- and the last analysis' records and summary on the
// host.  It reads the field's arrays during create and recompute only and never borrows the field.  The kernels and their launchers
// are occupancy_regions.hip's, the rules that need no device map_regions_plan.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "map_field_update_plan.hpp"
#include "map_regions_plan.hpp"
#include "occupancy_device.hpp"

using namespace kh;

struct kh_map_regions
{
  kh_map_regions_params params;
  int32_t rc = 0, device = 0;
  FieldWindow f;                       // the analysed window and its lattice; the field's arrays are not kept (nullptr between calls)
  DeviceWork work;                     // the stream, the events around a stage, a lookup's tables and answers
  uint32_t * d_label[2] = {nullptr, nullptr};
  uint32_t * d_count[2] = {nullptr, nullptr};
  RegionRecord * d_records[2] = {nullptr, nullptr};
  int32_t * d_unit = nullptr;
  unsigned long long * d_counters = nullptr;
  int64_t cells = 0;                   // what the window-sized arrays were allocated for
  bool valid = false;                  // an analysis stands
  kh_map_regions_stats stats;
  std::vector<kh_region> records[2];
  uint32_t maximum(int32_t which) const {return static_cast<uint32_t>(which == KH_REGIONS ? params.max_regions : params.max_frontiers);}
  uint32_t minimum(int32_t which) const {return static_cast<uint32_t>(which == KH_REGIONS ? params.min_region_cells : params.min_frontier_cells);}
};

namespace
{
int enter(kh_map_regions * r)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!r) {return KH_ERR_INVALID_ARG;}
  return hipSetDevice(r->device) == hipSuccess ? KH_OK : KH_ERR_HIP;
}

int failed(kh_map_regions * r, const char * who)
{
  (void)hipStreamSynchronize(r->work.stream);
  set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return KH_ERR_HIP;
}

void free_window_arrays(kh_map_regions * r)
{
  for (int32_t w = 0; w < 2; ++w) {
    (void)hipFree(r->d_label[w]); (void)hipFree(r->d_count[w]);
    r->d_label[w] = r->d_count[w] = nullptr;
  }
  (void)hipFree(r->d_unit);
  r->d_unit = nullptr;
  r->cells = 0;
}

// the window-sized arrays for `cells` cells: kept where the count is the same, made anew where the window changed
int layout(kh_map_regions * r, const char * who, int32_t width, int32_t height)
{
  const int64_t cells = static_cast<int64_t>(width) * height;
  if (cells == r->cells) {return KH_OK;}
  (void)hipStreamSynchronize(r->work.stream);
  free_window_arrays(r);
  const size_t bytes = static_cast<size_t>(cells) * sizeof(uint32_t);
  bool ok = hipMalloc(reinterpret_cast<void **>(&r->d_unit), (static_cast<size_t>(region_grid(width, height).units) + 1) * sizeof(int32_t)) == hipSuccess;
  for (int32_t w = 0; w < 2; ++w) {
    ok = ok && hipMalloc(reinterpret_cast<void **>(&r->d_label[w]), bytes) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&r->d_count[w]), bytes) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    free_window_arrays(r);
    set_error(std::string(who) + ": HIP allocation failed");
    return KH_ERR_HIP;
  }
  r->cells = cells;
  return KH_OK;
}

kh_region record_out(const RegionRecord & d, const FieldWindow & f)
{
  kh_region o;
  std::memset(&o, 0, sizeof(o));
  o.root = d.root; o.n_cells = d.n_cells;
  o.box[0] = d.x0 + f.ox; o.box[1] = d.y0 + f.oy; o.box[2] = d.x1 - d.x0 + 1; o.box[3] = d.y1 - d.y0 + 1;
  o.sum_i = d.sum_i; o.sum_j = d.sum_j;
  o.max_d2 = d.max_d2; o.n_other = d.n_other; o.link = d.link;
  o.anchor_cell = static_cast<uint32_t>(d.anchor_key & 0xFFFFFFFFull);
  o.centroid[0] = region_centroid(f.ax, f.ox, d.sum_i, d.n_cells, f.scale);
  o.centroid[1] = region_centroid(f.ay, f.oy, d.sum_j, d.n_cells, f.scale);
  o.anchor_xy[0] = region_cell_world(f.ax, f.ox, static_cast<int32_t>(o.anchor_cell % static_cast<uint32_t>(f.width)), f.scale);
  o.anchor_xy[1] = region_cell_world(f.ay, f.oy, static_cast<int32_t>(o.anchor_cell / static_cast<uint32_t>(f.width)), f.scale);
  return o;
}

// the whole analysis of the field as it stands; on a failure the handle holds none
int analyse(kh_map_regions * r, const char * who, const kh_map_field * field)
{
  const auto t_begin = std::chrono::steady_clock::now();
  const FieldWindow f = map_field_window(field);
  if (f.width < 1 || f.height < 1 || !f.cells || !f.d2) {set_error(std::string(who) + ": the field has no window yet"); return KH_ERR_INVALID_ARG;}
  if (!regions_reach_ok(f.radius, r->rc)) {
    set_error(std::string(who) + ": the field reaches " + std::to_string(f.radius) + " cells, the clearance asks for " + std::to_string(r->rc));
    return KH_ERR_INVALID_ARG;
  }
  r->valid = false;
  int rc = layout(r, who, f.width, f.height);
  if (rc) {return rc;}
  hipStream_t s = r->work.stream;
  const size_t bytes = static_cast<size_t>(r->cells) * sizeof(uint32_t);
  if (hipMemsetAsync(r->d_count[0], 0, bytes, s) != hipSuccess || hipMemsetAsync(r->d_count[1], 0, bytes, s) != hipSuccess ||
    hipMemsetAsync(r->d_counters, 0, kRegionCounters * sizeof(unsigned long long), s) != hipSuccess) {return failed(r, who);}
  RegionJob job;
  job.f = f;
  for (int32_t w = 0; w < 2; ++w) {job.set[w] = RegionSet{r->d_label[w], r->d_count[w], r->d_records[w], r->minimum(w), r->maximum(w)};}
  job.rc2 = static_cast<uint32_t>(r->rc) * static_cast<uint32_t>(r->rc);
  job.conn8 = r->params.connectivity == 8 ? 1 : 0;
  job.unit = r->d_unit; job.counters = r->d_counters;
  kh_map_regions_stats st;
  std::memset(&st, 0, sizeof(st));
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counters are downloaded as they lie");
  uint64_t counters[kRegionCounters] = {0};
  const Part answer{nullptr, sizeof(counters), reinterpret_cast<uint8_t *>(r->d_counters)};
  rc = work_run(r->work, who, [&] {region_tiles(s, job);}, nullptr, nullptr, &st.times_ms[0]);
  if (rc == KH_OK) {rc = work_run(r->work, who, [&] {region_seams(s, job);}, nullptr, nullptr, &st.times_ms[1]);}
  if (rc == KH_OK) {rc = work_run(r->work, who, [&] {region_flatten(s, job);}, nullptr, nullptr, &st.times_ms[2]);}
  if (rc == KH_OK) {rc = work_run(r->work, who, [&] {region_compact(s, job);}, nullptr, nullptr, &st.times_ms[3]);}
  if (rc == KH_OK) {rc = work_run(r->work, who, [&] {region_records(s, job);}, nullptr, nullptr, &st.times_ms[4]);}
  if (rc == KH_OK) {rc = work_run(r->work, who, [&] {region_anchors(s, job);}, &answer, counters, &st.times_ms[5]);}
  if (rc) {return rc;}
  if (counters[kRegionError] != 0) {set_error(std::string(who) + ": a label walk did not end (watchdog)"); return KH_ERR_HIP;}
  std::vector<RegionRecord> raw;
  for (int32_t w = 0; w < 2; ++w) {
    const uint64_t passing = counters[kRegionPassing + w], kept = std::min<uint64_t>(passing, r->maximum(w));
    st.n_total[w] = static_cast<uint32_t>(counters[kRegionTotal + w]); st.n_kept[w] = static_cast<uint32_t>(kept); st.truncated[w] = passing > kept ? 1 : 0;
    raw.resize(static_cast<size_t>(kept));
    if (kept > 0 && (hipMemcpyAsync(raw.data(), r->d_records[w], raw.size() * sizeof(RegionRecord), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)) {return failed(r, who);}
    r->records[w].resize(raw.size());
    for (size_t k = 0; k < raw.size(); ++k) {r->records[w][k] = record_out(raw[k], f);}
  }
  st.ox = f.ox; st.oy = f.oy; st.width = f.width; st.height = f.height; st.clearance_cells = r->rc; st.connectivity = r->params.connectivity;
  st.n_traversable = counters[kRegionTraversable]; st.n_frontier_cells = counters[kRegionFrontierCells];
  r->f = f;
  r->f.cells = nullptr; r->f.g = nullptr; r->f.d2 = nullptr;
  st.times_ms[6] = ms_since(t_begin);
  r->stats = st;
  r->valid = true;
  return KH_OK;
}

int no_analysis(const char * who) {set_error(std::string(who) + ": the handle holds no analysis (its last recompute failed)"); return KH_ERR_INVALID_ARG;}
}  // namespace

extern "C" {

void kh_map_regions_params_default(kh_map_regions_params * p)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  p->min_clearance = 0.0; p->connectivity = 8;
  p->min_region_cells = 1; p->max_regions = 4096; p->min_frontier_cells = 1; p->max_frontiers = 4096;
}

int kh_map_regions_create(kh_map_field * field, const kh_map_regions_params * params, kh_map_regions ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (!field || !params) {return KH_ERR_INVALID_ARG;}
  const FieldWindow f = map_field_window(field);
  int32_t rc_cells = 0;
  static const char * const kWhy[] = {"", "min_clearance must be finite and >= 0", "the clearance lies above 1024 cells", "connectivity must be 4 or 8",
    "a minimum must be >= 1", "a maximum must lie in 1 .. 2^20"};
  const int32_t bad = regions_check(*params, f.scale, &rc_cells);
  if (bad != kRegionsOk) {set_error(std::string("kh_map_regions_create: ") + kWhy[bad]); return KH_ERR_INVALID_ARG;}
  const int32_t device = map_field_device(field);
  if (require_device(0) != KH_OK || require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_map_regions * r = new kh_map_regions();
  std::memset(&r->stats, 0, sizeof(r->stats));
  std::memset(&r->f, 0, sizeof(r->f));
  r->params = *params; r->rc = rc_cells; r->device = device;
  r->f.ax = f.ax; r->f.ay = f.ay; r->f.scale = f.scale;
  bool ok = work_open(r->work, device) && hipMalloc(reinterpret_cast<void **>(&r->d_counters), kRegionCounters * sizeof(unsigned long long)) == hipSuccess;
  for (int32_t w = 0; w < 2; ++w) {ok = ok && hipMalloc(reinterpret_cast<void **>(&r->d_records[w]), r->maximum(w) * sizeof(RegionRecord)) == hipSuccess;}
  if (!ok) {
    (void)hipGetLastError();
    set_error("kh_map_regions_create: HIP stream, event or record allocation failed");
    kh_map_regions_destroy(r);
    return KH_ERR_HIP;
  }
  const int rc = analyse(r, "kh_map_regions_create", field);
  if (rc) {kh_map_regions_destroy(r); return rc;}
  *out = r;
  return KH_OK;
}

int kh_map_regions_recompute(kh_map_regions * r, kh_map_field * field)
{
  if (!field) {return KH_ERR_INVALID_ARG;}
  if (r) {
    static const char * const kOff[] = {"", "anchor x", "anchor y", "scale", "device"};
    const FieldWindow f = map_field_window(field);
    const double mine[2] = {r->f.ax, r->f.ay}, its[2] = {f.ax, f.ay};
    const int32_t off = lattice_check(mine, r->f.scale, r->device, its, f.scale, map_field_device(field));
    if (off != kLatticeSame) {
      set_error(std::string("kh_map_regions_recompute: the field is not on the handle's lattice: its ") + kOff[off] + " differs");
      return KH_ERR_INVALID_ARG;
    }
  }
  const int rc = enter(r);
  if (rc) {return rc;}
  return analyse(r, "kh_map_regions_recompute", field);
}

void kh_map_regions_destroy(kh_map_regions * r)
{
  if (!r) {return;}
  (void)hipSetDevice(r->device);
  if (r->work.stream) {(void)hipStreamSynchronize(r->work.stream);}
  free_window_arrays(r);
  (void)hipFree(r->d_records[0]); (void)hipFree(r->d_records[1]); (void)hipFree(r->d_counters);
  work_close(r->work);
  delete r;
}

int kh_map_regions_stats_get(kh_map_regions * r, kh_map_regions_stats * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(r);
  if (rc) {return rc;}
  if (!r->valid) {return no_analysis("kh_map_regions_stats_get");}
  *out = r->stats;
  return KH_OK;
}

int kh_map_regions_read(kh_map_regions * r, int32_t which, uint32_t * ids)
{
  if (!ids || which < KH_REGIONS || which > KH_FRONTIERS) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(r);
  if (rc) {return rc;}
  if (!r->valid) {return no_analysis("kh_map_regions_read");}
  if (hipMemcpyAsync(ids, r->d_label[which], static_cast<size_t>(r->cells) * sizeof(uint32_t), hipMemcpyDeviceToHost, r->work.stream) != hipSuccess ||
    hipStreamSynchronize(r->work.stream) != hipSuccess) {return failed(r, "kh_map_regions_read");}
  return KH_OK;
}

int kh_map_regions_get(kh_map_regions * r, int32_t which, kh_region * records, int32_t cap, int32_t * n)
{
  if (which < KH_REGIONS || which > KH_FRONTIERS || !n || cap < 0 || (cap > 0 && !records)) {return KH_ERR_INVALID_ARG;}
  *n = 0;
  const int rc = enter(r);
  if (rc) {return rc;}
  if (!r->valid) {return no_analysis("kh_map_regions_get");}
  const std::vector<kh_region> & have = r->records[which];
  *n = static_cast<int32_t>(have.size());
  const size_t take = std::min<size_t>(have.size(), static_cast<size_t>(cap));
  if (take > 0) {std::memcpy(records, have.data(), take * sizeof(kh_region));}
  return KH_OK;
}

int kh_map_regions_lookup(kh_map_regions * r, int32_t n, const double * xy, int32_t * status, uint32_t * id)
{
  if (n < 1 || !xy) {return KH_ERR_INVALID_ARG;}
  for (int64_t k = 0; k < 2 * static_cast<int64_t>(n); ++k) {
    if (!std::isfinite(xy[k])) {set_error("kh_map_regions_lookup: point " + std::to_string(k / 2) + " is not finite"); return KH_ERR_INVALID_ARG;}
  }
  int rc = enter(r);
  if (rc) {return rc;}
  if (!r->valid) {return no_analysis("kh_map_regions_lookup");}
  const size_t np = static_cast<size_t>(n), words = (np + 1) / 2 * 2;                 // every part a multiple of 8 bytes
  Part parts[] = {{nullptr, 2 * words * sizeof(uint32_t)}, {xy, np * 2 * sizeof(double)}};
  rc = work_stage(r->work, "kh_map_regions_lookup", "table", true, parts);
  if (rc) {return rc;}
  std::vector<uint32_t> answer(2 * words);
  rc = work_run(r->work, "kh_map_regions_lookup", [&] {
    region_lookup(r->work.stream, r->f, r->d_label[KH_REGIONS], n, parts[1].as<const double>(), parts[0].as<uint32_t>(), parts[0].as<int32_t>() + words);
  }, &parts[0], answer.data(), nullptr);
  if (rc) {return rc;}
  for (size_t k = 0; k < np; ++k) {
    if (id) {id[k] = answer[k];}
    if (status) {status[k] = static_cast<int32_t>(answer[words + k]);}
  }
  return KH_OK;
}

}  // extern "C"
