// Footprints on a map (kh_map_footprint_*): the handle owns the polygon, a snapshot of a distance field's
// cell states and d2 values over the field's window (copied on the device during create and recompute: the field is never borrowed)
// and the buffer of a call's tables and answers.  The kernels and their launchers are occupancy_footprint.hip's, the rules that need
// no device map_footprint_plan.hpp's.  A call computes its vertex cells (a check) or its stencil table (a layer) on the host -- libm
// stays there --, uploads them, launches and downloads once.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "map_field_update_plan.hpp"
#include "map_footprint_plan.hpp"
#include "occupancy_device.hpp"

using namespace kh;

struct kh_map_footprint
{
  int32_t n_vertices = 0, reach = 0, device = 0;
  double vertices[2 * kFootMaxVertices];
  FieldWindow f;                       // the snapshot: f.cells and f.d2 are the handle's own arrays of the field's stride, f.g is null
  DeviceWork work;                     // the stream, the events around a call's kernel, a call's tables and answers
  uint8_t * d_cells = nullptr;
  uint32_t * d_d2 = nullptr;
  int64_t cells = 0;                   // ws * height the two arrays were allocated for
  bool valid = false;                  // a snapshot stands
  kh_map_footprint_stats stats;
  FootJob job(uint32_t * error) const
  {
    FootJob j;
    j.f = f; j.n_vertices = n_vertices; j.reach = reach; j.error = error;
    return j;
  }
};

namespace
{
size_t up16(size_t bytes) {return (bytes + 15) / 16 * 16;}

int enter(kh_map_footprint * fp)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!fp) {return KH_ERR_INVALID_ARG;}
  return hipSetDevice(fp->device) == hipSuccess ? KH_OK : KH_ERR_HIP;
}

int failed(kh_map_footprint * fp, const char * who)
{
  (void)hipStreamSynchronize(fp->work.stream);
  set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return KH_ERR_HIP;
}

void free_snapshot(kh_map_footprint * fp)
{
  (void)hipFree(fp->d_cells); (void)hipFree(fp->d_d2);
  fp->d_cells = nullptr; fp->d_d2 = nullptr; fp->cells = 0;
}

// the field's cells and values as they stand; on a failure the handle holds no snapshot.  The arrays are kept where the window's
// strided size is the same, made anew where it changed.
int snapshot(kh_map_footprint * fp, const char * who, const kh_map_field * field)
{
  const auto t_begin = std::chrono::steady_clock::now();
  const FieldWindow f = map_field_window(field);
  if (f.width < 1 || f.height < 1 || !f.cells || !f.d2) {set_error(std::string(who) + ": the field has no window yet"); return KH_ERR_INVALID_ARG;}
  fp->valid = false;
  hipStream_t s = fp->work.stream;
  const int64_t cells = static_cast<int64_t>(f.ws) * f.height;
  if (cells != fp->cells) {
    (void)hipStreamSynchronize(s);
    free_snapshot(fp);
    if (hipMalloc(reinterpret_cast<void **>(&fp->d_cells), static_cast<size_t>(cells)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void **>(&fp->d_d2), static_cast<size_t>(cells) * sizeof(uint32_t)) != hipSuccess) {
      (void)hipGetLastError();
      free_snapshot(fp);
      set_error(std::string(who) + ": HIP allocation failed");
      return KH_ERR_HIP;
    }
    fp->cells = cells;
  }
  if (hipMemcpyAsync(fp->d_cells, f.cells, static_cast<size_t>(cells), hipMemcpyDeviceToDevice, s) != hipSuccess ||
    hipMemcpyAsync(fp->d_d2, f.d2, static_cast<size_t>(cells) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess ||
    hipStreamSynchronize(s) != hipSuccess) {return failed(fp, who);}
  fp->f = f;
  fp->f.cells = fp->d_cells; fp->f.d2 = fp->d_d2; fp->f.g = nullptr;
  kh_map_footprint_stats st;
  std::memset(&st, 0, sizeof(st));
  st.ox = f.ox; st.oy = f.oy; st.width = f.width; st.height = f.height; st.n_vertices = fp->n_vertices; st.reach = fp->reach;
  st.times_ms[2] = ms_since(t_begin);
  fp->stats = st;
  fp->valid = true;
  return KH_OK;
}

int no_snapshot(const char * who) {set_error(std::string(who) + ": the handle holds no snapshot (its last recompute failed)"); return KH_ERR_INVALID_ARG;}
int beyond_reach(const char * who) {set_error(std::string(who) + ": a vertex cell lies beyond the reach (the bound did not hold)"); return KH_ERR_HIP;}
}  // namespace

extern "C" {

int kh_map_footprint_create(kh_map_field * field, int32_t n_vertices, const double * vertices_xy, kh_map_footprint ** out)
{
  static const char * const who = "kh_map_footprint_create";
  if (out) {*out = nullptr;}
  static const char * const kWhy[] = {"", "", "n_vertices must lie in 3 .. 16", "a vertex is not finite", "the polygon is not strictly convex",
    "the polygon reaches beyond 255 cells: ceil(r_max * scale) + 1 > 255"};
  int32_t reach = 0;
  const int32_t bad = foot_create_check(field, n_vertices, vertices_xy, out, field ? map_field_window(field).scale : 1.0, &reach);
  if (bad != kFootOk) {
    if (bad != kFootNull) {set_error(std::string(who) + ": " + kWhy[bad]);}
    return KH_ERR_INVALID_ARG;
  }
  const int32_t device = map_field_device(field);
  if (require_device(0) != KH_OK || require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_map_footprint * fp = new kh_map_footprint();
  std::memset(&fp->stats, 0, sizeof(fp->stats));
  std::memset(&fp->f, 0, sizeof(fp->f));
  std::memset(fp->vertices, 0, sizeof(fp->vertices));
  std::memcpy(fp->vertices, vertices_xy, 2 * static_cast<size_t>(n_vertices) * sizeof(double));
  fp->n_vertices = n_vertices; fp->reach = reach; fp->device = device;
  const FieldWindow f = map_field_window(field);
  fp->f.ax = f.ax; fp->f.ay = f.ay; fp->f.scale = f.scale;
  if (!work_open(fp->work, device)) {
    (void)hipGetLastError();
    set_error(std::string(who) + ": HIP stream or event creation failed");
    kh_map_footprint_destroy(fp);
    return KH_ERR_HIP;
  }
  const int rc = snapshot(fp, who, field);
  if (rc) {kh_map_footprint_destroy(fp); return rc;}
  *out = fp;
  return KH_OK;
}

int kh_map_footprint_recompute(kh_map_footprint * fp, kh_map_field * field)
{
  if (!field) {return KH_ERR_INVALID_ARG;}
  if (fp) {
    static const char * const kOff[] = {"", "anchor x", "anchor y", "scale", "device"};
    const FieldWindow f = map_field_window(field);
    const double mine[2] = {fp->f.ax, fp->f.ay}, its[2] = {f.ax, f.ay};
    const int32_t off = lattice_check(mine, fp->f.scale, fp->device, its, f.scale, map_field_device(field));
    if (off != kLatticeSame) {
      set_error(std::string("kh_map_footprint_recompute: the field is not on the handle's lattice: its ") + kOff[off] + " differs");
      return KH_ERR_INVALID_ARG;
    }
  }
  const int rc = enter(fp);
  if (rc) {return rc;}
  return snapshot(fp, "kh_map_footprint_recompute", field);
}

void kh_map_footprint_destroy(kh_map_footprint * fp)
{
  if (!fp) {return;}
  (void)hipSetDevice(fp->device);
  if (fp->work.stream) {(void)hipStreamSynchronize(fp->work.stream);}
  free_snapshot(fp);
  work_close(fp->work);
  delete fp;
}

int kh_map_footprint_stats_get(kh_map_footprint * fp, kh_map_footprint_stats * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(fp);
  if (rc) {return rc;}
  if (!fp->valid) {return no_snapshot("kh_map_footprint_stats_get");}
  *out = fp->stats;
  return KH_OK;
}

int kh_map_footprint_check(kh_map_footprint * fp, int32_t n, const double * poses, kh_footprint_t * out)
{
  static const char * const who = "kh_map_footprint_check";
  int32_t bad_pose = -1;
  const int32_t bad = foot_check_check(n, poses, out, &bad_pose);
  if (bad != kFootCallOk) {
    if (bad == kFootCallCount) {set_error(std::string(who) + ": n must lie in 1 .. 65536");}
    if (bad == kFootCallPose) {set_error(std::string(who) + ": pose " + std::to_string(bad_pose) + " is not finite");}
    return KH_ERR_INVALID_ARG;
  }
  int rc = enter(fp);
  if (rc) {return rc;}
  if (!fp->valid) {return no_snapshot(who);}
  const auto t_begin = std::chrono::steady_clock::now();
  const size_t np = static_cast<size_t>(n);
  std::vector<FootPose> table(np);
  std::memset(table.data(), 0, np * sizeof(FootPose));
  for (size_t i = 0; i < np; ++i) {
    FootPose & p = table[i];
    int32_t own[2] = {0, 0};
    if (foot_pose_cells(fp->n_vertices, fp->vertices, poses + 3 * i, fp->f.ax, fp->f.ay, fp->f.scale, p.v, own)) {
      p.cx = own[0]; p.cy = own[1];
    } else {
      std::memset(&p, 0, sizeof(p));
      p.lattice = 1;
    }
  }
  // the error word and the records (downloaded together), the table
  const size_t record_bytes = np * sizeof(kh_footprint_t);
  Part parts[] = {{kZeros, 16}, {nullptr, record_bytes}, {table.data(), np * sizeof(FootPose)}};
  rc = work_stage(fp->work, who, "table", true, parts);
  if (rc) {return rc;}
  std::vector<uint8_t> answer(16 + record_bytes);
  const Part both{nullptr, answer.size(), parts[0].d};
  rc = work_run(fp->work, who, [&] {
    footprint_poses(fp->work.stream, fp->job(parts[0].as<uint32_t>()), n, parts[2].as<const FootPose>(), parts[1].as<kh_footprint_t>());
  }, &both, answer.data(), &fp->stats.times_ms[0]);
  if (rc) {return rc;}
  uint32_t error = 0u;
  std::memcpy(&error, answer.data(), sizeof(error));
  fp->stats.times_ms[2] = ms_since(t_begin);
  if (error != 0u) {return beyond_reach(who);}
  std::memcpy(out, answer.data() + 16, record_bytes);
  return KH_OK;
}

int kh_map_footprint_layer(kh_map_footprint * fp, int32_t n_headings, int32_t max_status, uint32_t * masks, kh_footprint_layer_t * summary)
{
  static const char * const who = "kh_map_footprint_layer";
  static const char * const kWhy[] = {"", "n_headings must lie in 1 .. 32", "max_status must lie in 0 .. 2",
    "the polygon reaches beyond 64 cells (KH_FOOTPRINT_LAYER_REACH): the tile and its halo would not fit in LDS"};
  const int32_t bad = foot_layer_check(n_headings, max_status, fp ? fp->reach : 0);
  if (bad != kFootLayerOk) {set_error(std::string(who) + ": " + kWhy[bad]); return KH_ERR_INVALID_ARG;}
  int rc = enter(fp);
  if (rc) {return rc;}
  if (!fp->valid) {return no_snapshot(who);}
  const auto t_begin = std::chrono::steady_clock::now();
  std::vector<int32_t> table;
  int32_t rows = 0;
  if (!foot_layer_table(fp->n_vertices, fp->vertices, n_headings, fp->f.scale, fp->reach, &table, &rows)) {return beyond_reach(who);}
  static_assert(sizeof(kh_footprint_layer_t) % 16 == 0, "the counters are a part of the call's buffer");
  const size_t mask_bytes = static_cast<size_t>(fp->f.width) * static_cast<size_t>(fp->f.height) * sizeof(uint32_t);
  Part parts[] = {{kZeros, sizeof(kh_footprint_layer_t)}, {table.data(), table.size() * sizeof(int32_t)}, {nullptr, masks ? up16(mask_bytes) : 0}};
  rc = work_stage(fp->work, who, "table", false, parts);
  if (rc) {return rc;}
  kh_footprint_layer_t sum;
  rc = work_run(fp->work, who, [&] {
    footprint_layer(fp->work.stream, fp->job(nullptr), n_headings, max_status, parts[1].as<const int32_t>(), masks ? parts[2].as<uint32_t>() : nullptr,
      parts[0].as<unsigned long long>());
  }, &parts[0], &sum, &fp->stats.times_ms[1]);
  if (rc) {return rc;}
  if (masks && (hipMemcpyAsync(masks, parts[2].d, mask_bytes, hipMemcpyDeviceToHost, fp->work.stream) != hipSuccess ||
    hipStreamSynchronize(fp->work.stream) != hipSuccess)) {return failed(fp, who);}
  if (summary) {*summary = sum;}
  fp->stats.layer_rows = rows; fp->stats.times_ms[2] = ms_since(t_begin);
  return KH_OK;
}

}  // extern "C"
