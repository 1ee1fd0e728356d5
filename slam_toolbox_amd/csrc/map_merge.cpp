// Two finished maps merged into one (kh_map_merge_*): the moving map warped through a rigid correction onto
// the target's lattice, the two composed cell by cell under a conflict policy, the overlap counted.  The handle owns the merged
// cells -- a kh_map_view of their own -- the codes and the statistics; the kernels and their launchers are occupancy_map.hip's, the
// rules that need no device map_merge_plan.hpp's.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>

#include "map_merge_plan.hpp"
#include "occupancy_device.hpp"

using namespace kh;

struct kh_map_merge
{
  kh_map_view view;                    // the merged map: the target's lattice, the output window, the handle's own cells
  DeviceWork work;                     // the stream, the events around a kernel, a call's tables and answers
  uint8_t * d_cells = nullptr;         // the merged cells ...
  uint8_t * d_codes = nullptr;         // ... and their KH_MERGED_ codes, both on the strided output window
  kh_map_merge_stats stats;
  size_t size() const {return static_cast<size_t>(view.width_step) * static_cast<size_t>(view.height);}
};

namespace
{
int failed(kh_map_merge * m, const char * who)
{
  (void)hipStreamSynchronize(m->work.stream);
  set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return KH_ERR_HIP;
}

// what every call on a handle begins with once its own arguments are judged: the device, then the handle
int enter(kh_map_merge * m)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!m) {return KH_ERR_INVALID_ARG;}
  return hipSetDevice(m->view.device) == hipSuccess ? KH_OK : KH_ERR_HIP;
}

// (1) the box of the moving map's known cells
int find_known_box(kh_map_merge * m, const kh_map_view & moving)
{
  const int32_t none[4] = {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN};
  Part parts[] = {{none, sizeof(none)}};
  int rc = work_stage(m->work, "kh_map_merge_create", "box", false, parts);
  if (rc) {return rc;}
  int32_t box[4];
  rc = work_run(m->work, "kh_map_merge_create", [&] {map_known_box(m->work.stream, moving, parts[0].as<int32_t>());}, &parts[0], box,
      &m->stats.times_ms[0]);
  if (rc) {return rc;}
  const bool any = box[2] >= box[0];
  for (int32_t k = 0; k < 4; ++k) {m->stats.known_box[k] = any ? box[k] : (k < 2 ? 0 : -1);}
  return KH_OK;
}

// (2) the output window, its buffers, the merge
int merge_into(kh_map_merge * m, const kh_map_view & target, const kh_map_view & moving, const kh_map_merge_params & p)
{
  MergeWindow w;
  switch (merge_window(target, moving, m->stats.known_box, p.correction, p.grow, &w)) {
    case kMergeCornerTooFar:
      set_error("kh_map_merge_create: the correction carries the moving map more than 2^30 cells from the target's anchor");
      return KH_ERR_INVALID_ARG;
    case kMergeSideTooLong:
      set_error("kh_map_merge_create: a side of the merged map would be longer than 32768 cells");
      return KH_ERR_INVALID_ARG;
    case kMergeTooManyCells:
      set_error("kh_map_merge_create: the merged map would hold more than 2^28 cells");
      return KH_ERR_INVALID_ARG;
    default:
      break;
  }
  m->view = target;
  m->view.device_cells = nullptr;
  m->view.ox = w.ox; m->view.oy = w.oy; m->view.width = w.width; m->view.height = w.height; m->view.width_step = w.ws;
  kh_map_merge_stats & st = m->stats;
  st.ox = w.ox; st.oy = w.oy; st.width = w.width; st.height = w.height; st.width_step = w.ws;
  st.footprint = p.footprint > 0 ? p.footprint : merge_default_footprint(moving.scale, target.scale);
  if (hipMalloc(reinterpret_cast<void **>(&m->d_cells), m->size()) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&m->d_codes), m->size()) != hipSuccess) {
    (void)hipGetLastError();
    set_error("kh_map_merge_create: HIP allocation failed");
    return KH_ERR_HIP;
  }
  m->view.device_cells = m->d_cells;
  const AlignRigid inv = align_inverse(AlignRigid(p.correction[0], p.correction[1], p.correction[2]));
  MergeJob job;
  job.target = window_of(target); job.moving = window_of(moving);
  job.ox = w.ox; job.oy = w.oy; job.width = w.width; job.height = w.height; job.ws = w.ws;
  job.footprint = st.footprint; job.conflict = p.conflict;
  job.c = inv.c; job.s = inv.s; job.tx = inv.x; job.ty = inv.y;
  merge_sample_offsets(st.footprint, target.scale, job.d);
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counters are downloaded as they lie");
  Part parts[] = {{kZeros, kMergeCounters * sizeof(unsigned long long)}};
  int rc = work_stage(m->work, "kh_map_merge_create", "counter", false, parts);
  if (rc) {return rc;}
  uint64_t counts[kMergeCounters];
  rc = work_run(m->work, "kh_map_merge_create", [&] {
    map_merge_cells(m->work.stream, job, m->d_cells, m->d_codes, parts[0].as<unsigned long long>());
  }, &parts[0], counts, &st.times_ms[1]);
  if (rc) {return rc;}
  st.target_only = counts[kMergeTargetOnly]; st.moving_only = counts[kMergeMovingOnly];
  st.agree_free = counts[kMergeAgreeFree]; st.agree_occupied = counts[kMergeAgreeOccupied];
  st.conflict_moving_occupied = counts[kMergeMovingOccupied]; st.conflict_moving_free = counts[kMergeMovingFree];
  st.overlap = merge_overlap(counts);
  st.agreement = merge_agreement(counts);
  return KH_OK;
}
}  // namespace

extern "C" {

void kh_map_merge_params_default(kh_map_merge_params * p)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  p->conflict = KH_MERGE_CONFLICT_OCCUPIED; p->grow = 1;
}

int kh_map_merge_create(const kh_map_view * target, const kh_map_view * moving, const kh_map_merge_params * params, kh_map_merge ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (!params || map_view_check(target) != KH_OK || map_view_check(moving) != KH_OK) {return KH_ERR_INVALID_ARG;}
  if (!merge_params_ok(*params)) {
    set_error("kh_map_merge_create: a finite correction, 0 <= footprint <= 4, 0 <= conflict <= 3 and 0 <= grow <= 1 are required");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (target->device != moving->device || target->device < 0) {
    set_error("kh_map_merge_create: the two views must lie on one device");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(target->device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  const auto t_begin = std::chrono::steady_clock::now();
  kh_map_merge * m = new kh_map_merge();
  std::memset(&m->stats, 0, sizeof(m->stats));
  m->view = *target;
  m->view.device_cells = nullptr;
  if (!work_open(m->work, target->device)) {
    (void)hipGetLastError();
    set_error("kh_map_merge_create: HIP stream / event creation failed");
    kh_map_merge_destroy(m);
    return KH_ERR_HIP;
  }
  int rc = find_known_box(m, *moving);
  if (rc == KH_OK) {rc = merge_into(m, *target, *moving, *params);}
  if (rc) {kh_map_merge_destroy(m); return rc;}
  m->stats.times_ms[2] = ms_since(t_begin);
  *out = m;
  return KH_OK;
}

void kh_map_merge_destroy(kh_map_merge * m)
{
  if (!m) {return;}
  (void)hipSetDevice(m->view.device);
  if (m->work.stream) {(void)hipStreamSynchronize(m->work.stream);}
  (void)hipFree(m->d_cells); (void)hipFree(m->d_codes);
  work_close(m->work);
  delete m;
}

int kh_map_merge_stats_get(kh_map_merge * m, kh_map_merge_stats * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(m);
  if (rc) {return rc;}
  *out = m->stats;
  return KH_OK;
}

int kh_map_merge_view(kh_map_merge * m, kh_map_view * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(m);
  if (rc) {return rc;}
  *out = m->view;
  return KH_OK;
}

int kh_map_merge_read(kh_map_merge * m, uint8_t * cells, uint8_t * codes)
{
  const int rc = enter(m);
  if (rc) {return rc;}
  if ((cells && hipMemcpyAsync(cells, m->d_cells, m->size(), hipMemcpyDeviceToHost, m->work.stream) != hipSuccess) ||
    (codes && hipMemcpyAsync(codes, m->d_codes, m->size(), hipMemcpyDeviceToHost, m->work.stream) != hipSuccess) ||
    hipStreamSynchronize(m->work.stream) != hipSuccess)
  {
    return failed(m, "kh_map_merge_read");
  }
  return KH_OK;
}

int kh_map_merge_read_nav(kh_map_merge * m, int8_t * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  int rc = enter(m);
  if (rc) {return rc;}
  const size_t total = static_cast<size_t>(m->view.width) * static_cast<size_t>(m->view.height);
  Part parts[] = {{nullptr, (total + 3) / 4 * 4}};           // (whole dwords are written ...
  rc = work_stage(m->work, "kh_map_merge_read_nav", "output", false, parts);
  if (rc) {return rc;}
  parts[0].bytes = total;                                     // ... and the values downloaded)
  return work_run(m->work, "kh_map_merge_read_nav", [&] {
    cells_to_nav(m->work.stream, m->d_cells, m->view.width, m->view.height, m->view.width_step, parts[0].as<uint32_t>());
  }, &parts[0], out, nullptr);
}

}  // extern "C"
