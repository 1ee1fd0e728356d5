// Travel costs on a map (kh_map_travel_*): the handle owns the weights and the values of a distance field's
// window, the tile flags of the relaxation and the counters.  It reads the field's arrays during create and recompute only and never
// borrows the field.  The kernels and their launchers are occupancy_travel.hip's, the rules that need no device
// map_travel_plan.hpp's.  The host loop of a solve: launches of k_travel_relax in batches of rounds_per_check, one read of the
// "anything flagged" words per batch, until the last launch of a batch flagged nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "map_field_update_plan.hpp"
#include "map_travel_plan.hpp"
#include "occupancy_device.hpp"

using namespace kh;

namespace
{
// what a batch leaves for the host, as it lies on the device: the counters, then one "this launch flagged a tile" word per launch
struct TravelWords
{
  unsigned long long counters[kTravelCounters];
  uint32_t any[kMaxRoundsPerCheck];
};
}  // namespace

struct kh_map_travel
{
  kh_map_travel_params params;
  int32_t rc = 0, rt = 0, device = 0;
  FieldWindow f;                       // the snapshot's window and its lattice; the field's arrays are not kept (nullptr between calls)
  DeviceWork work;                     // the stream, the events around a stage, a call's tables and answers
  uint16_t * d_q = nullptr;
  uint32_t * d_v = nullptr;
  uint32_t * d_flags = nullptr;
  TravelWords * d_words = nullptr;
  int32_t * d_paths = nullptr; size_t paths_cap = 0;       // the cells of the last kh_map_travel_paths (bytes)
  int64_t cells = 0, tiles = 0;        // what the window-sized arrays were allocated for
  int32_t rounds_per_check = 0;        // 0: kDefaultRoundsPerCheck
  bool valid = false, solved = false;  // a snapshot stands; a solution stands
  kh_map_travel_stats stats;
  TravelJob job() const
  {
    TravelJob j;
    j.f = f; j.q = d_q; j.v = d_v; j.conn8 = params.connectivity == 8 ? 1 : 0; j.cut_corners = params.cut_corners; j.flags = d_flags;
    j.counters = d_words->counters;
    return j;
  }
};

namespace
{
int enter(kh_map_travel * t)
{
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!t) {return KH_ERR_INVALID_ARG;}
  return hipSetDevice(t->device) == hipSuccess ? KH_OK : KH_ERR_HIP;
}

int failed(kh_map_travel * t, const char * who)
{
  (void)hipStreamSynchronize(t->work.stream);
  set_error(std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return KH_ERR_HIP;
}

void free_window_arrays(kh_map_travel * t)
{
  (void)hipFree(t->d_q); (void)hipFree(t->d_v); (void)hipFree(t->d_flags);
  t->d_q = nullptr; t->d_v = nullptr; t->d_flags = nullptr;
  t->cells = 0; t->tiles = 0;
}

// the window-sized arrays: kept where the cell and the tile count are the same, made anew where the window changed
int layout(kh_map_travel * t, const char * who, int32_t width, int32_t height)
{
  const int64_t cells = static_cast<int64_t>(width) * height, tiles = travel_grid(width, height).tiles;
  if (cells == t->cells && tiles == t->tiles) {return KH_OK;}
  (void)hipStreamSynchronize(t->work.stream);
  free_window_arrays(t);
  if (hipMalloc(reinterpret_cast<void **>(&t->d_q), static_cast<size_t>(cells) * sizeof(uint16_t)) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&t->d_v), static_cast<size_t>(cells) * sizeof(uint32_t)) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&t->d_flags), 2 * static_cast<size_t>(tiles) * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    free_window_arrays(t);
    set_error(std::string(who) + ": HIP allocation failed");
    return KH_ERR_HIP;
  }
  t->cells = cells; t->tiles = tiles;
  return KH_OK;
}

bool download_words(kh_map_travel * t, TravelWords * out)
{
  return hipMemcpyAsync(out, t->d_words, sizeof(TravelWords), hipMemcpyDeviceToHost, t->work.stream) == hipSuccess &&
         hipStreamSynchronize(t->work.stream) == hipSuccess;
}

// the weights of the field as it stands; on a failure the handle holds no snapshot
int snapshot(kh_map_travel * t, const char * who, const kh_map_field * field)
{
  const auto t_begin = std::chrono::steady_clock::now();
  const FieldWindow f = map_field_window(field);
  if (f.width < 1 || f.height < 1 || !f.cells || !f.d2) {set_error(std::string(who) + ": the field has no window yet"); return KH_ERR_INVALID_ARG;}
  static const char * const kWhy[] = {"", "the field does not reach as far as the clearance asks", "the field does not reach as far as the inflation radius",
    "width * height * Lmax * q_max lies above 0xFFFFFFFE: the values of this window could overflow"};
  const int32_t bad = travel_field_check(t->params, t->rc, t->rt, f.radius, f.width, f.height);
  if (bad != kTravelFieldOk) {set_error(std::string(who) + ": " + kWhy[bad]); return KH_ERR_INVALID_ARG;}
  t->valid = false; t->solved = false;
  int rc = layout(t, who, f.width, f.height);
  if (rc) {return rc;}
  const bool weighted = t->params.cost_weight > 0;
  std::vector<uint8_t> table = weighted ? inflation_table(t->params.inflation, f.scale, t->rt) : std::vector<uint8_t>();
  table.resize((table.size() + 16) / 16 * 16, 0);
  Part parts[] = {{table.data(), table.size()}};
  rc = work_stage(t->work, who, "table", false, parts);
  if (rc) {return rc;}
  hipStream_t s = t->work.stream;
  if (hipMemsetAsync(t->d_words, 0, sizeof(TravelWords), s) != hipSuccess) {return failed(t, who);}
  t->f = f;
  TravelWords words;
  const Part answer{nullptr, sizeof(TravelWords), reinterpret_cast<uint8_t *>(t->d_words)};
  kh_map_travel_stats st;
  std::memset(&st, 0, sizeof(st));
  const uint32_t rc2 = static_cast<uint32_t>(t->rc) * static_cast<uint32_t>(t->rc), rt2 = static_cast<uint32_t>(t->rt) * static_cast<uint32_t>(t->rt);
  rc = work_run(t->work, who, [&] {
    travel_weights(s, t->job(), rc2, weighted ? parts[0].as<const uint8_t>() : nullptr, rt2, static_cast<uint32_t>(t->params.neutral_cost),
      static_cast<uint32_t>(t->params.cost_weight));
  }, &answer, &words, &st.times_ms[0]);
  t->f.cells = nullptr; t->f.g = nullptr; t->f.d2 = nullptr;
  if (rc) {return rc;}
  st.ox = f.ox; st.oy = f.oy; st.width = f.width; st.height = f.height; st.clearance_cells = t->rc; st.inflation_cells = t->rt;
  st.connectivity = t->params.connectivity; st.n_traversable = words.counters[kTravelTraversable];
  st.times_ms[3] = ms_since(t_begin);
  t->stats = st;
  t->valid = true;
  return KH_OK;
}

int no_snapshot(const char * who) {set_error(std::string(who) + ": the handle holds no snapshot (its last recompute failed)"); return KH_ERR_INVALID_ARG;}
int no_solution(const char * who) {set_error(std::string(who) + ": no solve since the last snapshot"); return KH_ERR_NOT_FOUND;}

int points_check(const char * who, int32_t n, const double * xy)
{
  if (n < 1 || !xy) {return KH_ERR_INVALID_ARG;}
  for (int64_t k = 0; k < 2 * static_cast<int64_t>(n); ++k) {
    if (!std::isfinite(xy[k])) {set_error(std::string(who) + ": point " + std::to_string(k / 2) + " is not finite"); return KH_ERR_INVALID_ARG;}
  }
  return KH_OK;
}
}  // namespace

extern "C" {

void kh_map_travel_params_default(kh_map_travel_params * p)
{
  if (!p) {return;}
  std::memset(p, 0, sizeof(*p));
  kh_inflation_params_default(&p->inflation);
  p->min_clearance = 0.0; p->connectivity = 8; p->cut_corners = 0; p->neutral_cost = 50; p->cost_weight = 13; p->goal_snap_cells = 0;
}

int kh_map_travel_create(kh_map_field * field, const kh_map_travel_params * params, kh_map_travel ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (!field || !params) {return KH_ERR_INVALID_ARG;}
  const FieldWindow f = map_field_window(field);
  int32_t rc_cells = 0, rt_cells = 0;
  static const char * const kWhy[] = {"", "connectivity must be 4 or 8", "cut_corners must be 0 or 1", "neutral_cost must lie in 1 .. 255",
    "cost_weight must lie in 0 .. 255", "goal_snap_cells must lie in 0 .. 16", "min_clearance must be finite and >= 0", "the clearance lies above 1024 cells",
    "finite radii and factor >= 0, inscribed <= inflation <= 1024 cells and flags 0 / 1 are required of the inflation parameters"};
  const int32_t bad = travel_check(*params, f.scale, &rc_cells, &rt_cells);
  if (bad != kTravelOk) {set_error(std::string("kh_map_travel_create: ") + kWhy[bad]); return KH_ERR_INVALID_ARG;}
  const int32_t device = map_field_device(field);
  if (require_device(0) != KH_OK || require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_map_travel * t = new kh_map_travel();
  std::memset(&t->stats, 0, sizeof(t->stats));
  std::memset(&t->f, 0, sizeof(t->f));
  t->params = *params; t->rc = rc_cells; t->rt = rt_cells; t->device = device;
  t->f.ax = f.ax; t->f.ay = f.ay; t->f.scale = f.scale;
  if (!(work_open(t->work, device) && hipMalloc(reinterpret_cast<void **>(&t->d_words), sizeof(TravelWords)) == hipSuccess)) {
    (void)hipGetLastError();
    set_error("kh_map_travel_create: HIP stream, event or counter allocation failed");
    kh_map_travel_destroy(t);
    return KH_ERR_HIP;
  }
  const int rc = snapshot(t, "kh_map_travel_create", field);
  if (rc) {kh_map_travel_destroy(t); return rc;}
  *out = t;
  return KH_OK;
}

int kh_map_travel_recompute(kh_map_travel * t, kh_map_field * field)
{
  if (!field) {return KH_ERR_INVALID_ARG;}
  if (t) {
    static const char * const kOff[] = {"", "anchor x", "anchor y", "scale", "device"};
    const FieldWindow f = map_field_window(field);
    const double mine[2] = {t->f.ax, t->f.ay}, its[2] = {f.ax, f.ay};
    const int32_t off = lattice_check(mine, t->f.scale, t->device, its, f.scale, map_field_device(field));
    if (off != kLatticeSame) {
      set_error(std::string("kh_map_travel_recompute: the field is not on the handle's lattice: its ") + kOff[off] + " differs");
      return KH_ERR_INVALID_ARG;
    }
  }
  const int rc = enter(t);
  if (rc) {return rc;}
  return snapshot(t, "kh_map_travel_recompute", field);
}

void kh_map_travel_destroy(kh_map_travel * t)
{
  if (!t) {return;}
  (void)hipSetDevice(t->device);
  if (t->work.stream) {(void)hipStreamSynchronize(t->work.stream);}
  free_window_arrays(t);
  (void)hipFree(t->d_words); (void)hipFree(t->d_paths);
  work_close(t->work);
  delete t;
}

int kh_map_travel_set_rounds_per_check(kh_map_travel * t, int32_t k)
{
  if (k < 0 || k > kMaxRoundsPerCheck) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(t);
  if (rc) {return rc;}
  t->rounds_per_check = k;
  return KH_OK;
}

int kh_map_travel_solve(kh_map_travel * t, int32_t n_goals, const double * goals_xy, int32_t * goal_status)
{
  static const char * const who = "kh_map_travel_solve";
  if (n_goals > kMaxTravelGoals) {return KH_ERR_INVALID_ARG;}
  int rc = points_check(who, n_goals, goals_xy);
  if (rc) {return rc;}
  if ((rc = enter(t)) != KH_OK) {return rc;}
  if (!t->valid) {return no_snapshot(who);}
  const auto t_begin = std::chrono::steady_clock::now();
  t->solved = false;
  const size_t n = static_cast<size_t>(n_goals), words = (n + 3) / 4 * 4;            // every part a multiple of 16 bytes
  Part parts[] = {{nullptr, 2 * words * sizeof(uint32_t)}, {goals_xy, n * 2 * sizeof(double)}};
  rc = work_stage(t->work, who, "goal", true, parts);
  if (rc) {return rc;}
  hipStream_t s = t->work.stream;
  if (hipMemsetAsync(t->d_v, 0xFF, static_cast<size_t>(t->cells) * sizeof(uint32_t), s) != hipSuccess ||
    hipMemsetAsync(t->d_flags, 0, 2 * static_cast<size_t>(t->tiles) * sizeof(uint32_t), s) != hipSuccess ||
    hipMemsetAsync(t->d_words, 0, sizeof(TravelWords), s) != hipSuccess) {return failed(t, who);}
  const TravelJob job = t->job();
  kh_map_travel_stats st = t->stats;
  st.n_reached = 0; st.max_value = 0; st.rounds = 0; st.launches = 0; st.tile_runs = 0; st.times_ms[1] = st.times_ms[2] = 0.0;
  std::vector<uint32_t> answer(2 * words);
  rc = work_run(t->work, who, [&] {
    travel_goals(s, job, n_goals, parts[1].as<const double>(), t->params.goal_snap_cells, parts[0].as<int32_t>(), parts[0].as<uint32_t>() + words);
  }, &parts[0], answer.data(), &st.times_ms[1]);
  if (rc) {return rc;}
  bool pending = false;                                      // the next launch has a tile to run
  for (size_t k = 0; k < n; ++k) {
    if (goal_status) {goal_status[k] = static_cast<int32_t>(answer[k]);}
    pending = pending || static_cast<int32_t>(answer[k]) == KH_TRAVEL_GOAL_OK;
  }
  // The relaxation.  A best path crosses fewer tile borders than the window has cells and every round carries every value across
  // one more border: round cells + 1 runs no tile in a correct solve.
  const int32_t batch = t->rounds_per_check > 0 ? t->rounds_per_check : kDefaultRoundsPerCheck;
  const uint64_t round_limit = static_cast<uint64_t>(t->cells) + 1;
  TravelWords words_now;
  std::memset(&words_now, 0, sizeof(words_now));
  const Part all{nullptr, sizeof(TravelWords), reinterpret_cast<uint8_t *>(t->d_words)};
  while (pending) {
    if (st.rounds >= round_limit) {set_error(std::string(who) + ": the relaxation did not end (round watchdog)"); return KH_ERR_HIP;}
    double ms = 0.0;
    rc = work_run(t->work, who, [&] {
      (void)hipMemsetAsync(t->d_words->any, 0, sizeof(words_now.any), s);
      for (int32_t b = 0; b < batch; ++b) {travel_relax(s, job, st.launches + static_cast<uint32_t>(b), t->d_words->any + b);}
    }, &all, &words_now, &ms);
    if (rc) {return rc;}
    st.times_ms[2] += ms;
    for (int32_t b = 0; b < batch; ++b) {
      st.rounds += pending ? 1u : 0u;
      pending = words_now.any[b] != 0u;
    }
    st.launches += static_cast<uint32_t>(batch);
    if (words_now.counters[kTravelError] != 0) {set_error(std::string(who) + ": a tile's relaxation did not end (watchdog)"); return KH_ERR_HIP;}
  }
  rc = work_run(t->work, who, [&] {travel_count(s, job);}, &all, &words_now, nullptr);
  if (rc) {return rc;}
  st.n_reached = words_now.counters[kTravelReached]; st.max_value = static_cast<uint32_t>(words_now.counters[kTravelMaxValue]);
  st.tile_runs = words_now.counters[kTravelRuns];
  st.times_ms[3] = ms_since(t_begin);
  t->stats = st;
  t->solved = true;
  return KH_OK;
}

int kh_map_travel_stats_get(kh_map_travel * t, kh_map_travel_stats * out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  const int rc = enter(t);
  if (rc) {return rc;}
  if (!t->valid) {return no_snapshot("kh_map_travel_stats_get");}
  *out = t->stats;
  return KH_OK;
}

int kh_map_travel_read(kh_map_travel * t, uint32_t * values, uint16_t * weights)
{
  const int rc = enter(t);
  if (rc) {return rc;}
  if (!t->solved) {return no_solution("kh_map_travel_read");}
  hipStream_t s = t->work.stream;
  const size_t cells = static_cast<size_t>(t->cells);
  if ((values && hipMemcpyAsync(values, t->d_v, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess) ||
    (weights && hipMemcpyAsync(weights, t->d_q, cells * sizeof(uint16_t), hipMemcpyDeviceToHost, s) != hipSuccess) ||
    hipStreamSynchronize(s) != hipSuccess) {return failed(t, "kh_map_travel_read");}
  return KH_OK;
}

int kh_map_travel_lookup(kh_map_travel * t, int32_t n, const double * xy, int32_t snap_cells, int32_t * status, uint32_t * value, int32_t * cell)
{
  static const char * const who = "kh_map_travel_lookup";
  int rc = points_check(who, n, xy);
  if (rc) {return rc;}
  if (!travel_snap_ok(snap_cells)) {return KH_ERR_INVALID_ARG;}
  if ((rc = enter(t)) != KH_OK) {return rc;}
  if (!t->solved) {return no_solution(who);}
  const size_t np = static_cast<size_t>(n);
  Part parts[] = {{nullptr, np * sizeof(TravelAt)}, {xy, np * 2 * sizeof(double)}};
  rc = work_stage(t->work, who, "table", true, parts);
  if (rc) {return rc;}
  std::vector<TravelAt> answer(np);
  rc = work_run(t->work, who, [&] {
    travel_lookup(t->work.stream, t->job(), n, parts[1].as<const double>(), snap_cells, parts[0].as<TravelAt>());
  }, &parts[0], answer.data(), nullptr);
  if (rc) {return rc;}
  for (size_t k = 0; k < np; ++k) {
    if (status) {status[k] = answer[k].status;}
    if (value) {value[k] = answer[k].value;}
    if (cell) {cell[2 * k] = answer[k].x; cell[2 * k + 1] = answer[k].y;}
  }
  return KH_OK;
}

int kh_map_travel_paths(kh_map_travel * t, int32_t n, const double * starts_xy, int32_t snap_cells, int32_t max_cells, kh_travel_path * heads, int32_t * cells)
{
  static const char * const who = "kh_map_travel_paths";
  int rc = points_check(who, n, starts_xy);
  if (rc) {return rc;}
  if (!travel_snap_ok(snap_cells) || !heads) {return KH_ERR_INVALID_ARG;}
  if (!travel_path_buffer_ok(n, max_cells)) {set_error(std::string(who) + ": max_cells must lie in 1 .. 65536 and n * max_cells below 2^24"); return KH_ERR_INVALID_ARG;}
  if ((rc = enter(t)) != KH_OK) {return rc;}
  if (!t->solved) {return no_solution(who);}
  const size_t np = static_cast<size_t>(n), bytes = 2 * np * static_cast<size_t>(max_cells) * sizeof(int32_t);
  hipStream_t s = t->work.stream;
  if (cells) {
    if (!grow_device(s, reinterpret_cast<void **>(&t->d_paths), &t->paths_cap, bytes, bytes)) {set_error(std::string(who) + ": path allocation failed"); return KH_ERR_HIP;}
    if (hipMemsetAsync(t->d_paths, 0, bytes, s) != hipSuccess) {return failed(t, who);}
  }
  Part parts[] = {{nullptr, np * sizeof(TravelHead)}, {starts_xy, np * 2 * sizeof(double)}};
  rc = work_stage(t->work, who, "table", true, parts);
  if (rc) {return rc;}
  if (hipMemsetAsync(&t->d_words->counters[kTravelError], 0, sizeof(unsigned long long), s) != hipSuccess) {return failed(t, who);}
  static_assert(sizeof(TravelHead) == sizeof(kh_travel_path), "the heads are downloaded as they lie");
  rc = work_run(t->work, who, [&] {
    travel_paths(s, t->job(), n, parts[1].as<const double>(), snap_cells, max_cells, parts[0].as<TravelHead>(), cells ? t->d_paths : nullptr);
  }, &parts[0], heads, nullptr);
  if (rc) {return rc;}
  TravelWords words;
  if ((cells && hipMemcpyAsync(cells, t->d_paths, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) || !download_words(t, &words)) {return failed(t, who);}
  if (words.counters[kTravelError] != 0) {set_error(std::string(who) + ": a walk found no neighbour that explains its cell's value"); return KH_ERR_HIP;}
  return KH_OK;
}

}  // extern "C"
