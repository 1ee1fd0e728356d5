// karto::OccupancyGrid::CreateFromScans on the GPU: the map that slam_toolbox
// publishes every map_update_interval and that "end-to-end map build" (BASELINE config[4]) ends with.
//
//   ComputeDimensions  Karto.h:6086-6112 (+ LocalizedRangeScan::Update's bounding box, Karto.h:5694-5700)
//   AddScan            Karto.h:6148-6189   RayTrace   Karto.h:6199-6232
//   Grid::TraceLine    Karto.h:4874-4927   Update / UpdateCell  Karto.h:6240-6274
//
// One thread per beam: the clip to the range threshold and both WorldToGrid roundings are the reference's
// IEEE operations (compiled without FMA contraction), the Bresenham walk is integer, and the pass / hit
// counters are uint32 atomics in L2 -- increments commute, so the counters, hence the cells, are bit-exact.
// This file: the whole-grid kernels, the nav conversions and the kh_occupancy handle.  What the kernels share with those of a live
// map (occupancy_live.hip), a map view (occupancy_map.hip) and a change layer (occupancy_changes.hip): occupancy_walk.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/karto_hip.h"
#include "occupancy_walk.hpp"

namespace kh
{
// AddScan + RayTrace of one beam into a whole grid: what the three kernels below do once a thread has found its beam and its gates
// (the inputs by reference: a kernel that passes fields of a record it fetched leaves the fetch of the fields a dropped beam never
// needs behind the drop test, as when the statements stood in the kernel itself)
__device__ __forceinline__ void occ_trace_beam(const OccDev & g, const double & r, double px, double py, const double & sx, const double & sy,
  const double & range_threshold, const double & min_range, const double & max_range)
{
  const Beam b = occ_gate(r, px, py, sx, sy, range_threshold, min_range, max_range);
  if (!b.kept) {return;}
  const int32_t x0 = occ_cell(sx, g.off_x, g.scale), y0 = occ_cell(sy, g.off_y, g.scale);
  const int32_t x1 = occ_cell(b.px, g.off_x, g.scale), y1 = occ_cell(b.py, g.off_y, g.scale);
  occ_walk(CountCells<OccDev>{g, 1u}, x0, y0, x1, y1, b.hit);
}

// beams: [n_beams] of (range, point x, point y, sensor x, sensor y) packed as 5 doubles
__global__ __launch_bounds__(256) void k_occ_trace(
  OccDev g, const double * __restrict__ beams, int64_t n_beams, double range_threshold, double min_range, double max_range)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_beams) {return;}
  occ_trace_beam(g, beams[5 * i], beams[5 * i + 1], beams[5 * i + 2], beams[5 * i + 3], beams[5 * i + 4], range_threshold, min_range, max_range);
}

// The same trace fed from a mapper's RESIDENT scans (kh_mapper_build_map): one ResidentScan per scan instead of 40 bytes per beam.
// One wave per run of 64 neighbouring beams of ONE scan (a workgroup = 4 such runs): the beams of a wave leave the same cell and
// fan out over neighbouring ones, so its atomics land in neighbouring L2 lines, and neighbouring beams have similar lengths, which
// bounds the divergence of the walk.
__global__ __launch_bounds__(256) void k_occ_trace_resident(
  OccDev g, const ResidentScan * __restrict__ scans, int32_t n_scans, int32_t n_beams, int32_t runs_per_scan, double range_threshold,
  double min_range, double max_range)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int32_t lane = threadIdx.x & 63;
  const int64_t s = wave / runs_per_scan;
  if (s >= n_scans) {return;}
  const int32_t i = (int32_t)(wave - s * runs_per_scan) * 64 + lane;
  if (i >= n_beams) {return;}
  const ResidentScan sc = scans[s];
  occ_trace_beam(g, sc.ranges[i], sc.points[2 * i], sc.points[2 * i + 1], sc.sx, sc.sy, range_threshold, min_range, max_range);
}

// The trace of a MERGE of mapping sessions (kh_merge_build): the scans of several mappers, each mapper (submap) placed by a rigid
// correction.  The resident readings stay as their mapper made them; the submap's correction is applied to the point in registers
// -- x' = (c x - s y) + tx, y' = (s x + c y) + ty, no contraction -- and nothing transformed is written back.  The sensor position
// arrives transformed (the host does GetSensorAt of the transformed corrected pose, once per scan).
// The same work layout as k_occ_trace_resident.  Submaps may have different lasers: the grid is dealt max_runs waves per scan
// (the longest laser's), a wave beyond its scan's own beam count leaves at once.
__global__ __launch_bounds__(256) void k_occ_trace_merged(
  OccDev g, const MergeScan * __restrict__ scans, const MergeSubmap * __restrict__ submaps, int32_t n_scans, int32_t max_runs)
{
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int32_t lane = threadIdx.x & 63;
  const int64_t s = wave / max_runs;
  if (s >= n_scans) {return;}
  const MergeScan sc = scans[s];
  const MergeSubmap sm = submaps[sc.submap];
  const int32_t i = (int32_t)(wave - s * max_runs) * 64 + lane;
  if (i >= sm.n_beams) {return;}
  const double ux = sc.points[2 * i], uy = sc.points[2 * i + 1];
  const double px = (sm.c * ux - sm.s * uy) + sm.tx, py = (sm.s * ux + sm.c * uy) + sm.ty;
  occ_trace_beam(g, sc.ranges[i], px, py, sc.sx, sc.sy, sm.range_threshold, sm.min_range, sm.max_range);
}

// The FIT of candidate corrections of one submap against a finished grid (kh_merge_fit): k_occ_trace_merged's work layout times the
// candidates -- one wave per (candidate, scan, run of 64 beams) -- and its arithmetic, but the walk looks up the state of every
// cell it would have incremented and counts, per state, visits and hits in six registers of the lane (FitCells).  The grid is only
// read.  A workgroup holds waves of ONE candidate (blocks_per_candidate = ceil(n_scans * runs_per_scan / 4)), so its sums go to one
// row of `out` (fit_reduce).  A wave past the last scan and a lane past the beam count take part in the reduction with zeros:
// every wave reaches the barrier.  A candidate may put the submap anywhere, so the walk stands behind walk_bounded as on a map view
// (the host has refused what it would stop: merge_fit_check, map_localize_plan.hpp); a beam it stops counts nothing.
__global__ __launch_bounds__(256) void k_occ_fit_merged(
  OccDev g, const ResidentScan * __restrict__ scans, const FitCandidate * __restrict__ candidates, const FitSensor * __restrict__ sensors,
  int32_t n_scans, int32_t n_beams, int32_t runs_per_scan, int32_t blocks_per_candidate, double range_threshold, double min_range,
  double max_range, unsigned long long * __restrict__ out)
{
  const PoseWave w = pose_wave(blocks_per_candidate);
  const int32_t candidate = w.pose, lane = threadIdx.x & 63;
  const int64_t s = w.wave / runs_per_scan;
  const int32_t i = (int32_t)(w.wave - s * runs_per_scan) * 64 + lane;
  FitCounts n;
  if (s < n_scans && i < n_beams) {
    const ResidentScan sc = scans[s];
    const FitCandidate t = candidates[candidate];
    const FitSensor sensor = sensors[(int64_t)candidate * n_scans + s];
    const double ux = sc.points[2 * i], uy = sc.points[2 * i + 1];
    const double px = (t.c * ux - t.s * uy) + t.tx, py = (t.s * ux + t.c * uy) + t.ty;
    const Beam b = occ_gate(sc.ranges[i], px, py, sensor.sx, sensor.sy, range_threshold, min_range, max_range);
    if (b.kept) {
      const int32_t x0 = occ_cell(sensor.sx, g.off_x, g.scale), y0 = occ_cell(sensor.sy, g.off_y, g.scale);
      const int32_t x1 = occ_cell(b.px, g.off_x, g.scale), y1 = occ_cell(b.py, g.off_y, g.scale);
      if (walk_bounded(x0, y0, x1, y1)) {occ_walk(FitCells<OccDev>{g, n}, x0, y0, x1, y1, b.hit);}
    }
  }
  fit_reduce(n, out, candidate);
}

__global__ __launch_bounds__(256) void k_occ_update(OccDev g, uint32_t min_pass, double threshold)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)g.ws * g.height) {return;}
  occ_update_cell(g.pass, g.hits, g.cells, k, min_pass, threshold);
}

// toNavMap of a whole grid (kh_occupancy_read_nav): from the ws-strided cells into a DENSE width x height array, so that an output
// dword may span rows (any width, width < 4 too).  One thread per output dword; the bytes past `total` of the last one are padding
// of the buffer.
__global__ __launch_bounds__(256) void k_occ_to_nav(const uint8_t * __restrict__ cells, int32_t width, int32_t ws, int64_t total,
  uint32_t * __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t k = 4 * i;
  if (k >= total) {return;}
  int64_t y = k / width;
  int32_t x = (int32_t)(k - y * width);
  uint32_t v = 0;
  for (int32_t b = 0; b < 4 && k + b < total; ++b) {
    v |= (uint32_t)cells[x + y * ws] << (8 * b);
    if (++x == width) {x = 0; ++y;}
  }
  out[i] = occ_nav4(v);
}

// The inverse of k_occ_to_nav (kh_occupancy_write_nav): from a DENSE width x height array of nav values into the ws-strided cells,
// -1 -> 0 (unknown), 100 -> 100 (occupied), 0 -> 255 (free); the host has refused every other value.  One thread per dword of the
// cells (ws is a multiple of 8); the bytes of the row padding are written as 0.
__global__ __launch_bounds__(256) void k_nav_to_occ(const int8_t * __restrict__ nav, int32_t width, int32_t ws, int64_t words,
  uint32_t * __restrict__ cells)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words) {return;}
  const int32_t words_per_row = ws >> 2;
  const int64_t y = i / words_per_row;
  const int32_t x = 4 * (int32_t)(i - y * words_per_row);
  uint32_t v = 0;
  for (int32_t b = 0; b < 4 && x + b < width; ++b) {
    const int32_t n = nav[y * width + x + b];
    v |= (n == 100 ? 100u : n == 0 ? 255u : 0u) << (8 * b);
  }
  cells[i] = v;
}
}  // namespace kh

using namespace kh;

struct kh_occupancy
{
  DeviceWork work;                                            // the stream of the grid's kernels; the tables, beams or nav values of one call
  OccDev dev;
  double * h_beams = nullptr; size_t cap_hbeams = 0;          // kh_occupancy_add_scans' staging in pinned host memory (capacity in doubles)
  double trace_ms = 0.0; int64_t beams_traced = 0;
};

namespace kh
{
namespace
{
// What every AddScan route ends with: the trace kernel between two events, the wait for it, a failure reported under the caller's
// (`who`) name, the grid's trace time and beam counter.
template <typename Launch>
int timed_trace(kh_occupancy * g, const char * who, int64_t n_beams, Launch launch)
{
  double ms = 0.0;
  const int rc = work_run(g->work, who, launch, nullptr, nullptr, &ms);
  if (rc) {return rc;}
  g->trace_ms += ms; g->beams_traced += n_beams;
  return KH_OK;
}

// what a call on a grid that has nothing to trace returns: the stream's state
int drained(kh_occupancy * g) {return hipStreamSynchronize(g->work.stream) == hipSuccess ? KH_OK : KH_ERR_HIP;}
}  // namespace

void * occupancy_stream(kh_occupancy * g) {return g ? g->work.stream : nullptr;}

int occupancy_add_resident(kh_occupancy * g, int32_t n_scans, const ResidentScan * scans, int32_t n_beams, double range_threshold,
  double min_range, double max_range)
{
  if (!g || n_scans < 0 || n_beams < 0 || (n_scans > 0 && !scans)) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  if (n_scans == 0 || n_beams == 0) {return drained(g);}
  Part parts[] = {{scans, static_cast<size_t>(n_scans) * sizeof(ResidentScan)}};
  const int rc = work_stage(g->work, "kh_mapper_build_map", "scan table", true, parts);
  if (rc) {return rc;}
  const int32_t runs = (n_beams + 63) / 64;
  return timed_trace(g, "kh_mapper_build_map", static_cast<int64_t>(n_scans) * n_beams, [&] {
    hipLaunchKernelGGL(k_occ_trace_resident, dim3(blocks_of_runs(n_scans, runs)), dim3(256), 0, g->work.stream, g->dev, parts[0].as<const ResidentScan>(),
      n_scans, n_beams, runs, range_threshold, min_range, max_range);
  });
}

int occupancy_add_merged(kh_occupancy * g, int32_t n_scans, const MergeScan * scans, int32_t n_submaps, const MergeSubmap * submaps,
  int32_t max_beams, int64_t n_total_beams)
{
  if (!g || n_scans < 0 || n_submaps < 0 || max_beams < 0 || (n_scans > 0 && (!scans || !submaps || n_submaps == 0))) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  if (n_scans == 0 || max_beams == 0) {return drained(g);}
  // the submaps, then the scans (64 * n_submaps: 8-byte aligned)
  Part parts[] = {{submaps, static_cast<size_t>(n_submaps) * sizeof(MergeSubmap)}, {scans, static_cast<size_t>(n_scans) * sizeof(MergeScan)}};
  const int rc = work_stage(g->work, "kh_merge_build", "table", false, parts);
  if (rc) {return rc;}
  const int32_t runs = (max_beams + 63) / 64;
  return timed_trace(g, "kh_merge_build", n_total_beams, [&] {
    hipLaunchKernelGGL(k_occ_trace_merged, dim3(blocks_of_runs(n_scans, runs)), dim3(256), 0, g->work.stream, g->dev, parts[1].as<const MergeScan>(),
      parts[0].as<const MergeSubmap>(), n_scans, runs);
  });
}

int occupancy_fit_merged(kh_occupancy * g, int32_t n_candidates, const FitCandidate * candidates, const FitSensor * sensors, int32_t n_scans,
  const ResidentScan * scans, int32_t n_beams, double range_threshold, double min_range, double max_range, uint64_t * out, double * kernel_ms)
{
  if (!g || n_candidates < 1 || !candidates || !out || n_scans < 0 || n_beams < 0 || (n_scans > 0 && (!scans || !sensors))) {return KH_ERR_INVALID_ARG;}
  if (kernel_ms) {*kernel_ms = 0.0;}
  std::fill(out, out + static_cast<size_t>(n_candidates) * kFitCounters, uint64_t{0});
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  if (n_scans == 0 || n_beams == 0) {return drained(g);}
  const int32_t runs = (n_beams + 63) / 64;
  const int64_t blocks_per_candidate = (static_cast<int64_t>(n_scans) * runs + 3) / 4;
  if (blocks_per_candidate * n_candidates > INT32_MAX) {set_error("kh_merge_fit: too many candidates for one launch"); return KH_ERR_INVALID_ARG;}
  // the sums first, then the tables: every part a multiple of 8 bytes
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the sums are downloaded as they lie");
  const size_t nc = static_cast<size_t>(n_candidates), ns = static_cast<size_t>(n_scans);
  Part parts[] = {{kZeros, nc * kFitCounters * sizeof(unsigned long long)}, {candidates, nc * sizeof(FitCandidate)},
    {sensors, nc * ns * sizeof(FitSensor)}, {scans, ns * sizeof(ResidentScan)}};
  const int rc = work_stage(g->work, "kh_merge_fit", "table", false, parts);
  if (rc) {return rc;}
  return work_run(g->work, "kh_merge_fit", [&] {
    hipLaunchKernelGGL(k_occ_fit_merged, dim3(static_cast<unsigned>(blocks_per_candidate * n_candidates)), dim3(256), 0, g->work.stream, g->dev,
      parts[3].as<const ResidentScan>(), parts[1].as<const FitCandidate>(), parts[2].as<const FitSensor>(), n_scans, n_beams, runs,
      static_cast<int32_t>(blocks_per_candidate), range_threshold, min_range, max_range, parts[0].as<unsigned long long>());
  }, &parts[0], out, kernel_ms);
}

void cells_to_nav(void * stream, const uint8_t * d_cells, int32_t width, int32_t height, int32_t ws, uint32_t * d_out)
{
  const int64_t total = static_cast<int64_t>(width) * height, words = (total + 3) / 4;
  hipLaunchKernelGGL(k_occ_to_nav, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_cells, width,
    ws, total, d_out);
}
}  // namespace kh

extern "C" {

int kh_occupancy_compute_dimensions(
  int32_t n_scans, const kh_scan * scans, double min_range, double range_threshold, double resolution,
  int32_t * width, int32_t * height, double offset[2])
{
  if (n_scans <= 0 || !scans || !width || !height || !offset || !(resolution > 0)) {return KH_ERR_INVALID_ARG;}
  // BoundingBox2 (Karto.h:2846-2903) over every scan's box = sensor position + in-range points (Karto.h:5694-5700)
  Box box;
  for (int32_t s = 0; s < n_scans; ++s) {
    if (scans[s].n < 0 || (scans[s].n > 0 && (!scans[s].ranges || !scans[s].points_xy))) {return KH_ERR_INVALID_ARG;}
    box.add(scans[s].sensor_pose[0], scans[s].sensor_pose[1]);
    for (int32_t i = 0; i < scans[s].n; ++i) {
      const double r = scans[s].ranges[i];
      if (r >= min_range && r <= range_threshold) {box.add(scans[s].points_xy[2 * i], scans[s].points_xy[2 * i + 1]);}   // math::InRange
    }
  }
  grid_dimensions(box, resolution, width, height, offset);
  return KH_OK;
}

int kh_occupancy_create(int32_t width, int32_t height, double offset_x, double offset_y, double resolution,
  int32_t device, kh_occupancy ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  if (width <= 0 || height <= 0 || !(resolution > 0) || grid_too_large(width, height)) {
    set_error("OccupancyGrid: invalid dimensions");
    return KH_ERR_INVALID_ARG;
  }
  if (require_device(device) != KH_OK) {return KH_ERR_NO_DEVICE;}
  kh_occupancy * g = new kh_occupancy();
  g->dev.width = width; g->dev.height = height; g->dev.ws = (width + 7) & ~7;      // Karto.h:4640
  g->dev.off_x = offset_x; g->dev.off_y = offset_y; g->dev.scale = 1.0 / resolution;
  g->dev.pass = nullptr; g->dev.hits = nullptr; g->dev.cells = nullptr;
  const size_t size = static_cast<size_t>(g->dev.ws) * height;
  if (!work_open(g->work, device) ||
    hipMalloc(reinterpret_cast<void **>(&g->dev.pass), size * 4) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&g->dev.hits), size * 4) != hipSuccess ||
    hipMalloc(reinterpret_cast<void **>(&g->dev.cells), size) != hipSuccess || kh_occupancy_clear(g) != KH_OK)    // (zeros, on the grid's own stream)
  {
    set_error("kh_occupancy_create: HIP allocation failed");
    kh_occupancy_destroy(g);
    return KH_ERR_HIP;
  }
  *out = g;
  return KH_OK;
}

void kh_occupancy_destroy(kh_occupancy * g)
{
  if (!g) {return;}
  (void)hipSetDevice(g->work.device);
  if (g->work.stream) {(void)hipStreamSynchronize(g->work.stream);}
  (void)hipFree(g->dev.pass); (void)hipFree(g->dev.hits); (void)hipFree(g->dev.cells);
  if (g->h_beams) {(void)hipHostFree(g->h_beams);}
  work_close(g->work);
  delete g;
}

int kh_occupancy_clear(kh_occupancy * g)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t size = static_cast<size_t>(g->dev.ws) * g->dev.height;
  if (hipMemsetAsync(g->dev.pass, 0, size * 4, g->work.stream) != hipSuccess || hipMemsetAsync(g->dev.hits, 0, size * 4, g->work.stream) != hipSuccess ||
    hipMemsetAsync(g->dev.cells, 0, size, g->work.stream) != hipSuccess || hipStreamSynchronize(g->work.stream) != hipSuccess) {return KH_ERR_HIP;}
  return KH_OK;
}

int kh_occupancy_add_scans(kh_occupancy * g, int32_t n_scans, const kh_scan * scans, double range_threshold,
  double min_range, double max_range)
{
  if (!g || n_scans < 0 || (n_scans > 0 && !scans)) {return KH_ERR_INVALID_ARG;}
  if (n_scans == 0) {return KH_OK;}
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  size_t total = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    if (scans[s].n < 0 || (scans[s].n > 0 && (!scans[s].ranges || !scans[s].points_xy))) {return KH_ERR_INVALID_ARG;}
    total += static_cast<size_t>(scans[s].n);
  }
  if (total == 0) {return KH_OK;}
  if (total * 5 > g->cap_hbeams) {
    if (g->h_beams) {(void)hipStreamSynchronize(g->work.stream); (void)hipHostFree(g->h_beams); g->h_beams = nullptr;}
    const size_t cap = std::max(total * 5, g->cap_hbeams + g->cap_hbeams / 2);
    g->cap_hbeams = 0;
    if (hipHostMalloc(reinterpret_cast<void **>(&g->h_beams), cap * 8, hipHostMallocDefault) != hipSuccess) {
      set_error("kh_occupancy_add_scans: staging allocation failed");
      return KH_ERR_HIP;
    }
    g->cap_hbeams = cap;
  }
  size_t k = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    const double sx = scans[s].sensor_pose[0], sy = scans[s].sensor_pose[1];
    for (int32_t i = 0; i < scans[s].n; ++i, ++k) {
      double * b = g->h_beams + 5 * k;
      b[0] = scans[s].ranges[i]; b[1] = scans[s].points_xy[2 * i]; b[2] = scans[s].points_xy[2 * i + 1]; b[3] = sx; b[4] = sy;
    }
  }
  Part parts[] = {{g->h_beams, total * 5 * 8}};
  const int rc = work_stage(g->work, "kh_occupancy_add_scans", "staging", true, parts);
  if (rc) {return rc;}
  return timed_trace(g, "kh_occupancy_add_scans", static_cast<int64_t>(total), [&] {
    hipLaunchKernelGGL(k_occ_trace, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, g->work.stream, g->dev, parts[0].as<const double>(),
      static_cast<int64_t>(total), range_threshold, min_range, max_range);
  });
}

int kh_occupancy_update(kh_occupancy * g, uint32_t min_pass_through, double occupancy_threshold)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  const int64_t size = static_cast<int64_t>(g->dev.ws) * g->dev.height;
  hipLaunchKernelGGL(k_occ_update, dim3(static_cast<unsigned>((size + 255) / 256)), dim3(256), 0, g->work.stream, g->dev,
    min_pass_through, occupancy_threshold);
  if (hipStreamSynchronize(g->work.stream) != hipSuccess) {return KH_ERR_HIP;}
  return KH_OK;
}

int kh_occupancy_read(kh_occupancy * g, uint8_t * cells, uint32_t * pass, uint32_t * hits)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t size = static_cast<size_t>(g->dev.ws) * g->dev.height;
  if (cells && hipMemcpy(cells, g->dev.cells, size, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  if (pass && hipMemcpy(pass, g->dev.pass, size * 4, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  if (hits && hipMemcpy(hits, g->dev.hits, size * 4, hipMemcpyDeviceToHost) != hipSuccess) {return KH_ERR_HIP;}
  return KH_OK;
}

int kh_occupancy_read_nav(kh_occupancy * g, int8_t * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  const size_t total = static_cast<size_t>(g->dev.width) * g->dev.height;
  Part parts[] = {{nullptr, (total + 3) / 4 * 4}};           // (whole dwords are written ...
  const int rc = work_stage(g->work, "kh_occupancy_read_nav", "output", false, parts);
  if (rc) {return rc;}
  parts[0].bytes = total;                                     // ... and the values downloaded)
  return work_run(g->work, "kh_occupancy_read_nav", [&] {
    cells_to_nav(g->work.stream, g->dev.cells, g->dev.width, g->dev.height, g->dev.ws, parts[0].as<uint32_t>());
  }, &parts[0], out, nullptr);
}

int kh_occupancy_info(kh_occupancy * g, int32_t * width, int32_t * height, int32_t * width_step, double * trace_ms, int64_t * beams)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (width) {*width = g->dev.width;}
  if (height) {*height = g->dev.height;}
  if (width_step) {*width_step = g->dev.ws;}
  if (trace_ms) {*trace_ms = g->trace_ms;}
  if (beams) {*beams = g->beams_traced;}
  return KH_OK;
}

int kh_occupancy_geometry(kh_occupancy * g, double offset[2], double * resolution)
{
  if (!g) {return KH_ERR_INVALID_ARG;}
  if (offset) {offset[0] = g->dev.off_x; offset[1] = g->dev.off_y;}
  if (resolution) {*resolution = 1.0 / g->dev.scale;}
  return KH_OK;
}

int kh_occupancy_view(kh_occupancy * g, kh_map_view * out)
{
  if (!g || !out) {return KH_ERR_INVALID_ARG;}
  out->device_cells = g->dev.cells; out->device = g->work.device;
  out->width = g->dev.width; out->height = g->dev.height; out->width_step = g->dev.ws;
  out->ox = 0; out->oy = 0;
  out->anchor[0] = g->dev.off_x; out->anchor[1] = g->dev.off_y; out->scale = g->dev.scale;
  return KH_OK;
}

int kh_occupancy_write_nav(kh_occupancy * g, const int8_t * nav)
{
  if (!g || !nav) {return KH_ERR_INVALID_ARG;}
  const int64_t total = static_cast<int64_t>(g->dev.width) * g->dev.height;
  for (int64_t i = 0; i < total; ++i) {
    if (nav[i] != -1 && nav[i] != 0 && nav[i] != 100) {
      set_error("kh_occupancy_write_nav: value " + std::to_string(nav[i]) + " at " + std::to_string(i) + " is none of -1, 0, 100");
      return KH_ERR_INVALID_ARG;
    }
  }
  if (hipSetDevice(g->work.device) != hipSuccess) {return KH_ERR_HIP;}
  Part parts[] = {{nav, static_cast<size_t>(total)}};
  const int rc = work_stage(g->work, "kh_occupancy_write_nav", "input", false, parts);
  if (rc) {return rc;}
  const size_t size = static_cast<size_t>(g->dev.ws) * g->dev.height;
  const int64_t words = static_cast<int64_t>(size / 4);
  hipLaunchKernelGGL(k_nav_to_occ, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, g->work.stream, parts[0].as<const int8_t>(),
    g->dev.width, g->dev.ws, words, reinterpret_cast<uint32_t *>(g->dev.cells));
  // (the stream is drained before returning: `nav` is the caller's pageable memory)
  if (hipMemsetAsync(g->dev.pass, 0, size * 4, g->work.stream) != hipSuccess || hipMemsetAsync(g->dev.hits, 0, size * 4, g->work.stream) != hipSuccess ||
    hipStreamSynchronize(g->work.stream) != hipSuccess)
  {
    set_error(std::string("kh_occupancy_write_nav: ") + hipGetErrorString(hipGetLastError()));
    return KH_ERR_HIP;
  }
  return KH_OK;
}

}  // extern "C"

