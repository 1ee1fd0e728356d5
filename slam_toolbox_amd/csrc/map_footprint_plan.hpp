// The rules of kh_map_footprint_*  that need no device: strict convexity, the reach of a polygon, every
// refusal and their order, the vertex cells of a pose, the vertex offsets of a heading, and the one statement of "covered" -- the
// row spans of the outline that the vertex cells make -- which the pose kernel, the layer's stencil table and
// tests/map_footprint_plan_check.cpp all run.  Needs no HIP header.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "occupancy_device.hpp"      // round_half_away, RayWalk, KH_HOST_DEVICE

namespace kh
{
constexpr int32_t kFootMinVertices = 3, kFootMaxVertices = 16;
constexpr int32_t kFootMaxReach = 255;               // cells: 2 reach + 1 <= 511 rows of spans per pose
constexpr int32_t kFootMaxRows = 2 * kFootMaxReach + 1;
constexpr int32_t kFootLayerMaxReach = 64;           // the layer's tile plus a halo of reach cells lies in LDS
constexpr int32_t kFootMaxPoses = 65536, kFootMaxHeadings = 32, kFootMaxStatus = 2;
constexpr double kFootLattice = 1073741824.0;        // 2^30 cells: a vertex coordinate beyond it is KH_FOOTPRINT_LATTICE

// Strictly convex, in either winding: the cross products of consecutive edges all have one sign and none is 0 -- and the polygon
// goes round once: the x component of the edges changes sign exactly twice (a star that turns one way all along goes round twice).
inline bool foot_convex(int32_t n, const double * v)
{
  int32_t sign = 0, changes = 0, last_dx = 0;
  for (int32_t pass = 0; pass < 2; ++pass) {           // (the second pass closes the cycle of the sign changes)
    for (int32_t k = 0; k < n; ++k) {
      const int32_t k1 = (k + 1) % n, k2 = (k + 2) % n;
      const double ax = v[2 * k1] - v[2 * k], ay = v[2 * k1 + 1] - v[2 * k + 1];
      const double bx = v[2 * k2] - v[2 * k1], by = v[2 * k2 + 1] - v[2 * k1 + 1];
      const double cross = ax * by - ay * bx;
      const int32_t s = cross > 0.0 ? 1 : cross < 0.0 ? -1 : 0;
      if (s == 0 || (sign != 0 && s != sign)) {return false;}
      sign = s;
      const int32_t dx = ax > 0.0 ? 1 : ax < 0.0 ? -1 : 0;
      if (dx != 0) {
        if (pass == 1 && last_dx != 0 && dx != last_dx) {++changes;}
        last_dx = dx;
      }
    }
  }
  return changes == 2;
}

// r_max * scale as the rule states it; reach = ceil(that) + 1 cells, as a double: the caller compares before it converts
inline double foot_reach(int32_t n, const double * v, double scale)
{
  double r_max = 0.0;
  for (int32_t k = 0; k < n; ++k) {
    const double r = std::sqrt(v[2 * k] * v[2 * k] + v[2 * k + 1] * v[2 * k + 1]);
    r_max = r > r_max ? r : r_max;
  }
  return std::ceil(r_max * scale) + 1.0;
}

// what kh_map_footprint_create refuses before a device is looked for, in this order
enum : int32_t {kFootOk = 0, kFootNull = 1, kFootCount = 2, kFootNotFinite = 3, kFootNotConvex = 4, kFootTooFar = 5};
inline int32_t foot_create_check(const void * field, int32_t n, const double * v, const void * out, double scale, int32_t * reach)
{
  if (!field || !v || !out) {return kFootNull;}
  if (n < kFootMinVertices || n > kFootMaxVertices) {return kFootCount;}
  for (int32_t k = 0; k < 2 * n; ++k) {
    if (!std::isfinite(v[k])) {return kFootNotFinite;}
  }
  if (!foot_convex(n, v)) {return kFootNotConvex;}
  const double r = foot_reach(n, v, scale);
  if (!(r <= static_cast<double>(kFootMaxReach))) {return kFootTooFar;}
  *reach = static_cast<int32_t>(r);
  return kFootOk;
}

// what kh_map_footprint_check refuses before a device is looked for, in this order; *bad_pose takes the refused pose's index
enum : int32_t {kFootCallOk = 0, kFootCallCount = 1, kFootCallNull = 2, kFootCallPose = 3};
inline int32_t foot_check_check(int32_t n, const double * poses, const void * out, int32_t * bad_pose)
{
  if (n < 1 || n > kFootMaxPoses) {return kFootCallCount;}
  if (!poses || !out) {return kFootCallNull;}
  for (int64_t k = 0; k < 3 * static_cast<int64_t>(n); ++k) {
    if (!std::isfinite(poses[k])) {*bad_pose = static_cast<int32_t>(k / 3); return kFootCallPose;}
  }
  return kFootCallOk;
}

// what kh_map_footprint_layer refuses before a device is looked for, in this order (reach: the handle's, 0 without a handle)
enum : int32_t {kFootLayerOk = 0, kFootLayerHeadings = 1, kFootLayerStatus = 2, kFootLayerReach = 3};
inline int32_t foot_layer_check(int32_t n_headings, int32_t max_status, int32_t reach)
{
  if (n_headings < 1 || n_headings > kFootMaxHeadings) {return kFootLayerHeadings;}
  if (max_status < 0 || max_status > kFootMaxStatus) {return kFootLayerStatus;}
  if (reach > kFootLayerMaxReach) {return kFootLayerReach;}
  return kFootLayerOk;
}

// one coordinate pair rounded onto the lattice; false where either lies beyond +-2^30 cells (or is no number)
inline bool foot_cell(double cx, double cy, int32_t * out)
{
  if (!(std::fabs(cx) <= kFootLattice) || !(std::fabs(cy) <= kFootLattice)) {return false;}
  out[0] = static_cast<int32_t>(cx); out[1] = static_cast<int32_t>(cy);
  return true;
}

// libm's cos and sin, each called on its own: a compiler that sees both of one angle may call sincos in their place, and the rule
// (math.cos, math.sin) does not
__attribute__((noinline)) inline double foot_cos(double a) {return std::cos(a);}
__attribute__((noinline)) inline double foot_sin(double a) {return std::sin(a);}

// The vertex cells of pose (x, y, theta): libm's cos and sin here and nowhere else, the products and sums as written (the build
// contracts nothing).  cells takes 2 n words, own the pose's own cell; false = KH_FOOTPRINT_LATTICE.
inline bool foot_pose_cells(int32_t n, const double * v, const double * pose, double ax, double ay, double scale, int32_t * cells, int32_t * own)
{
  const double c = foot_cos(pose[2]), s = foot_sin(pose[2]);
  bool ok = true;
  for (int32_t k = 0; k < n; ++k) {
    const double wx = pose[0] + (c * v[2 * k] - s * v[2 * k + 1]);
    const double wy = pose[1] + (s * v[2 * k] + c * v[2 * k + 1]);
    ok = foot_cell(round_half_away((wx - ax) * scale), round_half_away((wy - ay) * scale), cells + 2 * k) && ok;
  }
  ok = foot_cell(round_half_away((pose[0] - ax) * scale), round_half_away((pose[1] - ay) * scale), own) && ok;
  return ok;
}

// The vertex offsets O_hk of heading h of H: theta_h = (2.0 * pi * h) / H.  (|O| <= ceil(r_max * scale) < reach: no lattice test.)
inline void foot_heading_offsets(int32_t n, const double * v, int32_t h, int32_t n_headings, double scale, int32_t * cells)
{
  const double theta = (2.0 * 3.141592653589793 * static_cast<double>(h)) / static_cast<double>(n_headings);
  const double c = foot_cos(theta), s = foot_sin(theta);
  for (int32_t k = 0; k < n; ++k) {
    cells[2 * k] = static_cast<int32_t>(round_half_away((c * v[2 * k] - s * v[2 * k + 1]) * scale));
    cells[2 * k + 1] = static_cast<int32_t>(round_half_away((s * v[2 * k] + c * v[2 * k + 1]) * scale));
  }
}

// ---- covered ----
// Edge k of the outline: the cells of RayWalk(V_k -> V_(k + 1) mod n), steps 0 .. length, each folded into the span of its row --
// rows.fold(x, y) keeps the smallest and the largest column per row.  The one statement of the outline: a lane of the pose kernel
// runs it for its edge with LDS atomics, the host for every edge in turn.  The caller has bounded the edge's length.
template <typename Rows>
KH_HOST_DEVICE void foot_edge(const int32_t * v, int32_t n, int32_t k, Rows & rows)
{
  const int32_t k1 = k + 1 == n ? 0 : k + 1;
  RayWalk walk(v[2 * k], v[2 * k + 1], v[2 * k1], v[2 * k1 + 1]);
  const int32_t length = walk.length();
  for (int32_t s = 0; s <= length; ++s, walk.next()) {rows.fold(walk.x(), walk.y());}
}

// The spans of a polygon on the host: rows y0 .. y0 + size - 1, row r covering columns lo[r] .. hi[r].
struct FootSpans
{
  int32_t y0 = 0;
  std::vector<int32_t> lo, hi;
  void fold(int32_t x, int32_t y)
  {
    const size_t r = static_cast<size_t>(y - y0);
    lo[r] = x < lo[r] ? x : lo[r]; hi[r] = x > hi[r] ? x : hi[r];
  }
};
// false where the vertex cells span more than kFootMaxRows rows or columns (the reach bounds both: it cannot happen)
inline bool foot_spans(const int32_t * v, int32_t n, FootSpans * out)
{
  int64_t x0 = v[0], x1 = v[0], y0 = v[1], y1 = v[1];
  for (int32_t k = 1; k < n; ++k) {
    x0 = v[2 * k] < x0 ? v[2 * k] : x0; x1 = v[2 * k] > x1 ? v[2 * k] : x1;
    y0 = v[2 * k + 1] < y0 ? v[2 * k + 1] : y0; y1 = v[2 * k + 1] > y1 ? v[2 * k + 1] : y1;
  }
  if (x1 - x0 >= kFootMaxRows || y1 - y0 >= kFootMaxRows) {return false;}
  out->y0 = static_cast<int32_t>(y0);
  out->lo.assign(static_cast<size_t>(y1 - y0 + 1), INT32_MAX); out->hi.assign(static_cast<size_t>(y1 - y0 + 1), INT32_MIN);
  for (int32_t k = 0; k < n; ++k) {foot_edge(v, n, k, *out);}
  return true;
}

// ---- the layer's stencil table ----
// 4 words per heading -- the first word of its spans, the first row's offset, its rows, 0 -- then (lo, hi) column offsets per row.
// false where an offset leaves the halo of `reach` cells (the bound did not hold).  *rows takes the rows of all headings.
inline bool foot_layer_table(int32_t n, const double * v, int32_t n_headings, double scale, int32_t reach, std::vector<int32_t> * table, int32_t * rows)
{
  table->assign(4 * static_cast<size_t>(n_headings), 0);
  *rows = 0;
  int32_t cells[2 * kFootMaxVertices];
  FootSpans spans;
  for (int32_t h = 0; h < n_headings; ++h) {
    foot_heading_offsets(n, v, h, n_headings, scale, cells);
    for (int32_t k = 0; k < 2 * n; ++k) {
      if (cells[k] < -reach || cells[k] > reach) {return false;}
    }
    if (!foot_spans(cells, n, &spans)) {return false;}
    (*table)[4 * h] = static_cast<int32_t>(table->size()); (*table)[4 * h + 1] = spans.y0; (*table)[4 * h + 2] = static_cast<int32_t>(spans.lo.size());
    for (size_t r = 0; r < spans.lo.size(); ++r) {table->push_back(spans.lo[r]); table->push_back(spans.hi[r]);}
    *rows += static_cast<int32_t>(spans.lo.size());
  }
  table->resize((table->size() + 3) / 4 * 4, 0);
  return true;
}
}  // namespace kh
