// Host half of ScanMatcher::ComputePositionalCovariance (Mapper.cpp:874-966) on the lattice maxima of a coarse search, and the exact
// scalar helpers it is written in (Math.h, Karto.h).  No device types: matcher_private.hpp includes it for the library, and
// tests/covariance_walk_check.cpp compiles it on its own.
//
// WorldToGrid (Karto.h:4421-4436) maps x and y independently, so a cell's column depends on the lattice column alone and its row on
// the lattice row alone: the indices are computed once per column and once per row (2 x (nx + ny) roundings instead of 2 x nx x ny)
// with the expressions the reference evaluates per cell, and the accumulation keeps the reference's order and expressions.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/karto_hip.h"

namespace kh
{

// ---- exact scalar helpers (Math.h) ----------------------------------------------------------
constexpr double kTolerance = 1e-06;                 // Math.h:41
constexpr double kMaxVariance = 500.0;               // Mapper.cpp:52

inline double round_half_away(double v) {return v >= 0.0 ? std::floor(v + 0.5) : std::ceil(v - 0.5);}
inline int32_t to_int32(double v)
{
  if (!(v > -2147483649.0 && v < 2147483648.0)) {return INT32_MIN;}
  return static_cast<int32_t>(v);
}
inline bool double_equal(double a, double b)
{
  const double delta = a - b;
  return delta < 0.0 ? delta >= -kTolerance : delta <= kTolerance;
}
struct Cell {int32_t x, y;};
// one axis of WorldToGrid, Karto.h:4421-4436
inline int32_t world_to_grid_axis(double scale, double offset, double world) {return to_int32(round_half_away((world - offset) * scale));}
inline Cell world_to_grid(double scale, double ox, double oy, double wx, double wy)
{
  return Cell{world_to_grid_axis(scale, ox, wx), world_to_grid_axis(scale, oy, wy)};
}

// the coarse search whose lattice maxima the walk reads: its centre, offsets and pose offsets (x_poses [nx], y_poses [ny])
struct WalkLattice
{
  double center[2] = {0, 0};
  double off_x = 0, off_y = 0;
  int32_t nx = 0, ny = 0;
  const double * x_poses = nullptr;
  const double * y_poses = nullptr;
};
// the CALLER's search geometry (Mapper.cpp:896-923)
struct WalkGeometry {double center[3], off_x, off_y, res_x, res_y, ang_res;};

// `side` and `resolution`: the matcher's search-space-probs grid (Grid<kt_double>, side x side, Mapper.cpp:513-514, 726-732);
// lattice_max [ny * nx].  KH_ERR_SEARCH: a cell left that grid (Mapper.cpp:786-796).
inline int positional_covariance(
  int32_t side, double resolution, const WalkLattice & c, const double * lattice_max, const WalkGeometry & w,
  const double best_pose[3], double best_response, double * cov)
{
  std::fill(cov, cov + 9, 0.0);
  cov[0] = 1.0; cov[4] = 1.0; cov[8] = 1.0;       // SetToIdentity
  if (best_response < kTolerance) {
    cov[0] = kMaxVariance; cov[4] = kMaxVariance; cov[8] = 4 * (w.ang_res * w.ang_res);
    return KH_OK;
  }
  // search-space-probs grid (Mapper.cpp:781-799)
  const double pscale = 1.0 / resolution;               // Grid::CreateGrid -> SetScale(1.0 / resolution)
  const double pox = c.center[0] - c.off_x, poy = c.center[1] - c.off_y;
  auto inside = [side](int32_t g) {return g >= 0 && g < side;};
  std::vector<int32_t> gx, gy;
  gx.reserve(static_cast<size_t>(std::max(c.nx, 0))); gy.reserve(static_cast<size_t>(std::max(c.ny, 0)));
  bool left = false;
  for (int32_t xi = 0; xi < c.nx; ++xi) {
    gx.push_back(world_to_grid_axis(pscale, pox, c.center[0] + c.x_poses[xi]));
    left = left || !inside(gx.back());
  }
  for (int32_t yi = 0; yi < c.ny; ++yi) {
    gy.push_back(world_to_grid_axis(pscale, poy, c.center[1] + c.y_poses[yi]));
    left = left || !inside(gy.back());
  }
  // (every column meets every row: a column or a row outside is a cell outside as soon as there is a cell at all)
  if (left && c.nx > 0 && c.ny > 0) {return KH_ERR_SEARCH;}   // Mapper.cpp:786-796
  std::vector<double> probs(static_cast<size_t>(side) * side, 0.0);
  for (int32_t yi = 0; yi < c.ny; ++yi) {
    double * row = probs.data() + static_cast<size_t>(gy[yi]) * side;
    const double * from = lattice_max + static_cast<size_t>(yi) * c.nx;
    for (int32_t xi = 0; xi < c.nx; ++xi) {
      double & cell = row[gx[xi]];
      const double v = from[xi];
      cell = v > cell ? v : cell;
    }
  }
  double aXX = 0, aXY = 0, aYY = 0, norm = 0;
  // the walk uses the CALLER's geometry on the grid the last coarse search left behind (Mapper.cpp:896-923)
  const double dx = best_pose[0] - w.center[0], dy = best_pose[1] - w.center[1];
  const uint32_t nX = static_cast<uint32_t>(round_half_away(w.off_x * 2.0 / w.res_x) + 1);
  const double startX = -w.off_x;
  const uint32_t nY = static_cast<uint32_t>(round_half_away(w.off_y * 2.0 / w.res_y) + 1);
  const double startY = -w.off_y;
  std::vector<double> xs, ys;
  if (nX > 0 && nY > 0) {
    // (the reference's walk ends at the first cell outside, in row 0 at the latest when a column is: the first cell's row is
    // looked at in front of the columns, so that a geometry far too wide for the grid ends here as early as it does there)
    if (!inside(world_to_grid_axis(pscale, poy, w.center[1] + (startY + 0u * w.res_y)))) {return KH_ERR_SEARCH;}
    gx.clear(); gy.clear();
    for (uint32_t xi = 0; xi < nX; ++xi) {
      const double x = startX + xi * w.res_x;
      const int32_t g = world_to_grid_axis(pscale, pox, w.center[0] + x);
      if (!inside(g)) {return KH_ERR_SEARCH;}
      xs.push_back(x); gx.push_back(g);
    }
    for (uint32_t yi = 0; yi < nY; ++yi) {
      const double y = startY + yi * w.res_y;
      const int32_t g = world_to_grid_axis(pscale, poy, w.center[1] + y);
      if (!inside(g)) {return KH_ERR_SEARCH;}
      ys.push_back(y); gy.push_back(g);
    }
    for (uint32_t yi = 0; yi < nY; ++yi) {
      const double y = ys[yi];
      const double * row = probs.data() + static_cast<size_t>(gy[yi]) * side;
      for (uint32_t xi = 0; xi < nX; ++xi) {
        const double x = xs[xi];
        const double response = row[gx[xi]];
        if (response >= (best_response - 0.1)) {
          norm += response;
          aXX += ((x - dx) * (x - dx) * response);
          aXY += ((x - dx) * (y - dy) * response);
          aYY += ((y - dy) * (y - dy) * response);
        }
      }
    }
  }
  if (norm > kTolerance) {
    double vXX = aXX / norm, vXY = aXY / norm, vYY = aYY / norm;
    const double vTHTH = 4 * (w.ang_res * w.ang_res);
    const double minXX = 0.1 * (w.res_x * w.res_x), minYY = 0.1 * (w.res_y * w.res_y);
    vXX = vXX > minXX ? vXX : minXX;
    vYY = vYY > minYY ? vYY : minYY;
    const double mult = 1.0 / best_response;
    cov[0] = vXX * mult; cov[1] = vXY * mult; cov[3] = vXY * mult; cov[4] = vYY * mult; cov[8] = vTHTH;
  }
  if (double_equal(cov[0], 0.0)) {cov[0] = kMaxVariance;}
  if (double_equal(cov[4], 0.0)) {cov[4] = kMaxVariance;}
  return KH_OK;
}

}  // namespace kh
