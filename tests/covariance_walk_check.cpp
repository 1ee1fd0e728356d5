// Stand-alone check of slam_toolbox_amd/csrc/covariance_walk.hpp (no GPU, no HIP): the separable covariance walk against the walk
// as the reference writes it -- WorldToGrid per lattice cell in both loops (Mapper.cpp:781-799, 896-923) -- which is kept here.
// One case per line of stdin, doubles as hex floats:
//   walk <side> <resolution> <cx> <cy> <off_x> <off_y> <res_x> <res_y>  <wcx> <wcy> <woff_x> <woff_y> <wres_x> <wres_y> <wang_res>
//        <bx> <by> <bt> <best_response> <seed>
// The search lattice (nx, ny, x_poses, y_poses) follows from the offsets and resolutions as in the library (Mapper.cpp:736-756); its
// maxima come from `seed`.  Answer, one line: <rc as written> <rc separable> <nx> <ny> <the 9 covariance words as written> <separable>,
// as 64-bit patterns
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../slam_toolbox_amd/csrc/covariance_walk.hpp"

using namespace kh;

// the walk as written: one WorldToGrid per cell, in both loops
static int positional_covariance_as_written(
  int32_t side, double resolution, const WalkLattice & c, const std::vector<double> & lattice_max, const WalkGeometry & w,
  const double best_pose[3], double best_response, double * cov)
{
  std::fill(cov, cov + 9, 0.0);
  cov[0] = 1.0; cov[4] = 1.0; cov[8] = 1.0;
  if (best_response < kTolerance) {
    cov[0] = kMaxVariance; cov[4] = kMaxVariance; cov[8] = 4 * (w.ang_res * w.ang_res);
    return KH_OK;
  }
  const double pscale = 1.0 / resolution;
  const double pox = c.center[0] - c.off_x, poy = c.center[1] - c.off_y;
  std::vector<double> probs(static_cast<size_t>(side) * side, 0.0);
  for (int32_t yi = 0; yi < c.ny; ++yi) {
    for (int32_t xi = 0; xi < c.nx; ++xi) {
      const double px = c.center[0] + c.x_poses[xi], py = c.center[1] + c.y_poses[yi];
      const double gx = (px - pox) * pscale;
      const double gy = (py - poy) * pscale;
      const Cell g{to_int32(round_half_away(gx)), to_int32(round_half_away(gy))};
      if (!(g.x >= 0 && g.x < side) || !(g.y >= 0 && g.y < side)) {return KH_ERR_SEARCH;}
      double & cell = probs[static_cast<size_t>(g.y) * side + g.x];
      const double v = lattice_max[static_cast<size_t>(yi) * c.nx + xi];
      cell = v > cell ? v : cell;
    }
  }
  double aXX = 0, aXY = 0, aYY = 0, norm = 0;
  const double dx = best_pose[0] - w.center[0], dy = best_pose[1] - w.center[1];
  const uint32_t nX = static_cast<uint32_t>(round_half_away(w.off_x * 2.0 / w.res_x) + 1);
  const double startX = -w.off_x;
  const uint32_t nY = static_cast<uint32_t>(round_half_away(w.off_y * 2.0 / w.res_y) + 1);
  const double startY = -w.off_y;
  for (uint32_t yi = 0; yi < nY; ++yi) {
    const double y = startY + yi * w.res_y;
    for (uint32_t xi = 0; xi < nX; ++xi) {
      const double x = startX + xi * w.res_x;
      const double gx = ((w.center[0] + x) - pox) * pscale;
      const double gy = ((w.center[1] + y) - poy) * pscale;
      const Cell g{to_int32(round_half_away(gx)), to_int32(round_half_away(gy))};
      if (!(g.x >= 0 && g.x < side) || !(g.y >= 0 && g.y < side)) {return KH_ERR_SEARCH;}
      const double response = probs[static_cast<size_t>(g.y) * side + g.x];
      if (response >= (best_response - 0.1)) {
        norm += response;
        aXX += ((x - dx) * (x - dx) * response);
        aXY += ((x - dx) * (y - dy) * response);
        aYY += ((y - dy) * (y - dy) * response);
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

static double hex_double(const std::string & s) {return std::strtod(s.c_str(), nullptr);}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string word;
    in >> word;
    if (word != "walk") {std::printf("unknown command\n"); return 2;}
    long side = 0;
    in >> side;
    std::vector<double> v;
    while (in >> word) {v.push_back(hex_double(word));}
    if (side <= 0 || v.size() != 19) {std::printf("bad line\n"); return 2;}
    const double resolution = v[0];
    WalkLattice c;
    c.center[0] = v[1]; c.center[1] = v[2]; c.off_x = v[3]; c.off_y = v[4];
    const double res_x = v[5], res_y = v[6];
    WalkGeometry w;
    w.center[0] = v[7]; w.center[1] = v[8]; w.center[2] = 0.0;
    w.off_x = v[9]; w.off_y = v[10]; w.res_x = v[11]; w.res_y = v[12]; w.ang_res = v[13];
    const double best_pose[3] = {v[14], v[15], v[16]};
    const double best_response = v[17];
    uint64_t state = static_cast<uint64_t>(v[18]) * 2654435761u + 12345u;
    // the search lattice, Mapper.cpp:736-756
    c.nx = static_cast<int32_t>(static_cast<uint32_t>(round_half_away(c.off_x * 2.0 / res_x) + 1));
    c.ny = static_cast<int32_t>(static_cast<uint32_t>(round_half_away(c.off_y * 2.0 / res_y) + 1));
    std::vector<double> xp(c.nx), yp(c.ny);
    for (int32_t k = 0; k < c.nx; ++k) {xp[k] = -c.off_x + static_cast<uint32_t>(k) * res_x;}
    for (int32_t k = 0; k < c.ny; ++k) {yp[k] = -c.off_y + static_cast<uint32_t>(k) * res_y;}
    c.x_poses = xp.data(); c.y_poses = yp.data();
    // maxima in [0, 0.9]: a ridge towards the middle and noise on it, so that the walk's threshold (best - 0.1) cuts through them
    std::vector<double> lattice(static_cast<size_t>(c.nx) * c.ny);
    for (int32_t yi = 0; yi < c.ny; ++yi) {
      for (int32_t xi = 0; xi < c.nx; ++xi) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const double noise = static_cast<double>(state >> 40) / static_cast<double>(1 << 24);
        const double fx = c.nx > 1 ? static_cast<double>(xi) / (c.nx - 1) - 0.5 : 0.0, fy = c.ny > 1 ? static_cast<double>(yi) / (c.ny - 1) - 0.5 : 0.0;
        lattice[static_cast<size_t>(yi) * c.nx + xi] = 0.9 * (0.7 * (1.0 - 2.0 * (fx * fx + fy * fy)) + 0.3 * noise);
      }
    }
    double cov_a[9], cov_b[9];
    for (int k = 0; k < 9; ++k) {cov_a[k] = cov_b[k] = -7.0 - k;}      // both walks write all nine
    const int rc_a = positional_covariance_as_written(static_cast<int32_t>(side), resolution, c, lattice, w, best_pose, best_response, cov_a);
    const int rc_b = positional_covariance(static_cast<int32_t>(side), resolution, c, lattice.data(), w, best_pose, best_response, cov_b);
    std::printf("%d %d %d %d", rc_a, rc_b, c.nx, c.ny);
    for (int k = 0; k < 9; ++k) {uint64_t b; std::memcpy(&b, &cov_a[k], 8); std::printf(" %016" PRIx64, b);}
    for (int k = 0; k < 9; ++k) {uint64_t b; std::memcpy(&b, &cov_b[k], 8); std::printf(" %016" PRIx64, b);}
    std::printf("\n");
  }
  return 0;
}
