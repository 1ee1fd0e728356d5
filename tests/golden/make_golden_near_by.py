"""Generates tests/golden/near_by.npz: what nanoflann itself answers to the two questions MapperGraph::FindNearByScan
(Mapper.cpp:1877-1912: knnSearch, one neighbour) and MapperGraph::FindNearByVertices (:1837-1875: radiusSearch with
maxDistance as the radius and default SearchParams) ask it, for seeded random points.

A throw-away driver (the text below, this project's own) is compiled against the reference tree's nanoflann.hpp in a temporary
directory, with a point adaptor of the shape of the reference's VertexVectorPoseNanoFlannAdaptor and the same index type and
leaf size as Mapper.cpp; only its output is kept.  Needs the reference tree and a C++ compiler; run once:

    python tests/golden/make_golden_near_by.py <reference tree>

tests/test_localization_oracle.py needs only the fixture."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "nanoflann.hpp"

struct Points
{
  std::vector<double> xy;
  inline size_t kdtree_get_point_count() const {return xy.size() / 2;}
  inline double kdtree_get_pt(const size_t idx, const size_t dim) const {return xy[2 * idx + dim];}
  template<class BBOX> bool kdtree_get_bbox(BBOX &) const {return false;}
};
typedef nanoflann::KDTreeSingleIndexAdaptor<nanoflann::L2_Simple_Adaptor<double, Points>, Points, 2> Tree;

int main(int argc, char ** argv)
{
  // in: n q r, n points, q queries, r radii (text, %la); out: per query the nearest index and its distance, then per radius the hits
  FILE * in = std::fopen(argv[1], "r");
  FILE * out = std::fopen(argv[2], "w");
  if (argc < 3 || !in || !out) {return 1;}
  int n = 0, q = 0, r = 0;
  if (std::fscanf(in, "%d %d %d", &n, &q, &r) != 3) {return 1;}
  Points pts;
  pts.xy.resize(2 * static_cast<size_t>(n));
  std::vector<double> queries(2 * static_cast<size_t>(q)), radii(static_cast<size_t>(r));
  for (double & v : pts.xy) {if (std::fscanf(in, "%la", &v) != 1) {return 1;}}
  for (double & v : queries) {if (std::fscanf(in, "%la", &v) != 1) {return 1;}}
  for (double & v : radii) {if (std::fscanf(in, "%la", &v) != 1) {return 1;}}
  Tree index(2, pts, nanoflann::KDTreeSingleIndexAdaptorParams(10));
  index.buildIndex();
  for (int k = 0; k < q; ++k) {
    size_t ret = 0;
    double d = 0.0;
    const size_t found = index.knnSearch(&queries[2 * k], 1, &ret, &d);
    std::fprintf(out, "N %d %ld %a\n", k, found ? static_cast<long>(ret) : -1L, d);
    for (int j = 0; j < r; ++j) {
      std::vector<std::pair<size_t, double>> matches;
      nanoflann::SearchParams params;
      index.radiusSearch(&queries[2 * k], radii[j], matches, params);
      std::fprintf(out, "R %d %d %zu", k, j, matches.size());
      for (const auto & m : matches) {std::fprintf(out, " %zu", m.first);}
      std::fprintf(out, "\n");
    }
  }
  std::fclose(out);
  return 0;
}
"""


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    include = os.path.join(sys.argv[1], "lib", "karto_sdk", "include", "karto_sdk")
    assert os.path.exists(os.path.join(include, "nanoflann.hpp")), include
    rng = np.random.default_rng(20261016)
    n, q = 2000, 64
    points = rng.uniform(0.0, 35.0, size=(n, 2))
    queries = rng.uniform(-1.0, 36.0, size=(q, 2))
    radii = np.array([0.5, 2.0, 9.0])            # compared with SQUARED distances: 0.71 m, 1.41 m, 3 m
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, fin, fout = (os.path.join(tmp, f) for f in ("driver.cpp", "driver", "in.txt", "out.txt"))
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-I", include, "-o", exe, src])
        with open(fin, "w") as f:
            f.write(f"{n} {q} {len(radii)}\n")
            for v in np.concatenate([points.reshape(-1), queries.reshape(-1), radii]):
                f.write(float(v).hex() + "\n")
        subprocess.check_call([exe, fin, fout])
        nearest = np.full(q, -2, dtype=np.int32)
        nearest_d = np.zeros(q)
        hit_begin = np.zeros((q, len(radii) + 1), dtype=np.int32)
        hits = []
        for line in open(fout):
            t = line.split()
            if t[0] == "N":
                nearest[int(t[1])] = int(t[2])
                nearest_d[int(t[1])] = float.fromhex(t[3])
            else:
                k, j, c = int(t[1]), int(t[2]), int(t[3])
                assert len(t) == 4 + c
                hit_begin[k, j] = len(hits)
                hits.extend(int(v) for v in t[4:])
                hit_begin[k, j + 1] = len(hits)
    assert (nearest >= 0).all()
    out = os.path.join(HERE, "near_by.npz")
    np.savez_compressed(out, points=points, queries=queries, radii=radii, nearest=nearest, nearest_dist_sq=nearest_d,
                        hit_begin=hit_begin, hits=np.asarray(hits, dtype=np.int32))
    print(out, os.path.getsize(out), "bytes;", len(hits), "hits")


if __name__ == "__main__":
    main()
