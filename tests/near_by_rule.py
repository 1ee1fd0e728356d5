"""The near-by queries of the graph store restated in numpy (float64), independent of the library: what
MapperGraph::FindNearByScan (Mapper.cpp:1877-1912) and MapperGraph::FindNearByVertices (:1837-1875) ask nanoflann.

* distance: nanoflann's L2_Simple_Adaptor sum, (dx * dx) + (dy * dy), every operation rounded on its own (numpy does not fuse);
* nearest: argmin (the first of equal distances = the lower index, the library's tie rule);
* radius: the reference hands maxDistance to radiusSearch, whose result set keeps `dist < radius` with dist the SQUARED
  distance (nanoflann.hpp:274): squared distance against the unsquared radius, strictly; hits by ascending distance
  (SearchParams::sorted, nanoflann.hpp:630, 1418), the lower index first between equal distances.

tests/test_localization_oracle.py pins this file to nanoflann itself (tests/golden/near_by.npz)."""
import numpy as np


def dist_sq(points, query):
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    dx = np.float64(query[0]) - points[:, 0]
    dy = np.float64(query[1]) - points[:, 1]
    return dx * dx + dy * dy


def find_near_by_scan(points, query):
    """-> (index, dist_sq); (-1, inf) for no points"""
    d = dist_sq(points, query)
    if d.size == 0:
        return -1, np.inf
    k = int(np.argmin(d))
    return k, d[k]


def find_near_by_vertices(points, query, max_distance):
    """-> indices of the points with dist_sq < max_distance, by ascending (dist_sq, index)"""
    d = dist_sq(points, query)
    hits = np.nonzero(d < np.float64(max_distance))[0]
    return hits[np.lexsort((hits, d[hits]))].astype(np.int32)


def best_two_differ(points, query):
    """no exact tie for the nearest point (nanoflann's answer to one depends on its tree)"""
    d = np.sort(dist_sq(points, query))
    return d.size < 2 or d[0] != d[1]


def hits_are_distinct(points, query, max_distance):
    """no two hits at the same distance and none exactly at the radius"""
    d = dist_sq(points, query)
    h = np.sort(d[d <= np.float64(max_distance)])
    return not np.any(d == np.float64(max_distance)) and not np.any(h[1:] == h[:-1])
