"""The rule of global relocalization in numpy, and nothing else: where one scan that comes without a pose is
tried in a map, and which tries are kept.  It reads nothing of the library; the matches are oracle.karto.Matcher's.

  vertices    the scans still in the graph, in scan-list order; positions = corrected pose x, y
  seeds       a lattice of side seed_spacing; the cell of a vertex is (floor(x / seed_spacing), floor(y / seed_spacing)), an FP64 divide
              and floor; the seed of a non-empty cell is its vertex with the lowest list index; seeds in ascending list index; with a
              region (centre, radius > 0) only the seeds with (dx * dx) + (dy * dy) < radius * radius + KT_TOLERANCE from the centre
  base        of a seed: every vertex with (dx * dx) + (dy * dy) < R * R + KT_TOLERANCE from it (R = loop_search_maximum_distance),
              ascending; of c > max_base entries, entries 0, s, 2s, ... with s = ceil(c / max_base)
  headings    -pi + h * (2 pi / n_headings), h = 0 .. n_headings - 1
  hypothesis  (seed k, heading h), index k * n_headings + h: the robot at (x_seed, y_seed, heading_h), the sensor through the laser's
              offset, the readings recomputed there; TryCloseLoop's test (Mapper.cpp:1515-1549): coarse match on the loop matcher
              (no penalty, no refinement), the gate (response > minimum_response_coarse, cov(0,0) and cov(1,1) <
              maximum_variance_coarse), fine match of the temporary scan at the coarse pose on the sequential matcher (no penalty,
              refined), accepted when fine response >= minimum_response_fine
  answer      the accepted hypotheses by fine response descending, then coarse response descending, then index ascending
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

KT_TOLERANCE = 1e-06           # Math.h:41


def cells(pose_xy, seed_spacing):
    """(n, 2) cell coordinates as FP64 values: floor of the FP64 quotient (a negative coordinate goes down; -0.0 is cell 0)"""
    return np.floor(np.asarray(pose_xy, dtype=np.float64).reshape(-1, 2) / np.float64(seed_spacing))


def dist_sq(pose_xy, q):
    """(dx * dx) + (dy * dy), each operation rounded on its own"""
    p = np.asarray(pose_xy, dtype=np.float64).reshape(-1, 2)
    dx, dy = p[:, 0] - np.float64(q[0]), p[:, 1] - np.float64(q[1])
    return (dx * dx) + (dy * dy)


def seeds(pose_xy, seed_spacing, center_xy=None, radius=0.0):
    p = np.asarray(pose_xy, dtype=np.float64).reshape(-1, 2)
    first = {}
    for i, c in enumerate(cells(p, seed_spacing)):
        first.setdefault((float(c[0]), float(c[1])), i)            # -0.0 == 0.0: one key
    s = np.asarray(sorted(first.values()), dtype=np.int32)
    if center_xy is not None and radius > 0 and s.size:
        s = s[dist_sq(p[s], center_xy) < np.float64(radius) * np.float64(radius) + KT_TOLERANCE]
    return s.astype(np.int32)


def base(pose_xy, seed, max_distance, max_base):
    p = np.asarray(pose_xy, dtype=np.float64).reshape(-1, 2)
    idx = np.nonzero(dist_sq(p, p[seed]) < np.float64(max_distance) * np.float64(max_distance) + KT_TOLERANCE)[0]
    c = idx.size
    if c > max_base:
        idx = idx[::-(-c // max_base)]
    return idx.astype(np.int32)


def candidates(pose_xy, seed_spacing, max_distance, max_base, center_xy=None, radius=0.0):
    """-> (seeds, base_begin, base_idx): the enumeration in CSR form"""
    s = seeds(pose_xy, seed_spacing, center_xy, radius)
    bases = [base(pose_xy, k, max_distance, max_base) for k in s]
    begin = np.concatenate([[0], np.cumsum([b.size for b in bases])]).astype(np.int32)
    idx = np.concatenate(bases).astype(np.int32) if bases else np.zeros(0, dtype=np.int32)
    return s, begin, idx


def default_n_headings(coarse_search_angle_offset):
    return int(math.ceil(2.0 * math.pi / (2.0 * coarse_search_angle_offset)))


def headings(n_headings):
    return np.asarray([-math.pi + h * (2.0 * math.pi / n_headings) for h in range(n_headings)], dtype=np.float64)


def sensor_at(robot, offset=(0.0, 0.0, 0.0)):
    """LocalizedRangeScan::GetSensorAt (Karto.h:5566-5569): the laser's offset pose carried to the robot pose.  With a zero offset the
    sensor pose is the robot pose, bit for bit (x + 0.0); with one, cos and sin here are libm's separate calls."""
    x, y, h = (float(v) for v in robot)
    ox, oy, oh = (float(v) for v in offset)
    c, s = math.cos(h), math.sin(h)
    a = h + oh
    while a < -math.pi:
        a += 2.0 * math.pi
    while a > math.pi:
        a -= 2.0 * math.pi
    return np.array([x + (c * ox + (-s) * oy + 0.0 * oh), y + (s * ox + c * oy + 0.0 * oh), a])


def robot_at(sensor, offset=(0.0, 0.0, 0.0)):
    """LocalizedRangeScan::GetCorrectedAt (Karto.h:5576-5588)"""
    ox, oy, oh = (float(v) for v in offset)
    length = math.sqrt(ox * ox + oy * oy)
    w = float(sensor[2]) + math.atan2(oy, ox) - oh
    h = float(sensor[2]) - oh
    while h < -math.pi:
        h += 2.0 * math.pi
    while h > math.pi:
        h -= 2.0 * math.pi
    return np.array([float(sensor[0]) - length * math.cos(w), float(sensor[1]) - length * math.sin(w), h])


Hyp = namedtuple("Hyp", "index seed heading coarse_mean coarse_cov coarse_response passed fine_mean fine_cov fine_response accepted")
Result = namedtuple("Result", "seeds base_begin base_idx headings hyps ranking")


def relocalize(pose_xy, base_scans, ranges, laser, coarse, fine, minimum_response_coarse, maximum_variance_coarse, minimum_response_fine,
               seed_spacing, max_distance, n_headings, max_base=40, center_xy=None, radius=0.0):
    """pose_xy (n, 2) and base_scans (n oracle.karto.Scan) in scan-list order; coarse / fine: oracle.karto.Matcher (loop / sequential).
    -> Result: every hypothesis in index order, and `ranking` = the indices of the accepted ones, best first."""
    from oracle import karto
    s, begin, idx = candidates(pose_xy, seed_spacing, max_distance, max_base, center_xy, radius)
    hs = headings(n_headings)
    p = np.asarray(pose_xy, dtype=np.float64).reshape(-1, 2)
    offset = tuple(getattr(laser, "offset", (0.0, 0.0, 0.0)))
    hyps = []
    for k, seed in enumerate(s):
        chain = [base_scans[j] for j in idx[begin[k]:begin[k + 1]]]
        for h, heading in enumerate(hs):
            query = karto.Scan(ranges, sensor_at((p[seed, 0], p[seed, 1], heading), offset), laser)
            cr, cm, cc = coarse.match_scan(query, chain, False, False)
            passed = bool(cr > minimum_response_coarse and cc[0, 0] < maximum_variance_coarse and cc[1, 1] < maximum_variance_coarse)
            fr, fm, fc, accepted = 0.0, np.zeros(3), np.zeros((3, 3)), False
            if passed:
                fr, fm, fc = fine.match_scan(query.with_sensor_pose(cm, laser), chain, False, True)        # tmpScan.SetSensorPose(bestPose)
                accepted = bool(fr >= minimum_response_fine)
            hyps.append(Hyp(k * n_headings + h, int(seed), float(heading), cm, cc, float(cr), passed, fm, fc, float(fr), accepted))
    ranking = sorted((h.index for h in hyps if h.accepted), key=lambda i: (-hyps[i].fine_response, -hyps[i].coarse_response, i))     # stable
    return Result(s, begin, idx, hs, hyps, ranking)
