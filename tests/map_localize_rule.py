"""TEST INFRASTRUCTURE (not a test): the rule of the map localizer in numpy on the CPU oracle -- what
kh_map_seeds, kh_map_fit and kh_map_localizer_* must compute.  It reads nothing of the library.  The matches are
tests/map_match_rule.py's (rule_grid + install + match on oracle.karto.Matcher), the counters' derived values tests/merge_fit_rule.py's.

  lattice     the cell of a world point v is o_to_int(o_round((v - anchor) * scale)); the window holds lattice cells
              [ox, ox + width) x [oy, oy + height); a cell outside it does not exist; columns width .. width_step - 1 are never read
  seeds       pitch = max(1, (int)round_half_away(seed_spacing * scale)) | 1 cells; block (bx, by) = floor quotients of the lattice index;
              the seed of a block is its cell of state 255 inside the window that minimises (2 i - (2 bx p + p - 1))^2 +
              (2 j - (2 by p + p - 1))^2, ties to the smaller j, then the smaller i; ascending (by, bx); world point
              anchor + (lattice index) / scale; with a region only (dx * dx) + (dy * dy) < radius * radius + KT_TOLERANCE
  hypothesis  k * n_headings + h: robot at seed k, heading -pi + h * (2 pi / n_headings), sensor through the laser offset, coarse match
              (loop matcher, no penalty, no refinement), gate, fine match at the coarse mean (sequential matcher, no penalty, refined)
  fit         AddScan's gate, TraceLine on the lattice, visits counted by the state of the cell, outside the window dropped
  answer      accepted by fine response desc, coarse response desc, index; fitted at the fine mean; known > 0 and score < min_fit_score
              dropped; greedy suppression within merge_distance / merge_heading of a KEPT one; the first top_k
  tracking    predicted = Transform(last odometric, last corrected).TransformPose(odometric); match on the sequential matcher,
              penalised and refined, from the sensor pose of the prediction; corrected = GetCorrectedAt(mean); fit at the mean
"""
from __future__ import annotations

import ctypes
import ctypes.util
import math
from collections import namedtuple

import numpy as np

import map_match_rule as mr
import merge_fit_rule as fr
import occupancy_cases as oc
import relocalize_rule as rr

KT_TOLERANCE = 1e-06
FREE = 255
MAX_PITCH = 4096
MAX_WALK = 1 << 20
MAX_CELL = float(1 << 30)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
_libm.sincos.restype = None


def sincos(a):
    """libm's sincos: what the reference's Release build calls for a cos / sin pair of one angle (not everywhere bit-equal to cos, sin)"""
    s, c = ctypes.c_double(), ctypes.c_double()
    _libm.sincos(float(a), ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


# ---------------------------------------------------------------- lattice
def o_round(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v >= 0.0, np.floor(v + 0.5), np.ceil(v - 0.5))


def lattice_cell(v, anchor, scale):
    """o_to_int(o_round((v - anchor) * scale)) of one coordinate, as a python int"""
    r = float(o_round((np.float64(v) - np.float64(anchor)) * np.float64(scale)))
    if not (-2147483649.0 < r < 2147483648.0):
        return -2 ** 31
    return int(r)


def state_at(view, cx, cy):
    """the state of lattice cell (cx, cy), None when it does not exist"""
    wx, wy = cx - view["ox"], cy - view["oy"]
    if 0 <= wx < view["width"] and 0 <= wy < view["height"]:
        return int(view["cells"][wy, wx])
    return None


# ---------------------------------------------------------------- seeds
def round_half_away(v):
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


def pitch_of(seed_spacing, scale):
    """-> the odd pitch in cells; ValueError where the library answers KH_ERR_INVALID_ARG"""
    if not (math.isfinite(seed_spacing) and seed_spacing > 0.0):
        raise ValueError("seed_spacing")
    cells = round_half_away(float(np.float64(seed_spacing) * np.float64(scale)))
    pitch = max(1, int(cells)) | 1 if cells <= MAX_PITCH else MAX_PITCH + 1
    if pitch > MAX_PITCH:
        raise ValueError("pitch above 4096 cells")
    return pitch


def seeds(view, seed_spacing, center_xy=None, radius=0.0):
    """-> (cells (n, 2) int64 lattice i, j; xy (n, 2) float64)"""
    p = pitch_of(seed_spacing, view["scale"])
    win = view["cells"][:view["height"], :view["width"]]
    j, i = np.nonzero(win == FREE)
    li, lj = i.astype(np.int64) + view["ox"], j.astype(np.int64) + view["oy"]
    bx, by = li // p, lj // p                                # floor quotients
    d = (2 * li - (2 * bx * p + p - 1)) ** 2 + (2 * lj - (2 * by * p + p - 1)) ** 2
    order = np.lexsort((li, lj, d, bx, by))                  # by, then bx, then distance, then j, then i
    first = np.ones(order.size, dtype=bool)
    first[1:] = (by[order][1:] != by[order][:-1]) | (bx[order][1:] != bx[order][:-1])
    pick = order[first]
    cells = np.stack([li[pick], lj[pick]], axis=1).reshape(-1, 2)
    xy = np.stack([view["anchor"][0] + cells[:, 0].astype(np.float64) / view["scale"],
                   view["anchor"][1] + cells[:, 1].astype(np.float64) / view["scale"]], axis=1).reshape(-1, 2)
    if center_xy is not None and radius > 0 and cells.shape[0]:
        keep = rr.dist_sq(xy, center_xy) < np.float64(radius) * np.float64(radius) + KT_TOLERANCE
        cells, xy = cells[keep], xy[keep]
    return cells, xy


# ---------------------------------------------------------------- fit
def gate(r, p, s, laser):
    """AddScan (Karto.h:6148-6189) of one beam: (kept, hit, end point)"""
    r = float(r)
    valid_end = r < (laser.range_threshold - 1e-06)
    if r <= laser.min_range or r >= laser.max_range or r != r:
        return False, False, None
    px, py = float(p[0]), float(p[1])
    if r >= laser.range_threshold:
        ratio = np.float64(laser.range_threshold) / np.float64(r)
        dx, dy = np.float64(px) - np.float64(s[0]), np.float64(py) - np.float64(s[1])
        px, py = float(np.float64(s[0]) + ratio * dx), float(np.float64(s[1]) + ratio * dy)
    return True, valid_end, (px, py)


def fit_refused(view, laser, pose):
    """does the library refuse this fit with KH_ERR_INVALID_ARG (a walk that could be longer than 2^20 cells)?"""
    if not (math.isfinite(laser.range_threshold) and laser.range_threshold > 0 and laser.range_threshold * view["scale"] + 2.0 <= MAX_WALK):
        return True
    if not all(math.isfinite(float(v)) for v in pose):
        return True
    return any(abs((float(pose[k]) - view["anchor"][k]) * view["scale"]) > MAX_CELL for k in (0, 1))


def line_cells(x0, y0, x1, y1):
    """Grid<T>::TraceLine (Karto.h:4874-4927) in closed form: the cells of tests/occupancy_cases.bresenham as two int64 arrays.  After k
    steps along the long axis the walk has stepped floor(k dy / dx + 1 / 2) times along the short one: it steps at step t exactly when
    2 ((t + 1) dy - dx y_t) >= dx.  (tests/test_map_localize_rule_oracle.py holds the two side by side.)"""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, x1, y0, y1 = x1, x0, y1, y0
    dx, dy = x1 - x0, abs(y1 - y0)
    k = np.arange(dx + 1, dtype=np.int64)
    x = x0 + k
    y = y0 + (1 if y0 < y1 else -1) * ((2 * k * dy + dx) // (2 * dx)) if dx > 0 else np.full(1, y0, dtype=np.int64)
    return (y, x) if steep else (x, y)


def fit_counters(view, laser, ranges, pose, points=None):
    """the six counters of one scan at sensor pose `pose`; points default to the oracle's scan_points at that pose"""
    from oracle import karto
    ranges = np.asarray(ranges, dtype=np.float64)
    pose = np.asarray(pose, dtype=np.float64)
    assert not fit_refused(view, laser, pose)
    if points is None:
        points = karto.scan_points(ranges, pose, laser)
    ax, ay, scale = view["anchor"][0], view["anchor"][1], view["scale"]
    win = view["cells"][:view["height"], :view["width"]]
    passes, hits = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    x0, y0 = lattice_cell(pose[0], ax, scale), lattice_cell(pose[1], ay, scale)
    for r, p in zip(ranges, points):
        kept, hit, end = gate(r, p, pose, laser)
        if not kept:
            continue
        x1, y1 = lattice_cell(end[0], ax, scale), lattice_cell(end[1], ay, scale)
        assert max(abs(x1 - x0), abs(y1 - y0)) <= MAX_WALK
        cx, cy = line_cells(x0, y0, x1, y1)
        wx, wy = cx - view["ox"], cy - view["oy"]
        inside = (wx >= 0) & (wx < view["width"]) & (wy >= 0) & (wy < view["height"])      # a cell outside the window does not exist
        passes += np.bincount(win[wy[inside], wx[inside]], minlength=256)
        state = state_at(view, x1, y1) if hit else None
        if state is not None:                                  # the end cell of a hit beam is visited twice
            passes[state] += 1
            hits[state] += 1
    out = {}
    for name, state in fr.STATES:
        out[f"pass_{name}"], out[f"hits_{name}"] = int(passes[state]), int(hits[state])
    return out


def fit(view, laser, ranges, pose, points=None):
    return fr.derive(fit_counters(view, laser, ranges, pose, points))


# ---------------------------------------------------------------- hypotheses and the answer
Hyp = namedtuple("Hyp", "index seed_cell heading coarse_mean coarse_cov coarse_response passed fine_mean fine_cov fine_response accepted")
Result = namedtuple("Result", "cells xy headings hyps accepted fits rejected_fit duplicates kept")


def match_on_map(om, params, map_points, scan, do_penalize, do_refine):
    mr.install(om, mr.rule_grid(om, scan.sensor_pose, map_points))
    return mr.match(om, scan, params, do_penalize, do_refine)


def hypothesis(index, view, map_points, ranges, laser, coarse, fine, params, gates, cells, xy, n_headings):
    from oracle import karto
    k, h = divmod(index, n_headings)
    heading = -math.pi + h * (2.0 * math.pi / n_headings)
    offset = tuple(getattr(laser, "offset", (0.0, 0.0, 0.0)))
    query = karto.Scan(ranges, rr.sensor_at((xy[k, 0], xy[k, 1], heading), offset), laser)
    cr, cm, cc = match_on_map(coarse, params, map_points, query, False, False)
    cc = np.asarray(cc).reshape(3, 3)
    passed = bool(cr > gates[0] and cc[0, 0] < gates[1] and cc[1, 1] < gates[1])
    fres, fm, fc, accepted = 0.0, np.zeros(3), np.zeros((3, 3)), False
    if passed:
        fres, fm, fc = match_on_map(fine, params, map_points, query.with_sensor_pose(cm, laser), False, True)
        fc = np.asarray(fc).reshape(3, 3)
        accepted = bool(fres >= gates[2])
    return Hyp(index, (int(cells[k, 0]), int(cells[k, 1])), float(heading), np.asarray(cm), cc, float(cr), passed, np.asarray(fm), fc, float(fres),
               accepted)


def normalize_angle(a):
    while a < -math.pi:
        a += 2.0 * math.pi
    while a > math.pi:
        a -= 2.0 * math.pi
    return a


def rank(hyps):
    """indices (positions in hyps) of the accepted ones: fine response desc, coarse response desc, index asc"""
    return sorted((k for k, h in enumerate(hyps) if h.accepted), key=lambda k: (-hyps[k].fine_response, -hyps[k].coarse_response, hyps[k].index))


def suppress(order, means, fits, min_fit_score, merge_distance, merge_heading):
    """order: positions in rank order; means / fits by position.  -> (kept, rejected by fit, duplicates), greedy"""
    kept, rejected, duplicates = [], [], []
    for k in order:
        if fits[k]["known"] > 0 and fits[k]["score"] < min_fit_score:
            rejected.append(k)
            continue
        dup = False
        if merge_distance > 0:
            for q in kept:
                dx, dy = np.float64(means[k][0]) - np.float64(means[q][0]), np.float64(means[k][1]) - np.float64(means[q][1])
                dh = normalize_angle(float(means[k][2]) - float(means[q][2]))
                if (dx * dx) + (dy * dy) < np.float64(merge_distance) * np.float64(merge_distance) and abs(dh) < merge_heading:
                    dup = True
                    break
        (duplicates if dup else kept).append(k)
    return kept, rejected, duplicates


def relocalize(view, ranges, laser, coarse, fine, params, gates, seed_spacing, n_headings, center_xy=None, radius=0.0, min_fit_score=0.0,
               merge_distance=0.05, merge_heading=0.0349, only=None):
    """coarse / fine: oracle.karto.Matcher (loop / sequential preset) made with `params`.  only: a list of hypothesis indices to run
    instead of all (the whole-map check of one index).  -> Result; `kept` etc. are positions in `hyps`"""
    cells, xy = seeds(view, seed_spacing, center_xy, radius)
    pts = mr.map_points(view)
    indices = range(cells.shape[0] * n_headings) if only is None else only
    hyps = [hypothesis(i, view, pts, ranges, laser, coarse, fine, params, gates, cells, xy, n_headings) for i in indices]
    order = rank(hyps)
    fits = {k: fit(view, laser, ranges, hyps[k].fine_mean) for k in order}
    kept, rejected, duplicates = suppress(order, {k: hyps[k].fine_mean for k in order}, fits, min_fit_score, merge_distance, merge_heading)
    return Result(cells, xy, rr.headings(n_headings), hyps, order, fits, rejected, duplicates, kept)


# ---------------------------------------------------------------- tracking
def transform_pose(p1, p2, src):
    """karto::Transform(p1, p2).TransformPose(src), Karto.h:2946-3024, in the reference's operation order (Matrix3::FromAxisAngle about
    z, Karto.h:2482-2511; Matrix3 * Pose2, :2654-2666)"""
    p1, p2, src = (tuple(float(v) for v in p) for p in (p1, p2, src))
    if p1 == p2:
        m = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        t = (0.0, 0.0, 0.0)
    else:
        s, c = sincos(p2[2] - p1[2])
        v = 1.0 - c
        axis = (0.0, 0.0, 1.0)
        m = [[0.0] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                if i == j:
                    m[i][i] = axis[i] * axis[i] * v + c
                    continue
                lo, hi = min(i, j), max(i, j)
                sym, skew = axis[lo] * axis[hi] * v, axis[3 - i - j] * s
                m[i][j] = sym + skew if (j - i + 3) % 3 == 2 else sym - skew
        if p1[0] != 0.0 or p1[1] != 0.0:
            rx = m[0][0] * p1[0] + m[0][1] * p1[1] + m[0][2] * p1[2]
            ry = m[1][0] * p1[0] + m[1][1] * p1[1] + m[1][2] * p1[2]
            t = (p2[0] - rx, p2[1] - ry, p2[2] - p1[2])
        else:
            t = (p2[0], p2[1], p2[2] - p1[2])
    rx = m[0][0] * src[0] + m[0][1] * src[1] + m[0][2] * src[2]
    ry = m[1][0] * src[0] + m[1][1] * src[1] + m[1][2] * src[2]
    return np.array([t[0] + rx, t[1] + ry, normalize_angle(src[2] + t[2])])


Step = namedtuple("Step", "predicted sensor_start response sensor_pose covariance robot_pose fit")


def track_step(view, map_points, laser, seq, params, last_robot, last_odometric, ranges, odometric):
    """one kh_map_localizer_process: -> Step; the caller carries (step.robot_pose, odometric) to the next one"""
    from oracle import karto
    offset = tuple(getattr(laser, "offset", (0.0, 0.0, 0.0)))
    predicted = transform_pose(last_odometric, last_robot, odometric)
    start = rr.sensor_at(predicted, offset)
    response, mean, cov = match_on_map(seq, params, map_points, karto.Scan(ranges, start, laser), True, True)
    return Step(predicted, start, float(response), np.asarray(mean), np.asarray(cov).reshape(3, 3), rr.robot_at(mean, offset),
                fit(view, laser, ranges, mean))
