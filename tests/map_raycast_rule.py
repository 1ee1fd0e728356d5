"""TEST INFRASTRUCTURE (not a test): the rule of kh_map_raycast in numpy on the CPU oracle -- the scan a map
would produce at a sensor pose.  It reads nothing of the library; lattice, states and TraceLine's closed form are
tests/map_localize_rule.py's.

  direction   beam b of sensor pose p runs to the far point: the oracle's scan_points of readings that are all range_threshold at p
  line        c0 = lattice cell of the sensor's (x, y), c1 = lattice cell of the far point; the beam's cells are exactly the set
              TraceLine(c0, c1) visits (line_cells), ordered by s = |long-axis coordinate - c0's|, s = 0 .. L
  states      a window cell of state 100 is occupied, of state 255 free; every other state and a cell outside the window is unknown
  walk        ascending s, counter unk: occupied -> HIT; unknown -> unk += 1, then UNKNOWN if max_unknown >= 0 and unk > max_unknown;
              the end of the line -> FREE with cell c1 and s = L
  range       HIT: dx = (anchor x + float(i) / scale) - sx, dy likewise, sqrt((dx * dx) + (dy * dy)); else no_return
  no_return   default: nextafter(range_threshold, inf) where that is below max_range, else NaN
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_localize_rule as ml

FREE, HIT, UNKNOWN = 0, 1, 2
OCCUPIED_STATE, FREE_STATE = 100, 255
Cast = namedtuple("Cast", "ranges codes cells steps")


def default_no_return(laser):
    above = float(np.nextafter(np.float64(laser.range_threshold), np.inf))
    return above if above < laser.max_range else math.nan


def far_points(laser, pose):
    from oracle import karto
    return karto.scan_points(np.full(laser.n_beams, laser.range_threshold, dtype=np.float64), np.asarray(pose, dtype=np.float64), laser)


def beam_cells(c0, c1):
    """the cells of TraceLine(c0, c1) outward from c0: (x, y) int64 arrays of length L + 1, entry s at distance s on the long axis"""
    x, y = ml.line_cells(c0[0], c0[1], c1[0], c1[1])
    steep = abs(c1[1] - c0[1]) > abs(c1[0] - c0[0])
    s = np.abs((y if steep else x) - (c0[1] if steep else c0[0]))
    order = np.argsort(s, kind="stable")
    assert np.array_equal(s[order], np.arange(s.size)), "s is unique per cell"
    return x[order], y[order]


def walk(view, c0, c1, max_unknown):
    """-> (cell i, cell j, s, code)"""
    x, y = beam_cells(c0, c1)
    wx, wy = x - view["ox"], y - view["oy"]
    inside = (wx >= 0) & (wx < view["width"]) & (wy >= 0) & (wy < view["height"])
    state = np.zeros(x.size, dtype=np.int64)
    state[inside] = view["cells"][wy[inside], wx[inside]]
    occupied = state == OCCUPIED_STATE
    unknown = ~occupied & (state != FREE_STATE)
    unk = np.cumsum(unknown)
    stop_hit = np.nonzero(occupied)[0]
    stop_unk = np.nonzero(unknown & (unk > max_unknown))[0] if max_unknown >= 0 else np.zeros(0, dtype=np.int64)
    s_hit = int(stop_hit[0]) if stop_hit.size else x.size
    s_unk = int(stop_unk[0]) if stop_unk.size else x.size
    if s_hit == x.size and s_unk == x.size:
        return int(c1[0]), int(c1[1]), x.size - 1, FREE
    s, code = (s_hit, HIT) if s_hit < s_unk else (s_unk, UNKNOWN)      # (one cell is never both)
    return int(x[s]), int(y[s]), s, code


def cast_refused(view, laser, pose, max_unknown):
    return max_unknown < -1 or ml.fit_refused(view, laser, pose)


def cast(view, laser, pose, max_unknown=-1, no_return=None):
    """one sensor pose -> Cast (ranges (n,) float64, codes (n,), cells (n, 2), steps (n,))"""
    pose = np.asarray(pose, dtype=np.float64)
    assert not cast_refused(view, laser, pose, max_unknown)
    if no_return is None:
        no_return = default_no_return(laser)
    ax, ay, scale = view["anchor"][0], view["anchor"][1], view["scale"]
    c0 = (ml.lattice_cell(pose[0], ax, scale), ml.lattice_cell(pose[1], ay, scale))
    n = laser.n_beams
    ranges, codes = np.full(n, no_return, dtype=np.float64), np.zeros(n, dtype=np.int32)
    cells, steps = np.zeros((n, 2), dtype=np.int32), np.zeros(n, dtype=np.int32)
    for b, p in enumerate(far_points(laser, pose)):
        c1 = (ml.lattice_cell(p[0], ax, scale), ml.lattice_cell(p[1], ay, scale))
        i, j, s, code = walk(view, c0, c1, max_unknown)
        cells[b], steps[b], codes[b] = (i, j), s, code
        if code == HIT:
            dx = (np.float64(ax) + np.float64(i) / np.float64(scale)) - pose[0]
            dy = (np.float64(ay) + np.float64(j) / np.float64(scale)) - pose[1]
            ranges[b] = np.sqrt((dx * dx) + (dy * dy))
    return Cast(ranges, codes, cells, steps)


def cast_poses(view, laser, poses, max_unknown=-1, no_return=None):
    """(n_poses, 3) -> Cast of arrays with a leading pose axis"""
    parts = [cast(view, laser, pose, max_unknown, no_return) for pose in np.asarray(poses, dtype=np.float64).reshape(-1, 3)]
    return Cast(*(np.stack([getattr(p, f) for p in parts]) for f in Cast._fields))
