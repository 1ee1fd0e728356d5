"""TEST INFRASTRUCTURE (not a test): the rule of kh_map_merge_*  in numpy -- one finished map warped through a
rigid correction onto another map's lattice, the two composed cell by cell, the overlap counted.  It reads nothing of the library;
lattice, states and windows are tests/map_localize_rule.py's, the corrections tests/merge_rule.py's.  Every double operation below is
one IEEE operation, in the order written.

  lattice     the output lives on the TARGET's lattice (anchor, scale); lattice index I lies at anchor + float(I) / scale
  correction  C carries moving-map coordinates into the target's frame; Cinv = inverse(C), c, s = cos, sin of its yaw, each called on
              its own; a point goes through as (c * x - s * y) + tx, (s * x + c * y) + ty
  warp        output cell (I, J), footprint n: the n x n sample points (wx + d_a, wy + d_b), d_k = ((2 k + 1 - n) / (2.0 n)) / scale_t;
              each carried by Cinv, rounded to a moving-lattice cell (lattice_cell), read there; a cell outside the moving window, or
              with an index beyond the int32 lattice (lattice_cell's -2^31), reads unknown.  M = 100 if any sample read 100, else 255
              if any read 255, else 0
  compose     T = the target's state at (I, J), 100 or 255, else (any other state, no such cell) unknown; code and merged cell by the
              table of compose(); a conflict by the policy
  counters    target_only, moving_only, agree_free, agree_occupied, conflict_moving_occupied, conflict_moving_free over the output
              window; overlap = the last four; agreement = float(agree_free + agree_occupied) / float(overlap), 0.0 without overlap
  window      grow 0: the target's window.  grow 1: its union with the carried box of the moving map's cells of state != 0 -- the
              inclusive lattice box of those cells, its corner points anchor_m + float(idx) / scale_m pushed outward by 0.5 / scale_m,
              carried by C, rounded to target-lattice cells, min / max over the four, one cell of padding on every side
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_localize_rule as ml
import merge_rule

UNKNOWN, OCCUPIED, FREE = 0, 100, 255
NEITHER, TARGET_ONLY, MOVING_ONLY, AGREE, MOVING_OCCUPIED, MOVING_FREE = range(6)
CONFLICT_TARGET, CONFLICT_MOVING, CONFLICT_OCCUPIED, CONFLICT_UNKNOWN = range(4)
COUNTERS = ("target_only", "moving_only", "agree_free", "agree_occupied", "conflict_moving_occupied", "conflict_moving_free")
MAX_CORNER, MAX_SIDE, MAX_CELLS = 1 << 30, 32768, 1 << 28
NO_CELL = -2 ** 31
Window = namedtuple("Window", "ox oy width height width_step")
Merged = namedtuple("Merged", "window footprint known_box cells codes counters overlap agreement view")


class Refused(ValueError):
    """where the library answers KH_ERR_INVALID_ARG; code: 0 the arguments, 1 / 2 / 3 the three refusals of the output window"""

    def __init__(self, text, code=0):
        super().__init__(text)
        self.code = code


def sample_offsets(n, scale_t):
    return [float((np.float64(2 * k + 1 - n) / (np.float64(2.0) * np.float64(n))) / np.float64(scale_t)) for k in range(n)]


def default_footprint(scale_m, scale_t):
    with np.errstate(over="ignore"):
        return int(min(4.0, max(1.0, float(np.ceil(np.float64(scale_m) / np.float64(scale_t))))))


def carry(t, x, y):
    """merge_rule.transform_point on arrays: (c * x - s * y) + tx, (s * x + c * y) + ty"""
    c, s = merge_rule.cos_sin(t[2])
    c, s = np.float64(c), np.float64(s)
    with np.errstate(invalid="ignore", over="ignore"):
        return (c * x - s * y) + np.float64(t[0]), (s * x + c * y) + np.float64(t[1])


def lattice_cells(v, anchor, scale):
    """ml.lattice_cell on an array -> int64; -2^31 where the index leaves the int32 lattice"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = ml.o_round((np.asarray(v, dtype=np.float64) - np.float64(anchor)) * np.float64(scale))
        ok = (r > -2147483649.0) & (r < 2147483648.0)
    return np.where(ok, r, float(NO_CELL)).astype(np.int64)


def states_at(view, cx, cy):
    """ml.state_at on arrays: the raw state, 0 where the cell does not exist"""
    wx, wy = cx - view["ox"], cy - view["oy"]
    inside = (cx != NO_CELL) & (cy != NO_CELL) & (wx >= 0) & (wx < view["width"]) & (wy >= 0) & (wy < view["height"])
    out = np.zeros(cx.shape, dtype=np.int64)
    out[inside] = view["cells"][wy[inside], wx[inside]]
    return out


def known_box(view):
    """(i0, j0, i1, j1) of the cells of state != 0, lattice indices, inclusive; None without one"""
    j, i = np.nonzero(view["cells"][:view["height"], :view["width"]] != UNKNOWN)
    if i.size == 0:
        return None
    return int(i.min()) + view["ox"], int(j.min()) + view["oy"], int(i.max()) + view["ox"], int(j.max()) + view["oy"]


def align8(w):
    return (int(w) + 7) & ~7


def output_window(target, moving, correction, grow=1, box="find"):
    """-> Window; Refused for a carried corner beyond +-2^30 cells, a side above 32768 cells, more than 2^28 cells"""
    x0, y0, x1, y1 = target["ox"], target["oy"], target["ox"] + target["width"], target["oy"] + target["height"]
    if box == "find":
        box = known_box(moving)
    if grow and box is not None:
        half = np.float64(0.5) / np.float64(moving["scale"])
        lo_x = (np.float64(moving["anchor"][0]) + np.float64(box[0]) / np.float64(moving["scale"])) - half
        lo_y = (np.float64(moving["anchor"][1]) + np.float64(box[1]) / np.float64(moving["scale"])) - half
        hi_x = (np.float64(moving["anchor"][0]) + np.float64(box[2]) / np.float64(moving["scale"])) + half
        hi_y = (np.float64(moving["anchor"][1]) + np.float64(box[3]) / np.float64(moving["scale"])) + half
        ci, cj = [], []
        for x, y in ((lo_x, lo_y), (hi_x, lo_y), (lo_x, hi_y), (hi_x, hi_y)):
            px, py = merge_rule.transform_point(correction, float(x), float(y))
            with np.errstate(invalid="ignore", over="ignore"):
                ri = float(ml.o_round((np.float64(px) - np.float64(target["anchor"][0])) * np.float64(target["scale"])))
                rj = float(ml.o_round((np.float64(py) - np.float64(target["anchor"][1])) * np.float64(target["scale"])))
            if not (abs(ri) <= MAX_CORNER and abs(rj) <= MAX_CORNER):
                raise Refused("a carried corner leaves +-2^30 cells", 1)
            ci.append(int(ri))
            cj.append(int(rj))
        x0, y0 = min(x0, min(ci) - 1), min(y0, min(cj) - 1)
        x1, y1 = max(x1, max(ci) + 2), max(y1, max(cj) + 2)
    width, height = x1 - x0, y1 - y0
    if width > MAX_SIDE or height > MAX_SIDE:
        raise Refused("an output side above 32768 cells", 2)
    if width * height > MAX_CELLS:
        raise Refused("an output above 2^28 cells", 3)
    return Window(x0, y0, width, height, align8(width))


def warp(window, target, moving, correction, footprint):
    """-> M (height, width) int64 of 0 / 100 / 255: the moving map on the cells of `window` of the target's lattice"""
    inv = merge_rule.inverse(correction)
    i = np.arange(window.ox, window.ox + window.width, dtype=np.int64)
    j = np.arange(window.oy, window.oy + window.height, dtype=np.int64)
    wx = np.float64(target["anchor"][0]) + i.astype(np.float64) / np.float64(target["scale"])
    wy = np.float64(target["anchor"][1]) + j.astype(np.float64) / np.float64(target["scale"])
    d = sample_offsets(footprint, target["scale"])
    occupied = np.zeros((window.height, window.width), dtype=bool)
    free = np.zeros((window.height, window.width), dtype=bool)
    for b in range(footprint):
        for a in range(footprint):
            sx, sy = np.meshgrid(wx + np.float64(d[a]), wy + np.float64(d[b]))
            px, py = carry(inv, sx, sy)
            state = states_at(moving, lattice_cells(px, moving["anchor"][0], moving["scale"]), lattice_cells(py, moving["anchor"][1], moving["scale"]))
            occupied |= state == OCCUPIED
            free |= state == FREE
    return np.where(occupied, OCCUPIED, np.where(free, FREE, UNKNOWN)).astype(np.int64)


def compose(t, m, conflict):
    """T and M arrays of 0 / 100 / 255 -> (codes, merged cells)"""
    codes = np.full(t.shape, NEITHER, dtype=np.int64)
    cells = np.zeros(t.shape, dtype=np.int64)
    tk, mk = t != UNKNOWN, m != UNKNOWN
    only_t, only_m, agree = tk & ~mk, mk & ~tk, tk & mk & (t == m)
    m_occ, m_free = (t == FREE) & (m == OCCUPIED), (t == OCCUPIED) & (m == FREE)
    codes[only_t], cells[only_t] = TARGET_ONLY, t[only_t]
    codes[only_m], cells[only_m] = MOVING_ONLY, m[only_m]
    codes[agree], cells[agree] = AGREE, t[agree]
    codes[m_occ], codes[m_free] = MOVING_OCCUPIED, MOVING_FREE
    both = m_occ | m_free
    cells[both] = {CONFLICT_TARGET: t, CONFLICT_MOVING: m, CONFLICT_OCCUPIED: np.full(t.shape, OCCUPIED), CONFLICT_UNKNOWN: np.zeros(t.shape, dtype=np.int64)}[
        conflict][both]
    return codes, cells


def count(t, codes):
    n = {"target_only": int((codes == TARGET_ONLY).sum()), "moving_only": int((codes == MOVING_ONLY).sum()),
         "agree_free": int(((codes == AGREE) & (t == FREE)).sum()), "agree_occupied": int(((codes == AGREE) & (t == OCCUPIED)).sum()),
         "conflict_moving_occupied": int((codes == MOVING_OCCUPIED).sum()), "conflict_moving_free": int((codes == MOVING_FREE).sum())}
    overlap = n["agree_free"] + n["agree_occupied"] + n["conflict_moving_occupied"] + n["conflict_moving_free"]
    return n, overlap, agreement(n["agree_free"], n["agree_occupied"], overlap)


def agreement(agree_free, agree_occupied, overlap):
    return float(np.float64(agree_free + agree_occupied) / np.float64(overlap)) if overlap else 0.0


def merge(target, moving, correction, footprint=0, conflict=CONFLICT_OCCUPIED, grow=1):
    """target, moving: view dicts (tests/map_match_rule.view_dict) -> Merged; its cells and codes have the row stride of the output, the
    padding 0; its view is a view dict of the merged cells on the target's lattice"""
    correction = tuple(float(v) for v in correction)
    if not all(math.isfinite(v) for v in correction) or footprint not in range(5) or conflict not in range(4) or grow not in (0, 1):
        raise Refused("arguments")
    n = footprint or default_footprint(moving["scale"], target["scale"])
    box = known_box(moving)
    window = output_window(target, moving, correction, grow, box)
    i = np.arange(window.ox, window.ox + window.width, dtype=np.int64)
    j = np.arange(window.oy, window.oy + window.height, dtype=np.int64)
    raw = states_at(target, *np.meshgrid(i, j))
    t = np.where((raw == OCCUPIED) | (raw == FREE), raw, UNKNOWN)
    m = warp(window, target, moving, correction, n)
    codes, cells = compose(t, m, conflict)
    counters, overlap, agree = count(t, codes)
    out_cells = np.zeros((window.height, window.width_step), dtype=np.uint8)
    out_codes = np.zeros((window.height, window.width_step), dtype=np.uint8)
    out_cells[:, :window.width], out_codes[:, :window.width] = cells, codes
    view = dict(cells=out_cells, anchor=(float(target["anchor"][0]), float(target["anchor"][1])), scale=float(target["scale"]), ox=window.ox, oy=window.oy,
                width=window.width, height=window.height)
    return Merged(window, n, box if box is not None else (0, 0, -1, -1), out_cells, out_codes, counters, overlap, agree, view)
