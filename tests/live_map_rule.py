"""The live map's rule as plain numpy, independent of the library: the lattice, the window, and the expected
content of a live map taken from the occupancy oracle alone.

Lattice: a fixed anchor and resolution; the cell of a world point is o_to_int(o_round((x - anchor) * scale)) with
scale = 1 / resolution -- the operations of OccupancyGrid's WorldToGrid (Karto.h:4421-4436) with the anchor as offset.
Window: with reach = ceil(range_threshold * scale) + MARGIN, the MINIMUM window holds every cell within `reach` of every sensor
cell; the library's window is the minimum window rounded outward to multiples of BLOCK lattice cells, joined with the window it had
before (it never shrinks).

Expected content: oracle.karto.occupancy_from_scans on a grid whose offset is the anchor itself, wide and high enough for every
beam; the live window is the sub-rectangle [oy : oy + h, ox : ox + w] of it and everything outside must be zero.  That needs
non-negative cell indices, i.e. an anchor to the lower left of everything.  For an anchor INSIDE the map the oracle runs with the
anchor moved down-left by a whole number of cells, which is only the same lattice when the shift is exact in floating point and no
point sits on a rounding tie left of or below the anchor (round half AWAY from zero is not shift-invariant there):
`shift_is_exact` checks that for the very points of the test.  Ties on the negative side are checked against `trace` below, the
restatement of the walk in tests/occupancy_cases.py driven by `cells_of`."""
import math

import numpy as np

BLOCK = 64
MARGIN = 2


def align8(w):
    return (int(w) + 7) & ~7


def cells_of(xy, anchor, resolution):
    """lattice cells of world points (n, 2): round half away from zero (Math.h:87-90) of (x - anchor) * scale"""
    scale = 1.0 / resolution
    v = (np.asarray(xy, dtype=np.float64).reshape(-1, 2) - np.asarray(anchor, dtype=np.float64)) * scale
    r = np.where(v >= 0.0, np.floor(v + 0.5), np.ceil(v - 0.5))
    return r.astype(np.int64)


def reach(range_threshold, resolution):
    return int(math.ceil(range_threshold * (1.0 / resolution))) + MARGIN


def min_window(sensor_xy, anchor, resolution, range_threshold):
    """(ox, oy, width, height) of the smallest window the coverage rule allows for these sensor positions"""
    c = cells_of(sensor_xy, anchor, resolution)
    r = reach(range_threshold, resolution)
    lo, hi = c.min(axis=0) - r, c.max(axis=0) + r
    return int(lo[0]), int(lo[1]), int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)


def window(previous, sensor_xy, anchor, resolution, range_threshold):
    """the library's window after an update that traced scans at `sensor_xy` (new or moved ones; scans that stay where they
    were are inside `previous`): whole blocks around the minimum window, joined with the previous window (None = no window yet)"""
    if len(sensor_xy) == 0:
        return previous
    ox, oy, w, h = min_window(sensor_xy, anchor, resolution, range_threshold)
    x0, y0 = (ox // BLOCK) * BLOCK, (oy // BLOCK) * BLOCK
    x1, y1 = ((ox + w - 1) // BLOCK) * BLOCK + BLOCK, ((oy + h - 1) // BLOCK) * BLOCK + BLOCK
    if previous is not None and previous[2] > 0:
        px, py, pw, ph = previous
        x0, y0, x1, y1 = min(x0, px), min(y0, py), max(x1, px + pw), max(y1, py + ph)
    return x0, y0, x1 - x0, y1 - y0


def shift_is_exact(points_xy, anchor, shift_cells, resolution):
    """does moving the anchor down-left by shift_cells whole cells move every cell index of these points by exactly that?"""
    pts = np.asarray(points_xy, dtype=np.float64).reshape(-1, 2)
    pts = pts[np.isfinite(pts).all(axis=1)]
    big = np.asarray(anchor, dtype=np.float64) - np.asarray(shift_cells, dtype=np.float64) * resolution
    return bool(np.array_equal(cells_of(pts, big, resolution), cells_of(pts, anchor, resolution) + np.asarray(shift_cells, dtype=np.int64)))


def expected(win, scans, anchor, resolution, laser, min_pass_through=2, occupancy_threshold=0.1, shift_cells=(0, 0)):
    """(cells, pass, hits) of the live window `win` = (ox, oy, w, h), each (h, align8(w)) with zero padding columns, from the
    oracle alone.  scans: oracle.karto.Scan list; laser: anything with range_threshold, min_range, max_range.  Asserts that the
    oracle's counters are zero everywhere outside the window (the coverage rule) and that the window lies inside the oracle's grid.
    shift_cells: the oracle's grid starts that many cells down-left of the anchor (see shift_is_exact)."""
    from oracle import karto
    ox, oy, w, h = win
    kx, ky = int(shift_cells[0]), int(shift_cells[1])
    big = np.asarray(anchor, dtype=np.float64) - np.array([kx, ky], dtype=np.float64) * resolution
    x0, y0 = ox + kx, oy + ky                         # the window in the oracle's grid
    assert x0 >= 0 and y0 >= 0, "the oracle's grid does not reach the window: move its anchor further down-left"
    r = reach(laser.range_threshold, resolution)
    W, H = x0 + w + r + 8, y0 + h + r + 8
    if scans:
        c = cells_of(np.array([s.sensor_pose[:2] for s in scans]), big, resolution)
        assert c.min() - r >= 0, "a beam could leave the oracle's grid on the low side"
        W, H = max(W, int(c[:, 0].max()) + r + 8), max(H, int(c[:, 1].max()) + r + 8)
    cells, p, hits = karto.occupancy_from_scans(W, H, big, resolution, scans, laser, min_pass_through, occupancy_threshold)
    inside = np.zeros(p.shape, dtype=bool)
    inside[y0:y0 + h, x0:x0 + w] = True
    assert not p[~inside].any() and not hits[~inside].any(), "the oracle counts outside the window: the coverage rule does not hold"
    ws = align8(w)
    out = []
    for a in (cells, p, hits):
        b = np.zeros((h, ws), dtype=a.dtype)
        b[:, :w] = a[y0:y0 + h, x0:x0 + w]
        out.append(b)
    return tuple(out)


def trace(win, beams, anchor, resolution):
    """(pass, hits) of the live window for explicit beams [(sensor_xy, end_xy, hit)], every one kept and unclipped: cells_of +
    tests/occupancy_cases.bresenham.  For the few beams whose rounding ties the oracle cannot see from a shifted anchor."""
    import occupancy_cases as oc
    ox, oy, w, h = win
    p, hits = np.zeros((h, align8(w)), dtype=np.uint32), np.zeros((h, align8(w)), dtype=np.uint32)
    for sensor, end, hit in beams:
        (x0, y0), (x1, y1) = (int(v) for v in cells_of(sensor, anchor, resolution)[0]), (int(v) for v in cells_of(end, anchor, resolution)[0])
        for cx, cy in oc.bresenham(x0, y0, x1, y1):
            p[cy - oy, cx - ox] += 1
        if hit:
            p[y1 - oy, x1 - ox] += 1
            hits[y1 - oy, x1 - ox] += 1
    return p, hits
