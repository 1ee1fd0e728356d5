"""Edge inputs of the occupancy grid as plain numpy data, independent of the library: what tests/test_edge_cases_oracle.py
runs through the oracle alone (does every case still reach the edge its name says?) and tests/test_occupancy_edges_gpu.py
through kh_occupancy_* next to the oracle.

A case is (name, width, height, offset, resolution, gates, scans, min_pass, threshold, probe):
  gates   what karto.occupancy_from_scans / OccupancyGrid.AddScans read from a laser (min_range, range_threshold, max_range);
  scans   [(sensor_xy, ranges, points)]: range and point readings are set independently, the way AddScan reads them
          (Karto.h:6148-6189: the range decides drop / clip / hit, the point is where the beam goes);
  probe   what the CPU check needs to know about the case (named cells, expected counts).

Resolutions are powers of two and offsets multiples of them, so that `cell * resolution + offset` is exact and a reading can be
put exactly on a rounding tie.  Every point reading of a KEPT beam is finite and a few hundred cells from the grid at most: a
non-finite point with a valid range sends the reference's (and the library's) Bresenham walk over 2^31 cells."""
from collections import namedtuple

import numpy as np

Gates = namedtuple("Gates", "min_range range_threshold max_range")
Case = namedtuple("Case", "name width height offset resolution gates scans min_pass threshold probe")

GATES = Gates(0.1, 20.0, 30.0)
HIT = 1.0                                   # a reading that is kept, not clipped, and marks its end cell
NO_HIT = GATES.range_threshold - 1e-06      # kept, not clipped, but not `< range_threshold - 1e-06`: traced without a hit


def align8(w):
    return (int(w) + 7) & ~7


def world(offset, resolution, cells):
    """centre coordinates of grid cells (fractions allowed)"""
    return np.asarray(offset, dtype=np.float64) + np.asarray(cells, dtype=np.float64) * resolution


def beams(offset, resolution, sensor_cell, end_cells, ranges=HIT):
    """one scan: a sensor cell, end cells, and one range for all beams or one per beam"""
    end_cells = np.asarray(end_cells, dtype=np.float64).reshape(-1, 2)
    r = np.broadcast_to(np.asarray(ranges, dtype=np.float64), (end_cells.shape[0],)).copy()
    return world(offset, resolution, sensor_cell), r, np.ascontiguousarray(world(offset, resolution, end_cells))


def ring(centre, radius):
    """every cell at Chebyshev distance `radius` from `centre`"""
    cx, cy = centre
    if radius == 0:
        return [(cx, cy)]
    out = []
    for d in range(-radius, radius + 1):
        out += [(cx + d, cy - radius), (cx + d, cy + radius)]
    for d in range(-radius + 1, radius):
        out += [(cx - radius, cy + d), (cx + radius, cy + d)]
    return out


def bresenham(x0, y0, x1, y1):
    """Grid<T>::TraceLine (Karto.h:4874-4927) restated a second time: the cells one beam visits, in order"""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, x1, y0, y1 = x1, x0, y1, y0
    dx, dy, err, y, cells = x1 - x0, abs(y1 - y0), 0, y0, []
    for x in range(x0, x1 + 1):
        cells.append((y, x) if steep else (x, y))
        err += dy
        if 2 * err >= dx:
            y += 1 if y0 < y1 else -1
            err -= dx
    return cells


# ---------------------------------------------------------------- beams that leave the grid
def leaving_cases():
    w, h, res, off = 13, 11, 0.5, (-2.0, 3.0)              # width step 16: three padding columns
    c = (6, 5)
    yield Case("leaving: sensor inside, beams out through every edge and corner", w, h, off, res, GATES,
               [beams(off, res, c, ring(c, 30))], 2, 0.1, dict(borders=True, no_hits=True))
    crossing = [beams(off, res, (-10, 5), [(30, y) for y in range(-6, 18)]), beams(off, res, (6, -9), [(x, 25) for x in range(-4, 18)]),
                # the exact diagonals through the four corner cells (0, 0), (12, 10), (12, 0), (0, 10)
                beams(off, res, (-5, -5), [(20, 20)]), beams(off, res, (-1, -3), [(25, 23)]), beams(off, res, (19, -7), [(-8, 20)]),
                beams(off, res, (17, -7), [(-8, 18)])]
    yield Case("leaving: sensor outside, beams crossing", w, h, off, res, GATES, crossing, 2, 0.1, dict(borders=True, no_hits=True))
    outside = [beams(off, res, (-9, -9), [(-1, y) for y in range(-9, 25)] + [(x, -1) for x in range(-9, 25)]),
               beams(off, res, (30, 30), [(13, y) for y in range(-5, 30)] + [(x, 11) for x in range(-5, 30)] + [(13, 11), (40, 2)]),
               beams(off, res, (-1, 11), [(-1, 11)]), beams(off, res, (13, -1), [(13, -1)])]
    yield Case("leaving: beams wholly outside", w, h, off, res, GATES, outside, 2, 0.1, dict(all_zero=True))
    ends = [(13, 5), (-1, 5), (6, 11), (6, -1), (13, 11), (-1, -1), (15, 5), (14, 10)]     # (15, 5), (14, 10): in the padding columns
    yield Case("leaving: valid end point outside", w, h, off, res, GATES, [beams(off, res, c, ends)], 2, 0.1,
               dict(no_hits=True, passed=[(12, 5), (0, 5), (6, 10), (6, 0)]))
    # round half away from zero (Math.h:87-90): -1.5 -> -2, -0.5 -> -1, +0.5 -> 1.  floor(v + 0.5) would give -1, 0, 1.
    half = [beams(off, res, (-1.5, 2.5), [(0.5, 2.5), (-0.5, 2.5), (-1.5, 2.5)]),
            beams(off, res, (2.5, -1.5), [(2.5, 0.5), (2.5, -0.5), (2.5, -1.5)]),
            beams(off, res, (-0.5, -0.5), [(0.5, 0.5), (-0.5, -0.5), (-1.5, -1.5)])]
    yield Case("leaving: negative indices, readings on rounding ties", w, h, off, res, GATES, half, 0, 0.1,
               dict(counts={(0, 3): (1, 0), (1, 3): (2, 1), (3, 0): (1, 0), (3, 1): (2, 1), (0, 0): (1, 0), (1, 1): (2, 1),
                            (0, 2): (0, 0), (2, 0): (0, 0)}))


# ---------------------------------------------------------------- every direction from one cell
def direction_cases():
    w, h, res, off = 91, 91, 0.25, (-11.25, -11.25)        # width step 96
    c = (45, 45)
    star = [beams(off, res, c, ring(c, r)) for r in (0, 1, 2, 7, 40)]
    yield Case("directions: star of beams, radius 0, 1, 2, 7, 40", w, h, off, res, GATES, star, 2, 0.1, dict(star=c))
    # the same star from a corner of a small grid: three quarters of it leave, some of it through the padding columns
    w2, h2 = 43, 41
    c2 = (40, 2)
    yield Case("directions: star from a corner, clipped by the grid", w2, h2, off, res, GATES, [beams(off, res, c2, ring(c2, r)) for r in (0, 1, 2, 7, 40)],
               2, 0.1, dict(star=c2))


# ---------------------------------------------------------------- range gates
def gate_values(g=GATES):
    """(label, reading, kept, hit): what Karto.h:6167-6180 does with the reading"""
    na, inf = np.nextafter, np.inf
    edge = g.range_threshold - 1e-06
    return [
        ("min_range", g.min_range, False, False), ("below min_range", na(g.min_range, -inf), False, False),
        ("above min_range", na(g.min_range, inf), True, True), ("ordinary", 7.25, True, True),
        ("below range_threshold - 1e-6", na(edge, -inf), True, True), ("range_threshold - 1e-6", edge, True, False),
        ("above range_threshold - 1e-6", na(edge, inf), True, False), ("below range_threshold", na(g.range_threshold, -inf), True, False),
        ("range_threshold", g.range_threshold, True, False), ("between threshold and max_range", 25.0, True, False),
        ("below max_range", na(g.max_range, -inf), True, False), ("max_range", g.max_range, False, False),
        ("above max_range", na(g.max_range, inf), False, False), ("NaN", np.nan, False, False), ("+inf", inf, False, False),
        ("-inf", -inf, False, False), ("zero", 0.0, False, False), ("negative", -3.0, False, False),
    ]


def gate_cases():
    res, off = 0.0625, (0.0, 0.0)                          # 20 m = 320 cells
    vals = gate_values()
    w, h = 490, 2 * len(vals) + 1                          # width step 496; row 2 k + 1 belongs to reading k
    scans, rows = [], {}
    for k, (label, r, kept, hit) in enumerate(vals):
        sensor = world(off, res, (2, 2 * k + 1))
        # a kept beam points along +x to where its reading says; a dropped one carries a NaN point (never converted).
        # NB a kernel that wrongly KEEPS a dropped reading would not fail on this case by assertion but walk 2^31 cells: the GPU
        # test runs finite_twin(case) first, which catches it by assertion
        pt = sensor + np.array([r, 0.0]) if kept else np.array([np.nan, np.nan])
        scans.append((sensor, np.array([r]), pt.reshape(1, 2)))
        rows[label] = (2 * k + 1, kept, hit)
    yield Case("gates: one beam per gate value", w, h, off, res, GATES, scans, 0, 0.1, dict(gate_rows=rows, sensor_x=2))
    # all of them as ONE scan from one sensor, fanned out, each reading three times
    sensor = world(off, res, (2, 1))
    r = np.repeat(np.array([v[1] for v in vals]), 3)
    kept = np.repeat(np.array([v[2] for v in vals]), 3)
    ang = np.linspace(0.0, 0.11, r.size)
    with np.errstate(invalid="ignore"):
        pts = sensor + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    pts[~kept] = np.nan
    yield Case("gates: all readings in one scan", w, h, off, res, GATES, [(sensor, r, pts)], 2, 0.1, dict(some_hits=True))
    # a narrow grid that the clipped beams leave: the clip is applied before the grid test, not after
    yield Case("gates: clipped beams in a narrow grid", 203, h, off, res, GATES, scans, 0, 0.1, dict(some_hits=True))


# ---------------------------------------------------------------- grid and call shapes
SHAPE_BEAMS = (0, 1, 63, 64, 65, 255, 256, 257, 1081)


def _shape_scans(w, h, off, res, counts):
    scans = []
    for s, n in enumerate(counts):
        k = np.arange(n)
        ends = np.stack([(k * 37 + s) % (w + 4) - 2, k % (h + 2) - 1], axis=1)
        r = np.where(k % 5 == 4, NO_HIT, HIT)
        scans.append(beams(off, res, ((7 * s) % (w + 2) - 1, s % h), ends, r))
    return scans


def shape_cases():
    res, off = 0.5, (1.0, -0.5)
    for w in (1, 7, 8, 9, 4095):
        for h in (1, 3):
            yield Case(f"shapes: {w} x {h}, scans of {SHAPE_BEAMS} beams", w, h, off, res, GATES, _shape_scans(w, h, off, res, SHAPE_BEAMS),
                       2, 0.1, dict(some_hits=True, beams=sum(SHAPE_BEAMS)))
    n = 300
    dropped = (world(off, res, (3, 1)), np.tile([np.nan, 0.0, GATES.max_range, -1.0, GATES.min_range, np.inf], n // 6), np.full((n, 2), np.nan))
    yield Case("shapes: every beam of the call dropped", 9, 3, off, res, GATES, [dropped, dropped], 2, 0.1, dict(all_zero=True))
    yield Case("shapes: no scans", 9, 3, off, res, GATES, [], 2, 0.1, dict(all_zero=True))
    yield Case("shapes: scans without beams", 9, 3, off, res, GATES, _shape_scans(9, 3, off, res, (0, 0)), 2, 0.1, dict(all_zero=True))


# ---------------------------------------------------------------- Update: cells exactly on the two comparisons
# cell -> (pass, hits).  A zero-length beam adds (2, 1) to its cell when its end is valid and (1, 0) when it is not, so every
# pair with 2 * hits <= pass can be made -- and no other: a hit always comes with two passes, hits / pass never exceeds 0.5.
UPDATE_COUNTS = {
    (0, 0): (0, 0), (1, 0): (1, 0), (2, 0): (2, 0), (3, 0): (2, 1), (4, 0): (3, 0), (5, 0): (3, 1), (6, 0): (4, 0), (7, 0): (4, 2), (8, 0): (4, 1),
    (0, 1): (10, 1), (1, 1): (10, 2), (2, 1): (10, 0), (3, 1): (8, 2), (4, 1): (8, 3), (5, 1): (20, 2), (6, 1): (20, 3), (7, 1): (6, 3), (8, 1): (5, 2),
    (0, 2): (30, 3), (1, 2): (30, 4), (2, 2): (40, 20), (3, 2): (41, 20),
}
UPDATE_MIN_PASS = (0, 2, 3)
UPDATE_THRESHOLDS = (0.0, 0.1, 0.5, 1.0)


def update_scans(off, res):
    scans = []
    for cell, (p, hits) in UPDATE_COUNTS.items():
        r = [HIT] * hits + [NO_HIT] * (p - 2 * hits)
        if r:
            scans.append(beams(off, res, cell, [cell] * len(r), r))
    return scans


def expected_state(p, hits, min_pass, threshold):
    """Karto.h:6240-6258 on one cell, in Python's own IEEE division"""
    if not p > min_pass:
        return 0
    return 100 if hits / p > threshold else 255


def update_cases():
    w, h, res, off = 9, 3, 0.5, (4.0, 4.0)
    scans = update_scans(off, res)
    for mp in UPDATE_MIN_PASS:
        for th in UPDATE_THRESHOLDS:
            yield Case(f"update: min_pass_through {mp}, threshold {th}", w, h, off, res, GATES, scans, mp, th, dict(counts=UPDATE_COUNTS, update=True))


# ---------------------------------------------------------------- contention and reuse
CONTENTION_BEAMS = 50000


def contention_case():
    w, h, res, off = 9, 3, 0.5, (0.0, 0.0)
    scans = [beams(off, res, (1, 1), [(6, 1)] * 25000), beams(off, res, (1, 1), [(6, 1)] * 24999), beams(off, res, (1, 1), [(6, 1)])]
    n = CONTENTION_BEAMS
    counts = {(1, 1): (n, 0), (3, 1): (n, 0), (6, 1): (2 * n, n), (7, 1): (0, 0), (1, 0): (0, 0)}
    return Case("contention: 50 000 beams between two cells", w, h, off, res, GATES, scans, 2, 0.1, dict(counts=counts))


def reuse_steps():
    """(width, height, offset, resolution, steps); a step is ("add", scans) or ("clear", None).  The second call carries 20 x the
    beams of the first (the staging buffers regrow), the third fits the grown buffers, the last repeats the first on a cleared grid."""
    w, h, res, off = 29, 17, 0.5, (-3.0, 2.0)
    small = _shape_scans(w, h, off, res, (40, 24))
    large = _shape_scans(w, h, off, res, (1081, 199))[::-1]
    other = _shape_scans(w, h, off, res, (3, 0, 17))
    assert sum(s[1].size for s in large) == 20 * sum(s[1].size for s in small)
    return w, h, off, res, [("add", small), ("add", large), ("add", other), ("clear", None), ("add", small)]


def finite_twin(case):
    """the case with every non-finite point replaced by a point 1 m from the sensor, or None if all its points are finite.  Run
    BEFORE the case itself: a kernel that wrongly keeps a dropped reading differs from the oracle on the twin and fails by
    assertion, where the case itself would send it over 2^31 cells"""
    if all(np.isfinite(p).all() for _, _, p in case.scans):
        return None
    scans = []
    for s, r, p in case.scans:
        p = p.copy()
        p[~np.isfinite(p).all(axis=1)] = np.asarray(s) + np.array([1.0, 0.0])
        scans.append((s, r, p))
    return case._replace(name=case.name + " (finite twin)", scans=scans)


def all_cases():
    for gen in (leaving_cases, direction_cases, gate_cases, shape_cases, update_cases):
        yield from gen()
    yield contention_case()
