"""Edge inputs of the map localizer's two kernels (k_map_seeds, k_map_fit in csrc/occupancy_map.hip) as plain numpy data, and the small
map its end-to-end tests share.  tests/test_map_localize_rule_oracle.py checks on the CPU that every case sits on the edge its name
says (Case.check, fed with tests/map_localize_rule.py's answer); tests/test_map_seeds_gpu.py and tests/test_map_fit_gpu.py ask the
library for the same cases and compare exactly.  Scales are powers of two and anchors multiples of the cell where a case needs an
exact rounding tie."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_localize_rule as rule
import map_match_rule as mr
import relocalize_cases as rc

U, O, F = 0, 100, 255                                       # unknown, occupied, free
SeedCase = namedtuple("SeedCase", "name view spacing center radius check")
FitCase = namedtuple("FitCase", "name view laser ranges poses check")
CaseLaser = namedtuple("CaseLaser", "n_beams min_angle ang_res min_range max_range range_threshold")


def align8(w):
    return (int(w) + 7) & ~7


def view_of(cells, anchor, scale, ox=0, oy=0, padding=U):
    """cells (h, w) -> a view dict whose array has the row stride align8(w), the padding columns filled with `padding`"""
    cells = np.asarray(cells, dtype=np.uint8)
    h, w = cells.shape
    buf = np.full((h, align8(w)), padding, dtype=np.uint8)
    buf[:, :w] = cells
    return mr.view_dict(buf, anchor, scale, ox, oy, w)


def random_cells(rng, h, w, p_free=0.3, p_occ=0.1):
    return rng.choice(np.array([U, O, F], dtype=np.uint8), size=(h, w), p=[1.0 - p_free - p_occ, p_occ, p_free])


# ---------------------------------------------------------------- seeds
def seed_cases():
    out = []
    rng = np.random.default_rng(11)
    a, k = (0.5, -0.25), 20.0

    def add(name, view, spacing, check, center=None, radius=0.0):
        out.append(SeedCase(name, view, spacing, center, radius, check))

    cells = random_cells(rng, 9, 13)

    def every_free(c, xy, cells=cells):
        j, i = np.nonzero(cells == F)
        assert np.array_equal(c, np.stack([i, j], axis=1)), "row-major: ascending (by, bx) with one cell per block"
    add("pitch 1: every free cell is a seed", view_of(cells, a, k), 0.01, every_free)

    cells = random_cells(rng, 7, 10)
    cells[6, 9] = U
    cells[5, 9] = F

    def one_block(c, xy):
        assert c.tolist() == [[9, 5]], "the free cell nearest to the centre (50, 50) of the one block"
    add("pitch larger than the map", view_of(cells, a, k), 101 / k, one_block)

    big = random_cells(rng, 135, 140)
    for p in (63, 65, 129):
        def many(c, xy, p=p):
            nx, ny = -(-140 // p), -(-135 // p)
            assert c.shape[0] == nx * ny and rule.pitch_of(p / k, k) == p
        add(f"pitch {p}: more cells than a wave's first pass", view_of(big, a, k), p / k, many)
    # one free cell per block, anywhere in it: the minimum comes from any pass and any lane
    lone = np.full((130, 130), O, dtype=np.uint8)
    where = []
    for by in range(2):
        for bx in range(2):
            i, j = int(rng.integers(0, 65)), int(rng.integers(0, 65))
            lone[by * 65 + j, bx * 65 + i] = F
            where.append([bx * 65 + i, by * 65 + j])

    def lone_cells(c, xy, where=where):
        assert c.tolist() == where
    add("pitch 65: one free cell per block", view_of(lone, a, k), 65 / k, lone_cells)

    for w in (63, 64, 65):
        row = random_cells(rng, 1, w, p_free=0.5)

        def strip(c, xy, w=w):
            assert c.shape[0] == -(-w // 31) and (c[:, 1] == 0).all()
        add(f"a window of width {w} and height 1", view_of(row, a, k), 31 / k, strip)

    cut = random_cells(rng, 60, 77, p_free=0.4)

    def cut_blocks(c, xy):
        bx, by = c[:, 0] // 21, c[:, 1] // 21
        assert bx.min() == -2 and bx.max() == 1 and by.min() == -2 and by.max() == 1, "blocks cut by all four window edges"
        assert c[:, 0].min() >= -40 and c[:, 0].max() < 37 and c[:, 1].min() >= -25 and c[:, 1].max() < 35
        assert c.shape[0] == 16 and np.array_equal(np.lexsort((bx, by)), np.arange(16)), "ascending (by, bx)"
    add("negative origin, blocks cut by all four window edges", view_of(cut, a, k, -40, -25), 21 / k, cut_blocks)

    holes = random_cells(rng, 42, 63, p_free=0.4)
    holes[0:21, 21:42] = O
    holes[21:42, 0:21] = U

    def with_holes(c, xy):
        assert sorted(map(tuple, np.stack([c[:, 0] // 21, c[:, 1] // 21], axis=1).tolist())) == [(0, 0), (1, 1), (2, 0), (2, 1)]
    add("blocks with no free cell", view_of(holes, a, k), 21 / k, with_holes)

    # ties: the user's pitch of 4 cells is made 5; the block's centre cell (2, 2) is not free
    def tie_case(name, free, want):
        t = np.full((5, 5), U, dtype=np.uint8)
        for i, j in free:
            t[j, i] = F

        def tie(c, xy, want=want):
            assert rule.pitch_of(4 / k, k) == 5 and c.tolist() == [list(want)]
        add(name, view_of(t, a, k), 4 / k, tie)
    tie_case("a four-way tie at an even pitch made odd", [(1, 2), (3, 2), (2, 1), (2, 3)], (2, 1))
    tie_case("a tie decided by j", [(3, 1), (1, 3), (3, 3)], (3, 1))
    tie_case("a tie decided by i", [(3, 2), (1, 2)], (1, 2))

    pad = np.full((6, 13), U, dtype=np.uint8)
    pad[2, 12] = F

    def padded(c, xy):
        assert c.tolist() == [[12, 2]], "the padding columns are not cells"
    for fill in (F, O):
        add(f"padding columns filled with {fill}", view_of(pad, a, k, padding=fill), 31 / k, padded)
    add("all unknown", view_of(np.zeros((20, 33), dtype=np.uint8), a, k), 0.5, lambda c, xy: None if c.shape[0] == 0 else 1 / 0)

    # the region: lattice = world (anchor 0, scale 1), one free cell at the origin, the centre one double inside / outside
    lo, hi = rc.edge_of(2.0 * 2.0 + rule.KT_TOLERANCE)
    origin = np.full((3, 3), U, dtype=np.uint8)
    origin[1, 1] = F
    for axis in (0, 1):
        for d, kept in ((lo, True), (hi, False), (-lo, True), (-hi, False)):
            center = (d, 0.0) if axis == 0 else (0.0, d)

            def region(c, xy, kept=kept):
                assert c.tolist() == ([[0, 0]] if kept else [])
            add(f"region boundary {'inside' if kept else 'outside'} ({'x' if axis == 0 else 'y'} {d:+.3f})", view_of(origin, (0.0, 0.0), 1.0, -1, -1),
                1.0, region, center, 2.0)
    return out


# ---------------------------------------------------------------- fit
def circle(n, **kw):
    """a laser of n beams all around, beam 0 along -x"""
    gates = dict(min_range=0.1, max_range=7.5, range_threshold=5.0)
    gates.update(kw)
    return CaseLaser(n, -math.pi, 2.0 * math.pi / n, gates["min_range"], gates["max_range"], gates["range_threshold"])


def fit_cases():
    out = []
    rng = np.random.default_rng(23)
    a, k = (-1.0, 0.5), 4.0                                  # 0.25 m cells
    field = random_cells(rng, 50, 60, p_free=0.5, p_occ=0.2)

    def add(name, view, laser, ranges, poses, check=lambda fits: None):
        out.append(FitCase(name, view, laser, np.asarray(ranges, dtype=np.float64), np.asarray(poses, dtype=np.float64).reshape(-1, 3), check))

    def some_of_each(fits):
        assert all(f["pass_free"] > 0 for f in fits)
    inside = [(6.0, 7.0, 0.3), (2.0, 3.0, -1.0), (12.5, 11.0, 2.0), (0.5, 1.0, 0.0), (8.0, 6.5, 3.0)]
    for n in (1, 63, 64, 65, 130):
        for n_poses in (1, 2, 5):
            add(f"{n} beams, {n_poses} poses", view_of(field, a, k), circle(n), rng.uniform(0.5, 4.9, size=n), inside[:n_poses],
                some_of_each if n > 1 else (lambda fits: None))

    # a window with a negative lattice origin; sensors inside it, beside it on each side, and far off
    small = random_cells(rng, 24, 30, p_free=0.6, p_occ=0.2)
    v = view_of(small, (3.0, 2.0), k, -12, -10)              # world [0, 7.5) x [-0.5, 5.5)
    r = rng.uniform(3.0, 4.9, size=32)

    def leaves(fits):
        assert fits[0]["pass_unknown"] + fits[0]["pass_free"] + fits[0]["pass_occupied"] > 0
        assert all(sum(f[c] for c in ("pass_unknown", "pass_occupied", "pass_free")) > 0 for f in fits[1:5]), "beams from outside cross the window"
        assert sum(fits[5][c] for c in ("pass_unknown", "pass_occupied", "pass_free")) == 0, "far off: nothing lands in the window"
    add("beams leaving the window on each side, the sensor outside it, a negative lattice origin", v, circle(32), r,
        [(3.5, 2.5, 0.1), (-1.0, 2.5, 0.0), (8.5, 2.5, 0.5), (3.5, -1.5, 1.0), (3.5, 6.5, -2.0), (40.0, -30.0, 0.0)], leaves)

    # every octant and both directions of both axes: 16 beams 22.5 degrees apart, from a cell centre, on a map of free cells
    free = np.full((41, 41), F, dtype=np.uint8)

    def star(fits):
        assert fits[0]["hits_free"] == 16 and fits[0]["pass_free"] > 16 * 8
    add("all eight octants and both axis directions", view_of(free, (0.0, 0.0), k), circle(16), np.full(16, 3.1), [(5.0, 5.0, 0.0)], star)

    def on_the_spot(fits):
        assert fits[0]["pass_free"] == 2 * 4 and fits[0]["hits_free"] == 4, "the line's one cell, and the same cell as the hit"
    add("zero-length beams", view_of(free, (0.0, 0.0), k), circle(4, min_range=0.0), np.full(4, 1e-9), [(5.0, 5.0, 0.7)], on_the_spot)

    g = circle(1)
    na, inf = np.nextafter, np.inf
    edge = g.range_threshold - 1e-06
    values = [(g.min_range, False, False), (na(g.min_range, inf), True, True), (2.0, True, True), (na(edge, -inf), True, True), (edge, True, False),
              (g.range_threshold, True, False), (6.0, True, False), (na(g.max_range, -inf), True, False), (g.max_range, False, False),
              (np.nan, False, False), (inf, False, False), (-inf, False, False), (0.0, False, False), (-3.0, False, False)]
    for value, kept, hit in values:
        def gated(fits, kept=kept, hit=hit, value=value):
            f = fits[0]
            assert (f["pass_free"] > 0) == kept and f["hits_free"] == int(hit)
            if kept and value >= 5.0:
                assert f["pass_free"] == 21, "the clipped beam ends 5 m = 20 cells away and that end is not a hit"
        add(f"reading {float(value)!r}", view_of(np.full((9, 60), F, dtype=np.uint8), (0.0, 0.0), k), g, [value], [(12.0, 1.0, 0.0)], gated)

    # end cells on each of the three states: a row of free cells that ends in an unknown, an occupied and a free cell
    lanes = np.full((7, 24), F, dtype=np.uint8)
    lanes[1, 20] = U
    lanes[3, 20] = O

    def ends(fits):
        assert [(f["hits_unknown"], f["hits_occupied"], f["hits_free"]) for f in fits] == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
        assert [f["pass_free"] for f in fits] == [16, 16, 18]
    add("end cells on each of the three states", view_of(lanes, (0.0, 0.0), k), circle(1), [4.0],
        [(1.0, 0.25, math.pi), (1.0, 0.75, math.pi), (1.0, 1.25, math.pi)], ends)

    narrow = np.full((9, 13), U, dtype=np.uint8)

    def not_cells(fits):
        assert fits[0]["pass_unknown"] == 11 and fits[0]["pass_occupied"] == 0, "columns 2 .. 12 of the row, nothing of the padding"
    add("padding filled with 100", view_of(narrow, (0.0, 0.0), k, padding=O), circle(1), [4.0], [(0.5, 1.0, math.pi)], not_cells)
    return out


REFUSED_POSES = [(2.0 ** 30 / 4.0 + 1.0, 0.0, 0.0), (0.0, -1e12, 0.0), (math.nan, 0.0, 0.0), (0.0, 0.0, math.inf)]      # at scale 4, anchor near 0


# ---------------------------------------------------------------- the small map of the end-to-end tests
# The occupancy map of the eight scans of tests/relocalize_cases.py's small map at 0.05 m, from the occupancy oracle: ComputeDimensions'
# box of the sensor positions and the in-range readings, grown by a margin of 1 m on every side.
RESOLUTION, MARGIN = 0.05, 1.0
COARSE, FINE = (4.0, 0.05, 0.03), (0.5, 0.01, 0.1)          # loop / sequential preset of the localizer (dimension, resolution, smear)
PITCH, N_HEADINGS, RADIUS = 31, 8, 2.5
CENTER_OFFSET = (0.8, -0.6)
MapOf = namedtuple("MapOf", "view nav offset width height")


def occupancy_map(ranges, poses, laser, resolution=RESOLUTION, margin=MARGIN):
    from oracle import karto
    scans = [karto.Scan(r, p, laser) for r, p in zip(ranges, poses)]
    lo, hi = np.full(2, np.inf), np.full(2, -np.inf)
    for s in scans:
        ok = (s.ranges >= laser.min_range) & (s.ranges <= laser.range_threshold)
        pts = np.vstack([s.points.reshape(-1, 2)[ok], s.sensor_pose[:2]])
        lo, hi = np.minimum(lo, pts.min(axis=0)), np.maximum(hi, pts.max(axis=0))
    offset = np.floor((lo - margin) / resolution) * resolution
    width, height = (int(v) for v in np.ceil((hi + margin - offset) / resolution))
    cells, _, _ = karto.occupancy_from_scans(width, height, offset, resolution, scans, laser)
    nav = np.full((height, width), -1, dtype=np.int8)
    nav[cells[:, :width] == O] = 100
    nav[cells[:, :width] == F] = 0
    return MapOf(mr.view_dict(cells, offset, 1.0 / resolution, 0, 0, width), nav, offset, width, height)


_cache = {}


def small_map():
    """(relocalize_cases.SmallMap, MapOf)"""
    if "small" not in _cache:
        from common import LASER
        sm = rc.small_map()
        _cache["small"] = (sm, occupancy_map(sm.ranges, sm.poses, LASER))
    return _cache["small"]


def rule_on_small_map(spacing=PITCH * RESOLUTION, n_headings=N_HEADINGS, region=True, gates=rc.GATES, threads=8, **kw):
    """the rule's relocalization on the small map (computed once per distinct argument set, shared by the tests of a process)"""
    from common import LASER, OFFLINE_PARAMS
    from oracle import karto
    sm, m = small_map()
    key = (spacing, n_headings, region, gates, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))
    if key not in _cache:
        coarse = karto.Matcher(*COARSE, LASER.range_threshold, OFFLINE_PARAMS, threads=threads)
        fine = karto.Matcher(*FINE, LASER.range_threshold, OFFLINE_PARAMS, threads=threads)
        center = (sm.true_pose[0] + CENTER_OFFSET[0], sm.true_pose[1] + CENTER_OFFSET[1]) if region else None
        _cache[key] = rule.relocalize(m.view, sm.query, LASER, coarse, fine, OFFLINE_PARAMS, gates, spacing, n_headings, center,
                                      RADIUS if region else 0.0, **kw)
    return _cache[key]
