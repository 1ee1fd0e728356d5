"""Edge inputs of the map merge's two kernels (k_map_known_box, k_map_merge in csrc/occupancy_map.hip) as plain numpy data, and the
real pair its end-to-end tests share.  tests/test_map_merge_rule_oracle.py checks on the CPU that every case sits on the edge its name
says (Case.check, fed with tests/map_merge_rule.py's answer); tests/test_map_merge_gpu.py asks the library for the same cases and
compares exactly.  The shapes are the smallest at which the kernel can still go wrong: a thread holds four cells of a row, a
workgroup a tile of 64 x 16 cells.  Scales are powers of two and anchors multiples of the cell where a case needs an exact rounding
tie."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_align_cases as ac
import map_localize_cases as lc
import map_merge_rule as rule
import merge_rule
from map_localize_cases import F, O, U

Case = namedtuple("Case", "name target moving correction footprint conflict grow check")
A, K = (0.5, -0.25), 20.0                                   # the anchor and scale of most cases: 0.05 m cells
TABLE_STATES = (U, O, F)


def table_pair():
    """the 3 x 3 pair that holds all nine (T, M) combinations on one lattice: row j has T = TABLE_STATES[j], column i has M = TABLE_STATES[i]"""
    t = np.repeat(np.array(TABLE_STATES, dtype=np.uint8)[:, None], 3, axis=1)
    m = np.repeat(np.array(TABLE_STATES, dtype=np.uint8)[None, :], 3, axis=0)
    return lc.view_of(t, A, K), lc.view_of(m, A, K)


def merge_cases():
    out = []
    rng = np.random.default_rng(47)

    def add(name, target, moving, correction, footprint=0, conflict=rule.CONFLICT_OCCUPIED, grow=1, check=lambda r: None):
        out.append(Case(name, target, moving, tuple(float(v) for v in correction), footprint, conflict, grow, check))

    def view(h, w, anchor=A, scale=K, ox=0, oy=0, padding=U):
        return lc.view_of(lc.random_cells(rng, h, w, p_free=0.45, p_occ=0.2), anchor, scale, ox, oy, padding)

    def some_of_each(r):
        assert all(r.counters[k] > 0 for k in rule.COUNTERS), r.counters

    # ---- window sizes: the output is the target's window (grow 0), the moving map covers it under a rotation
    wide = view(40, 90, ox=-10, oy=-10)

    def sized(w, h):
        def check(r):
            assert (r.window.width, r.window.height, r.window.width_step) == (w, h, lc.align8(w)) and r.overlap + r.counters["target_only"] > 0
        return check
    for w, h in ((1, 1), (3, 2), (4, 2), (5, 2), (67, 3), (65, 17)):
        add(f"a {w} x {h} output", view(h, w, padding=F), wide, (0.4, 0.3, 0.3), grow=0, check=sized(w, h))
    add("a 1 x 1 moving map into a 1 x 1 target", lc.view_of([[F]], A, K), lc.view_of([[O]], A, K), (0.0, 0.0, 0.0),
        check=lambda r: None if r.counters["conflict_moving_occupied"] == 1 and r.overlap == 1 else 1 / 0)

    # ---- padding of both inputs filled with states: never read; the output's is 0
    def padded(r):
        assert r.window.width_step > r.window.width and (r.cells[:, r.window.width:] == 0).all() and (r.codes[:, r.window.width:] == 0).all()
    add("garbage in the padding of both inputs", view(9, 13, padding=F), view(11, 10, padding=O), (0.1, 0.05, 0.2), check=padded)
    hidden = lc.view_of(np.zeros((6, 13), dtype=np.uint8), A, K, padding=O)

    def nothing_known(r):
        assert r.known_box == (0, 0, -1, -1) and r.counters["moving_only"] == 0 and r.overlap == 0
    add("a moving map known only in its padding", view(9, 13), hidden, (0.1, 0.05, 0.2), check=nothing_known)

    # ---- origins
    add("a non-zero origin on both views", view(12, 21, ox=7, oy=5), view(15, 18, ox=3, oy=9), (0.2, -0.1, 0.1), check=some_of_each)
    add("a negative origin on both views", view(12, 21, ox=-17, oy=-9), view(15, 18, ox=-12, oy=-20), (0.2, 0.3, -0.1), check=some_of_each)

    # ---- translations: whole cells, and exactly half a cell at positive and negative coordinates (scale 4, anchor 0)
    m8 = lc.random_cells(rng, 6, 8, p_free=0.5, p_occ=0.3)

    def shifted(r):
        i0, j0 = -4 + 3 - r.window.ox, -3 + 2 - r.window.oy
        assert np.array_equal(r.cells[j0:j0 + 6, i0:i0 + 8], m8), "three cells along x, two along y"
    add("a translation by whole cells", lc.view_of(np.zeros((1, 1)), (0.0, 0.0), 4.0), lc.view_of(m8, (0.0, 0.0), 4.0, -4, -3), (0.75, 0.5, 0.0), check=shifted)
    # the sample of output cell I lands on I - 1 / 2 of the moving lattice: round half away from zero reads I for I >= 1 and I - 1 for
    # I <= 0, so moving column 0 and moving row 0 are never read
    cross = np.full((9, 9), F, dtype=np.uint8)
    cross[4, :] = O
    cross[:, 4] = O

    def half_away(r):
        assert r.counters["moving_only"] > 0 and (r.cells != O).all(), "the occupied row and column 0 of the moving lattice are skipped"
    add("half a cell: ties at positive and negative coordinates", lc.view_of(np.zeros((10, 10)), (0.0, 0.0), 4.0, -5, -5),
        lc.view_of(cross, (0.0, 0.0), 4.0, -4, -4), (0.125, 0.125, 0.0), grow=0, check=half_away)

    # ---- yaws
    for yaw in (0.3, math.pi / 2, -3.0, float(np.nextafter(math.pi, 0.0))):
        add(f"yaw {yaw!r}", view(20, 70, ox=-30, oy=-8), view(33, 27, ox=-11, oy=-14), (0.15, -0.2, yaw), check=some_of_each)

    # ---- scale ratios and footprints
    fine = view(50, 60, scale=2 * K, ox=-20, oy=-15)
    coarse = view(9, 11, scale=K / 2, ox=-3, oy=-2)

    def footprint_is(n):
        def check(r):
            assert r.footprint == n and r.counters["moving_only"] + r.overlap > 0
        return check
    add("a moving map twice as fine, footprint 1", view(16, 24, ox=-6, oy=-4), fine, (0.1, 0.05, 0.3), footprint=1, check=footprint_is(1))
    add("a moving map twice as fine, footprint 2", view(16, 24, ox=-6, oy=-4), fine, (0.1, 0.05, 0.3), footprint=2, check=footprint_is(2))
    add("a moving map twice as fine, the default footprint", view(16, 24, ox=-6, oy=-4), fine, (0.1, 0.05, 0.3), check=footprint_is(2))
    add("a moving map half as fine, footprint 1", view(16, 24, ox=-6, oy=-4), coarse, (0.1, 0.05, 0.3), footprint=1, check=footprint_is(1))
    add("footprint 3", view(16, 24, ox=-6, oy=-4), fine, (0.1, 0.05, -0.4), footprint=3, check=footprint_is(3))
    add("footprint 4", view(16, 24, ox=-6, oy=-4), view(90, 99, scale=4 * K, ox=-40, oy=-30), (0.1, 0.05, 0.3), footprint=4, check=footprint_is(4))

    # ---- coverage
    def target_again(t):
        def check(r):
            w = t["width"]
            assert tuple(r.window) == (t["ox"], t["oy"], w, t["height"], lc.align8(w)) and np.array_equal(r.cells[:, :w], t["cells"][:, :w])
            assert r.counters["moving_only"] == 0 and r.overlap == 0
        return check
    t = view(7, 12, ox=2, oy=1)
    add("a moving map with no known cell", t, lc.view_of(np.zeros((20, 20)), A, K), (0.1, 0.0, 0.4), check=target_again(t))
    away = view(6, 5)

    def low_side(r):
        assert r.window.ox < t["ox"] - 50 and r.window.oy < t["oy"] - 30 and r.window.ox + r.window.width == t["ox"] + 12
        assert r.counters["moving_only"] > 0 and r.overlap == 0 and r.counters["target_only"] > 0
    add("a moving map wholly outside the target: the window grows on the low side", t, away, (-3.0, -2.0, 0.2), check=low_side)
    add("a moving map wholly outside the target, not grown", t, away, (-3.0, -2.0, 0.2), grow=0, check=target_again(t))

    # ---- the four policies on the table of all nine (T, M) combinations
    tt, tm = table_pair()
    for conflict in range(4):
        add(f"the 3 x 3 table under policy {conflict}", tt, tm, (0.0, 0.0, 0.0), footprint=1, conflict=conflict, grow=0)
    odd = lc.view_of([[7, O, F, 1]], A, K)
    add("states that are none of 0 / 100 / 255", odd, lc.view_of([[O, 9, 200, 3]], A, K), (0.0, 0.0, 0.0), grow=0,
        check=lambda r: None if r.codes[0, :4].tolist() == [rule.MOVING_ONLY, rule.TARGET_ONLY, rule.TARGET_ONLY, rule.NEITHER] else 1 / 0)
    return out


# ---------------------------------------------------------------- the real pair
TRUTH = tuple(float(v) for v in merge_rule.inverse(ac.G))
PERTURBED = {"0.05 m in x": (TRUTH[0] + 0.05, TRUTH[1], TRUTH[2]), "0.10 m in y": (TRUTH[0], TRUTH[1] + 0.10, TRUTH[2]),
             "0.02 rad": (TRUTH[0], TRUTH[1], TRUTH[2] + 0.02)}
_cache = {}


def real_pair():
    """(target MapOf, moving MapOf, the rule's merge under the true correction): computed once per process and left unchanged"""
    if "pair" not in _cache:
        target, moving = ac.maps()
        _cache["pair"] = (target, moving, rule.merge(target.view, moving.view, TRUTH, footprint=1, conflict=rule.CONFLICT_OCCUPIED, grow=1))
    return _cache["pair"]
