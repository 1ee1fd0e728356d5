"""Edge inputs of k_map_raycast (csrc/occupancy_map.hip) as plain numpy data.  tests/test_map_raycast_rule_oracle.py checks on the CPU that
every case sits on the edge its name says (Case.check, fed with tests/map_raycast_rule.py's answer, arrays with a leading pose axis);
tests/test_map_raycast_gpu.py asks the library for the same cases and compares exactly.  Views, lasers and the small map are
tests/map_localize_cases.py's: 0.25 m cells, sensors on cell centres where a case needs an exact cell."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_localize_cases as lc
import map_raycast_rule as rule
from map_localize_cases import F, O, U, CaseLaser, circle, view_of

RayCase = namedtuple("RayCase", "name view laser poses max_unknown no_return check")
K = 4.0                                                      # cells per metre
SMALL_MAP_COUNTS = {-1: (174, 907, 0), 20: (3, 906, 172)}   # beams by code (FREE, HIT, UNKNOWN) of the cast at the held-out pose


def counts(codes):
    return tuple(int((np.asarray(codes) == c).sum()) for c in (rule.FREE, rule.HIT, rule.UNKNOWN))


def one_beam(dx_cells, dy_cells):
    """a laser of one beam that, at heading 0 from a cell centre, ends exactly (dx, dy) cells away"""
    return CaseLaser(1, math.atan2(dy_cells, dx_cells), 0.1, 0.1, 30.0, math.hypot(dx_cells, dy_cells) / K)


def mirror_cells(c0, c1):
    """(cells of TraceLine(c0, c1), cells of the same walk started at c0: the line reflected through its midpoint), as sets"""
    x, y = rule.beam_cells(c0, c1)
    true = set(zip(x.tolist(), y.tolist()))
    return true, {(c0[0] + c1[0] - i, c0[1] + c1[1] - j) for i, j in true}


def row_case(states, width=24):
    """a strip of free cells, the sensor on cell (22, 1), one beam along -x: cell s of the beam takes states[s]"""
    cells = np.full((3, width), F, dtype=np.uint8)
    for s, state in enumerate(states):
        cells[1, 22 - s] = state
    return view_of(cells, (0.0, 0.0), K), circle(1), [(22 / K, 1 / K, 0.0)]


def ray_cases():
    out = []
    rng = np.random.default_rng(41)

    def add(name, view, laser, poses, max_unknown=-1, check=lambda c: None, no_return=None):
        out.append(RayCase(name, view, laser, np.asarray(poses, dtype=np.float64).reshape(-1, 3), max_unknown, no_return, check))

    field = lc.random_cells(rng, 50, 60, p_free=0.75, p_occ=0.05)
    inside = [(6.0, 7.0, 0.3), (2.0, 3.0, -1.0), (12.5, 11.0, 2.0), (0.5, 1.0, 0.0), (8.0, 6.5, 3.0)]
    for n in (1, 63, 64, 65, 130):
        for n_poses, budget in ((1, -1), (2, 2), (5, -1)):
            def shaped(c, n=n, n_poses=n_poses):
                assert c.codes.shape == (n_poses, n) and c.cells.shape == (n_poses, n, 2)
                if n > 1:
                    assert (c.codes == rule.HIT).any() and (c.steps > 1).any()
            add(f"{n} beams, {n_poses} poses, budget {budget}", view_of(field, (-1.0, 0.5), K), circle(n), inside[:n_poses], budget, shaped)

    # every octant and both directions of both axes: 16 beams 22.5 degrees apart from a cell centre, inside a ring of occupied cells
    ring = np.full((41, 41), F, dtype=np.uint8)
    ring[8, 8:33] = ring[32, 8:33] = ring[8:33, 8] = ring[8:33, 32] = O

    def star(c):
        assert (c.codes == rule.HIT).all()
        d = np.abs(c.cells[0].astype(np.int64) - 20)
        assert (d.max(axis=1) == 12).all() and (c.steps[0] == 12).all(), "every beam ends on the ring, 12 steps out on its long axis"
        assert len({tuple(v) for v in c.cells[0].tolist()}) == 16
    add("all eight octants and both axis directions, inside a ring", view_of(ring, (0.0, 0.0), K), circle(16), [(5.0, 5.0, 0.0)], -1, star)

    # the direction: in an octant where TraceLine swaps the end points, the outward walk is not the mirror image of the line
    c0, delta = (25, 10), (-12, 9)
    c1 = (c0[0] + delta[0], c0[1] + delta[1])
    true, mirrored = mirror_cells(c0, c1)
    only_true, only_mirrored = sorted(true - mirrored), sorted(mirrored - true)
    assert only_true and only_mirrored and delta[0] < 0 and abs(delta[1]) < abs(delta[0]) and abs(delta[0]) % abs(delta[1])
    for name, wall, code in (("a wall on a cell only TraceLine(c0, c1) visits", only_true[0], rule.HIT),
                             ("a wall on a cell only the mirrored line visits", only_mirrored[-1], rule.FREE)):
        cells = np.full((41, 41), F, dtype=np.uint8)
        cells[wall[1], wall[0]] = O

        def sided(c, wall=wall, code=code):
            assert c.codes[0, 0] == code
            assert tuple(c.cells[0, 0]) == (wall if code == rule.HIT else c1)
        add(f"swapped octant: {name}", view_of(cells, (0.0, 0.0), K), one_beam(*delta), [(c0[0] / K, c0[1] / K, 0.0)], -1, sided)

    own = np.full((9, 9), F, dtype=np.uint8)
    own[4, 4] = O

    def at_once(c):
        assert (c.codes == rule.HIT).all() and (c.steps == 0).all() and (c.cells == 4).all()
        assert (np.abs(c.ranges[0] - math.hypot(0.1, 0.05)) < 1e-12).all(), "to the cell's centre, not 0"
    add("the sensor's own cell occupied", view_of(own, (0.0, 0.0), K), circle(8), [(1.1, 1.05, 0.4)], -1, at_once)

    def last_cell(c):
        assert c.codes[0, 0] == rule.HIT and c.steps[0, 0] == 20 and tuple(c.cells[0, 0]) == (2, 1) and c.ranges[0, 0] == 5.0
    add("the hit in the line's last cell", *row_case([F] * 20 + [O]), -1, last_cell)

    def one_short(c):
        assert c.codes[0, 0] == rule.FREE and c.steps[0, 0] == 20 and tuple(c.cells[0, 0]) == (2, 1) and c.ranges[0, 0] == -1.0
    add("a wall one cell beyond the line's last cell", *row_case([F] * 21 + [O]), -1, one_short, no_return=-1.0)

    short = CaseLaser(4, -math.pi, math.pi / 2, 0.0, 7.5, 0.05)

    def on_the_spot(c):
        assert (c.steps == 0).all() and (c.cells[0] == (4, 4)).all() and (c.cells[1] == (2, 2)).all()
        assert (c.codes[0] == rule.HIT).all() and (c.codes[1] == rule.FREE).all()
    add("the far cell equal to the sensor cell", view_of(own, (0.0, 0.0), K), short, [(1.0, 1.0, 0.7), (0.5, 0.5, 0.0)], -1, on_the_spot)

    # a window with a negative lattice origin; sensors inside it, beside it on each side, and far off
    small = lc.random_cells(rng, 24, 30, p_free=0.7, p_occ=0.15)
    v = view_of(small, (3.0, 2.0), K, -12, -10)             # world [0, 7.5) x [-0.5, 5.5)
    poses = [(3.5, 2.5, 0.1), (-1.0, 2.5, 0.0), (8.5, 2.5, 0.5), (3.5, -1.5, 1.0), (3.5, 6.5, -2.0), (40.0, -30.0, 0.0)]

    def enters(c):
        assert all((c.codes[k] == rule.HIT).any() for k in range(5)), "beams from outside enter the window after unknown cells"
        assert (c.codes[5] == rule.FREE).all() and (c.steps[5] >= 14).all(), "far off: every line runs to its end"
    add("a negative lattice origin, the sensor inside, beside it on each side and far off", v, circle(32), poses, -1, enters)

    def stopped(c):
        assert (c.codes[1:] == rule.UNKNOWN).all() and (c.steps[1:] == 0).all(), "the sensor's own cell is outside the window: unknown"
    add("a negative lattice origin, budget 0", v, circle(32), poses, 0, stopped)

    def few(c):
        assert (c.codes[5] == rule.UNKNOWN).all() and (c.steps[5] == 3).all()
        assert all((c.codes[k] == rule.HIT).any() or (c.codes[k] == rule.UNKNOWN).all() for k in range(5))
    add("a negative lattice origin, budget 3", v, circle(32), poses, 3, few)

    for budget, code, steps in ((-1, rule.HIT, 5), (0, rule.UNKNOWN, 2), (1, rule.HIT, 5)):
        def budgeted(c, code=code, steps=steps):
            assert c.codes[0, 0] == code and c.steps[0, 0] == steps and tuple(c.cells[0, 0]) == (22 - steps, 1)
        add(f"one unknown cell before a wall, budget {budget}", *row_case([F, F, U, F, F, O]), budget, budgeted)
    for budget, code, steps in ((3, rule.HIT, 6), (2, rule.UNKNOWN, 4)):
        def exactly(c, code=code, steps=steps):
            assert c.codes[0, 0] == code and c.steps[0, 0] == steps
        add(f"three unknown cells before a wall, budget {budget}", *row_case([F, U, F, U, U, F, O]), budget, exactly)
    for budget, code, steps in ((0, rule.UNKNOWN, 2), (1, rule.HIT, 4)):
        def seven(c, code=code, steps=steps):
            assert c.codes[0, 0] == code and c.steps[0, 0] == steps
        add(f"a state of 7 is unknown, budget {budget}", *row_case([F, F, 7, F, O]), budget, seven)

    narrow = np.full((9, 13), F, dtype=np.uint8)

    def not_cells(c):
        assert c.codes[0, 0] == rule.FREE and c.steps[0, 0] == 20 and tuple(c.cells[0, 0]) == (22, 4), "nothing of the padding"
    add("padding filled with 100", view_of(narrow, (0.0, 0.0), K, padding=O), circle(1), [(0.5, 1.0, math.pi)], -1, not_cells)

    def not_cells_either(c):
        assert c.codes[0, 0] == rule.UNKNOWN and c.steps[0, 0] == 11 and tuple(c.cells[0, 0]) == (13, 4), "the first cell beyond the window"
    add("padding filled with 255", view_of(narrow, (0.0, 0.0), K, padding=F), circle(1), [(0.5, 1.0, math.pi)], 0, not_cells_either)
    return out
