"""Edge inputs of the visibility kernels (csrc/occupancy_visibility.hip) as plain numpy data.  tests/test_map_visibility_rule_oracle.py
checks the rule on them against an independent restatement on the CPU; tests/test_map_visibility_gpu.py asks the library for the same
cases and compares exactly.  Views, lasers and the small map are tests/map_localize_cases.py's, the rows and the direction cases
tests/map_raycast_cases.py's: 0.25 m cells, sensors on cell centres where a case needs an exact cell."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_localize_cases as lc
import map_raycast_cases as rc
from map_localize_cases import F, O, U, CaseLaser, circle, random_cells, view_of
from map_raycast_cases import K, row_case

VisCase = namedtuple("VisCase", "name view laser poses params")
SelectCase = namedtuple("SelectCase", "name view laser poses k min_gain params committed")
BEAMS = (1, 63, 64, 65, 255, 256, 257, 513)
BUDGETS = (-1, 0, 2, 20)
INSIDE = [(6.0, 7.0, 0.3), (2.0, 3.0, -1.0), (12.5, 11.0, 2.0), (0.5, 1.0, 0.0), (8.0, 6.5, 3.0)]
_cache = {}


def reach_laser(reach, n=16):
    """a laser of n beams all around whose reach at K cells per metre is exactly `reach`: floor(range_threshold * K) = reach - 2"""
    return circle(n, range_threshold=(reach - 2) / K, max_range=(reach - 2) / K + 10.0)


def field():
    if "field" not in _cache:
        _cache["field"] = random_cells(np.random.default_rng(41), 50, 60, p_free=0.75, p_occ=0.05)
    return _cache["field"]


def door_views():
    """two rooms and a wall between them, closed and with a door of 3 cells opened: the same window and lattice"""
    closed = np.full((30, 40), F, dtype=np.uint8)
    closed[0, :] = closed[-1, :] = closed[:, 0] = closed[:, -1] = O
    closed[:, 20] = O
    closed[3:8, 25:38] = U
    opened = closed.copy()
    opened[14:17, 20] = F
    return view_of(closed, (0.5, -0.25), K, -3, 4), view_of(opened, (0.5, -0.25), K, -3, 4)


def vis_cases():
    if "vis" in _cache:
        return _cache["vis"]
    out = []
    rng = np.random.default_rng(43)

    def add(name, view, laser, poses, **params):
        out.append(VisCase(name, view, laser, np.asarray(poses, dtype=np.float64).reshape(-1, 3), params))

    # wave and run-of-256 edges: every beam count with 1, 2 and 5 poses, the four budgets in turn
    v = view_of(field(), (-1.0, 0.5), K)
    turn = 0
    for n in BEAMS:
        for n_poses in (1, 2, 5):
            budget = BUDGETS[turn % 4]
            turn += 1
            add(f"{n} beams, {n_poses} poses, budget {budget}", v, circle(n), INSIDE[:n_poses], max_unknown=budget)

    for state, word in ((F, "free"), (O, "occupied"), (U, "unknown")):
        add(f"a window of one {word} cell", view_of(np.full((1, 1), state, dtype=np.uint8), (0.0, 0.0), K, 3, -2), circle(16),
            [(0.75, -0.5, 0.0), (1.25, -0.5, 0.0), (0.75, 1.0, 0.5)], max_unknown=-1)
    add("a window of 1 x 7", view_of(random_cells(rng, 1, 7, p_free=0.6, p_occ=0.1), (0.0, 0.0), K), circle(32), [(0.75, 0.0, 0.1), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0)], max_unknown=4)
    add("a window of 7 x 1", view_of(random_cells(rng, 7, 1, p_free=0.6, p_occ=0.1), (0.0, 0.0), K), circle(32), [(0.0, 0.75, 0.1), (1.0, 0.5, 0.0), (0.0, -1.0, 0.0)], max_unknown=4)
    narrow = np.full((9, 13), F, dtype=np.uint8)
    for fill in (O, F):
        add(f"a width of 13, padding filled with {fill}", view_of(narrow, (0.0, 0.0), K, padding=fill), circle(64), [(0.5, 1.0, math.pi), (3.0, 1.0, 0.0)],
            max_unknown=0 if fill == F else -1)

    small = random_cells(rng, 24, 30, p_free=0.7, p_occ=0.15)
    negative = view_of(small, (3.0, 2.0), K, -12, -10)        # world [0, 7.5) x [-0.5, 5.5)
    around = [(3.5, 2.5, 0.1), (-1.0, 2.5, 0.0), (8.5, 2.5, 0.5), (3.5, -1.5, 1.0), (3.5, 6.5, -2.0), (40.0, -30.0, 0.0)]
    for budget in (-1, 0, 3):
        add(f"a negative lattice origin, the sensor inside, beside each side and far off, budget {budget}", negative, circle(32), around, max_unknown=budget)

    by_name = {c.name: c for c in rc.ray_cases()}
    for name in ("all eight octants and both axis directions, inside a ring", "swapped octant: a wall on a cell only TraceLine(c0, c1) visits",
                 "swapped octant: a wall on a cell only the mirrored line visits", "the sensor's own cell occupied", "the far cell equal to the sensor cell"):
        c = by_name[name]
        add(name, c.view, c.laser, c.poses, max_unknown=c.max_unknown)
    for budget in (-1, 0, 1):
        add(f"one unknown cell before a wall, budget {budget}", *row_case([F, F, U, F, F, O]), max_unknown=budget)

    # the reach: the smallest there is (a range_threshold below one cell: 2, a bitmap of 5 x 5) with the sensor's own cell occupied;
    # the first bitmaps above 64 KB; the largest accepted.  The window stays small, so the walks stay short.
    own = np.full((9, 9), F, dtype=np.uint8)
    own[4, 4] = O
    add("reach 2 with the sensor's own cell occupied", view_of(own, (0.0, 0.0), K), circle(8, range_threshold=0.2, max_range=7.5), [(1.1, 1.05, 0.4), (0.5, 0.5, 0.0)], max_unknown=-1)
    for reach in (361, 362, 363, 511):
        add(f"reach {reach}", v, reach_laser(reach), INSIDE[:2] + [(-20.0, 3.0, 0.2)], max_unknown=20 if reach != 363 else -1)
    _cache["vis"] = out
    return out


def select_cases():
    if "select" in _cache:
        return _cache["select"]
    out = []
    rng = np.random.default_rng(47)
    v = view_of(field(), (-1.0, 0.5), K)

    def scattered(n):
        return np.stack([rng.uniform(-1.5, 14.5, n), rng.uniform(0.0, 13.5, n), rng.uniform(-3.0, 3.0, n)], axis=1)

    def add(name, view, laser, poses, k, min_gain=1, committed=(), **params):
        out.append(SelectCase(name, view, laser, np.asarray(poses, dtype=np.float64).reshape(-1, 3), k, min_gain, params,
                              np.asarray(committed, dtype=np.float64).reshape(-1, 3)))

    add("1 candidate, k 1", v, circle(16), INSIDE[:1], 1, max_unknown=-1)
    add("65 candidates, k 2", v, circle(16), scattered(65), 2)
    add("65 candidates, k 8, weights (0, 1, 0)", v, circle(16), scattered(65), 8, w_unknown=0, w_free=1, w_occupied=0)
    add("300 candidates, k 8, weights (3, 1, 2)", v, circle(16), scattered(300), 8, w_unknown=3, w_free=1, w_occupied=2)
    add("300 candidates, k 1", v, circle(16), scattered(300), 1)
    # two distinct poses among five candidates: once both are picked no candidate adds a cell, and the selection ends
    add("an early stop: 5 candidates of 2 distinct poses, k 5", v, circle(16), [INSIDE[0], INSIDE[0], INSIDE[1], INSIDE[1], INSIDE[0]], 5)
    add("a tie between two identical candidates", v, circle(16), [INSIDE[2], INSIDE[3], INSIDE[2], INSIDE[3]], 3, w_unknown=1, w_free=1, w_occupied=1)
    add("a pre-committed mask", v, circle(16), scattered(20), 4, committed=scattered(6), w_unknown=1, w_free=1, w_occupied=0)
    _cache["select"] = out
    return out
