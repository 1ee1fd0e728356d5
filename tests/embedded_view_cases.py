"""Which rows of the existing case tables run through tests/embedded_view.py's layouts, consumer by consumer -- every entry point of
include/karto_hip.h that reads the cells of a kh_map_view -- and the few cases made here: maps for the matcher's AddMap and
rectangles of a field update whose first and last columns take every residue modulo 4.  Plain numpy data;
tests/test_embedded_view_rule_oracle.py checks on the CPU that the rows exist and sit where this file says,
tests/test_embedded_view_gpu.py asks the library."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import map_changes_cases as cc
import map_field_cases as fc
import map_field_rule as field_rule
import map_field_update_cases as uc
import map_localize_cases as lc
import map_match_cases as mc
import map_merge_cases as gc
import map_raycast_cases as rc

WIDTHS = {1, 3, 5, 13, 37, 67}                              # every one of them is some case's window width

SEED_ROWS = ["negative origin, blocks cut by all four window edges", "padding columns filled with 255", "a four-way tie at an even pitch made odd",
             "pitch larger than the map"]
FIT_ROWS = ["beams leaving the window on each side, the sensor outside it, a negative lattice origin", "padding filled with 100",
            "end cells on each of the three states"]
RAY_ROWS = ["a negative lattice origin, the sensor inside, beside it on each side and far off", "a negative lattice origin, budget 3",
            "padding filled with 100", "padding filled with 255"]
MERGE_ROWS = ["a 1 x 1 output", "a 3 x 2 output", "a 5 x 2 output", "a 67 x 3 output", "a negative origin on both views", "yaw 0.3",
              "a moving map wholly outside the target: the window grows on the low side", "a moving map wholly outside the target, not grown"]
OBSERVE_ROWS = FIT_ROWS
FIELD_ROWS = ["1 x 7, R 3", "13 x 7, R 3", "65 x 3, R 0", "3 x 65, R 3", "padding columns filled with 100",
              "padding columns filled with 100, not-free obstacles", "40 x 50 random, p_occ 0.3, seed 1, R 11"]
SHAPE_EDIT_ROWS = ["1 x 7, R 3", "13 x 7, R 3", "65 x 3, R 3", "3 x 65, R 11"]
MERGE_LAYOUTS = [("L1", "L3"), ("L3", "L2"), ("L2", "L1"), ("L4", "L3"), ("L3", "L4")]     # target, moving: never the same; L4 where the width is odd


def rows(table, names):
    by_name = {c.name: c for c in table}
    return [by_name[n] for n in names]


def seed_rows():
    return rows(lc.seed_cases(), SEED_ROWS)


def fit_rows():
    return rows(lc.fit_cases(), FIT_ROWS)


def ray_rows():
    return rows(rc.ray_cases(), RAY_ROWS)


def merge_rows():
    return rows(gc.merge_cases(), MERGE_ROWS)


def observe_rows():
    return rows(cc.observe_cases(), OBSERVE_ROWS)


def field_rows():
    return rows(fc.field_cases(), FIELD_ROWS)


def shape_edit_rows():
    return rows(uc.shape_edits(), SHAPE_EDIT_ROWS)


def inflation_for(radius):
    """the widest of fc.INFLATIONS (Rt = 10, 3, 2 cells) a field of this radius reaches, or None"""
    for k, rt in ((2, 10), (0, 3), (1, 2)):
        if radius == 0 or radius >= rt:
            return fc.INFLATIONS[k]
    return None


# ---------------------------------------------------------------- the matcher's AddMap: maps of 0.01 m cells around the query's pose
MapCase = namedtuple("MapCase", "name view pose ranges")
QUERY_BEAMS = 8                                             # the first beams of the synthetic laser, 0.25 degrees apart


def map_cases():
    """the query looks along 0.2 rad from a cell near the window's low corner: its eight points lie 0.12 .. 0.28 m out, among the
    window's cells, so the match on the map has a response above 0"""
    import math
    rng = np.random.default_rng(53)
    out = []
    heading = 0.2 + math.radians(135.0)
    for name, (w, h), (ox, oy), (px, py) in (("37 x 20", (37, 20), (0, 0), (0.5, 0.25)), ("67 x 5", (67, 5), (3, 40), (0.5, 0.56)),
                                            ("13 x 30 at a negative origin", (13, 30), (-25, -12), (0.05, 0.15))):
        cells = lc.random_cells(rng, h, w, p_free=0.3, p_occ=0.4)
        cells[0, 0] = cells[h - 1, w - 1] = cells[0, w - 1] = cells[h - 1, 0] = lc.O
        out.append(MapCase(name, lc.view_of(cells, (0.43, 0.17), 100.0, ox, oy), np.array([px, py, heading]), np.linspace(0.12, 0.28, QUERY_BEAMS)))
    return out


MATCHER = mc.FOOT                                           # the smear kernel holds 100 beside its centre: the order of the cells shows in the bytes


# ---------------------------------------------------------------- MapField.update: rectangles at every residue modulo 4
def rect_forms_mod4():
    """uc.state_only_edit(NOT_FREE) -- 37 x 30 at (-8, 3), the edit inside columns 20 .. 25, rows 10 .. 13 -- named by rectangles whose
    first column is 17, 18, 19, 20 and whose last column is 25, 26, 27, 28: every residue modulo 4 on either side, where
    k_field_changed chooses between the dword and the bytes"""
    e = uc.state_only_edit(field_rule.NOT_FREE)
    ox, oy = e.before["ox"], e.before["oy"]
    out = []
    for first in (17, 18, 19, 20):
        for last in (25, 26, 27, 28):
            out.append(uc.Edit(f"columns {first} .. {last}", e.before, e.after, e.radius, e.obstacles, (ox + first, oy + 9, last - first + 1, 6)))
    return out


RANDOM_ROUNDS = dict(density=0.1, obstacles=field_rule.OCCUPIED, rounds=10, seed=5)
RANDOM_RADIUS = 4
