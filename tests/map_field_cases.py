"""Edge inputs of the distance field's kernels (csrc/occupancy_field.hip) as plain numpy data: the smallest windows at which each
kernel can still go wrong.  tests/test_map_field_rule_oracle.py checks on the CPU that every case sits on the edge its name says
(Case.check, fed with tests/map_field_rule.py's answer); tests/test_map_field_gpu.py asks the library for the same cases and compares
exactly.  The scale is a power of two, so max_distance = R / scale gives exactly R cells."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import map_field_rule as rule
import map_localize_cases as lc

U, O, F = lc.U, lc.O, lc.F
A, K = (-1.0, 0.5), 4.0                                     # anchor, scale: 0.25 m cells
FieldCase = namedtuple("FieldCase", "name view radius obstacles check")
INFLATIONS = [dict(), dict(inscribed_radius=0.5, inflation_radius=0.5, cost_scaling_factor=0.0),
              dict(inscribed_radius=0.0, inflation_radius=2.5, cost_scaling_factor=1.3)]       # Rt = 3, 2, 10 at scale 4
UNKNOWN_POLICIES = [(0, 0), (0, 1), (1, 0), (1, 1)]         # track_unknown, inflate_unknown


def mixed(rng, h, w, p_occ=0.15):
    return rng.choice(np.array([U, O, F], dtype=np.uint8), size=(h, w), p=[0.25, p_occ, 0.75 - p_occ])


def field_cases():
    out = []
    rng = np.random.default_rng(41)

    def add(name, cells, radius, obstacles=rule.OCCUPIED, check=lambda d2: None, ox=0, oy=0, padding=U):
        out.append(FieldCase(name, lc.view_of(cells, A, K, ox, oy, padding), radius, obstacles, check))

    # ---- sizes
    shapes = [(1, 1), (1, 7), (7, 1), (13, 7), (65, 3), (129, 2), (3, 65)]       # width x height
    grids = {s: mixed(rng, s[1], s[0]) for s in shapes}
    grids[(1, 7)][3, 0] = O
    grids[(7, 1)][0, 2] = O
    for r in (0, 1, 3):
        add(f"1 x 1 with an obstacle, R {r}", np.array([[O]], dtype=np.uint8), r, check=lambda d2: None if d2.tolist() == [[0]] else 1 / 0)
        add(f"1 x 1 without an obstacle, R {r}", np.array([[F]], dtype=np.uint8), r, check=lambda d2: None if d2.tolist() == [[rule.FAR]] else 1 / 0)
        for w, h in shapes[1:]:
            add(f"{w} x {h}, R {r}", grids[(w, h)], r)

    # ---- padding
    pad = np.full((5, 13), F, dtype=np.uint8)
    pad[2, 3] = O

    def padded(d2):
        assert d2[2, 12] == 81 and d2[0, 12] == 85, "the padding columns hold no obstacle"
    add("padding columns filled with 100", pad, 0, check=padded, padding=O)
    add("padding columns filled with 100, not-free obstacles", pad, 0, rule.NOT_FREE, check=padded, padding=O)

    # ---- content
    def all_far(d2):
        assert (d2 == rule.FAR).all()
    add("no obstacle", np.full((6, 70), F, dtype=np.uint8), 0, check=all_far)
    add("no obstacle, capped", np.full((6, 70), F, dtype=np.uint8), 3, check=all_far)
    add("unknown cells are no obstacle under OCCUPIED", np.full((4, 9), U, dtype=np.uint8), 3, check=all_far)

    def all_zero(d2):
        assert (d2 == 0).all()
    add("every cell an obstacle", np.full((7, 66), O, dtype=np.uint8), 0, check=all_zero)
    add("unknown cells are obstacles under NOT_FREE", np.full((4, 9), U, dtype=np.uint8), 3, rule.NOT_FREE, check=all_zero)
    corners = np.full((9, 70), F, dtype=np.uint8)
    for j, i in ((0, 0), (0, 69), (8, 0), (8, 69)):
        corners[j, i] = O

    def cornered(d2):
        assert d2[4, 34] == 16 + 34 * 34 and d2[4, 35] == 16 + 34 * 34 and d2[0, 1] == 1 and d2[8, 68] == 1
    add("one obstacle in each corner", corners, 0, check=cornered)
    seven = np.full((5, 9), F, dtype=np.uint8)
    seven[2, 4] = 7
    add("a cell of state 7 is no obstacle under OCCUPIED", seven, 0, check=all_far)
    add("a cell of state 7 is an obstacle under NOT_FREE", seven, 0, rule.NOT_FREE, check=lambda d2: None if d2[2, 4] == 0 and d2[0, 0] == 20 else 1 / 0)
    both = mixed(rng, 11, 21)
    add("unknown, occupied and free cells under OCCUPIED", both, 3)
    add("unknown, occupied and free cells under NOT_FREE", both, 3, rule.NOT_FREE)

    # ---- reach
    wide = np.full((2, 300), F, dtype=np.uint8)
    wide[0, 0] = O
    add("300 x 2, the only obstacle at column 0, uncapped", wide, 0, check=lambda d2: None if d2[0, 299] == 299 ** 2 and d2[1, 299] == 299 ** 2 + 1 else 1 / 0)
    tall = np.full((300, 2), F, dtype=np.uint8)
    tall[0, 0] = O
    add("2 x 300, the only obstacle at row 0, uncapped", tall, 0, check=lambda d2: None if d2[299, 0] == 299 ** 2 and d2[299, 1] == 299 ** 2 + 1 else 1 / 0)
    add("2 x 300, the obstacle beyond the cap", tall, 3, check=lambda d2: None if d2[3, 0] == 9 and d2[3, 1] == rule.FAR and d2[4, 0] == rule.FAR else 1 / 0)
    near = np.full((40, 40), F, dtype=np.uint8)
    near[20, 26] = O                                           # 6 cells along the row from (20, 20): beyond R = 5
    near[17, 16] = O                                           # 3 up and 4 to the left: d2 = 25, within it

    def diagonal(d2):
        assert d2[20, 20] == 25 and d2[20, 21] == 25 and d2[21, 20] == rule.FAR, "the 3-4-5 neighbour is kept, d2 = 32 and 37 are not"
    add("40 x 40, the row neighbour beyond R, a diagonal one within it", near, 5, check=diagonal)

    # ---- random
    for p_occ in (0.02, 0.3):
        for seed in (1, 2, 3):
            cells = mixed(np.random.default_rng(100 + seed), 50, 40, p_occ)
            for r in (0, 4, 11):
                add(f"40 x 50 random, p_occ {p_occ}, seed {seed}, R {r}", cells, r, ox=-17, oy=-33)
    return out


def cost_fields():
    """the cases the costs are checked on: windows that hold all three states, fields that reach Rt = 10 cells"""
    return [c for c in field_cases() if c.name.startswith("40 x 50 random") and c.name.endswith(("R 0", "R 11")) and "seed 1" in c.name]


def clearance_points(view, d2):
    """world points of the window `view` on cell centres (the first FAR cell and the first obstacle of the field `d2` among them), on
    the rounding edges, one cell outside each side, and beyond 2^30 cells (the last nine are OUTSIDE)"""
    ax, ay, k = view["anchor"][0], view["anchor"][1], view["scale"]
    ox, oy, w, h = view["ox"], view["oy"], view["width"], view["height"]
    (fj, fi), (zj, zi) = (np.argwhere(d2 == v)[0] if (d2 == v).any() else (0, 0) for v in (rule.FAR, 0))
    pts = [(ax + (ox + i) / k, ay + (oy + j) / k) for i, j in ((0, 0), (w - 1, h - 1), (w // 2, h // 3), (1, h - 1), (int(fi), int(fj)), (int(zi), int(zj)))]
    for i in (ox, ox + w - 1, -1, 0, 1):                       # half-way between two cells: rounds away from zero, both signs
        pts += [(ax + (i + 0.5) / k, ay + (oy + 2) / k), (ax - (i + 0.5) / k, ay + (oy + 2) / k), (ax + (ox + 2) / k, ay + (i + 0.5) / k)]
    pts += [(ax + (ox - 1) / k, ay + oy / k), (ax + (ox + w) / k, ay + oy / k), (ax + ox / k, ay + (oy - 1) / k), (ax + ox / k, ay + (oy + h) / k)]
    pts += [(ax + (2.0 ** 30 + 1) / k, ay), (ax, ay - (2.0 ** 30 + 1) / k), (ax + 2.0 ** 30 / k, ay), (1e300, -1e300), (ax + 3.0e9 / k, ay)]
    return np.array(pts, dtype=np.float64)
