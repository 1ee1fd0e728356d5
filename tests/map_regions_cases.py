"""Edge inputs of the region analysis' kernels (csrc/occupancy_regions.hip) as plain numpy data: the smallest windows at which each
kernel can still go wrong -- window sizes around the 64 x 16 tile, fills, long union chains across tile seams, tile corners, the
clearance threshold, the frontier's definition, the limits.  tests/test_map_regions_rule_oracle.py checks the rule on them against a
brute-force search and pins hand values; tests/test_map_regions_gpu.py asks the library for the same cases and compares exactly.
The scale is a power of two, so min_clearance = Rc / scale gives exactly Rc cells.  A case's `radius` is the field's R."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import map_field_rule as fr
import map_localize_cases as lc

U, O, F = lc.U, lc.O, lc.F
A, K = (-1.0, 0.5), 4.0                                     # anchor, scale: 0.25 m cells
RegionCase = namedtuple("RegionCase", "name view radius params")
_d2 = {}


def clearance_of(rc, scale):
    """a min_clearance whose ceiling at `scale` is rc cells whatever the scale's rounding"""
    return max(0.0, rc - 0.5) / scale


def field_values(case):
    """the field's values of a case (computed once per view and radius, shared by the tests of a process)"""
    key = (id(case.view), case.radius)
    if key not in _d2:
        _d2[key] = fr.d2_brute(case.view, case.radius)
    return _d2[key]


def mixed(rng, h, w, p_occ=0.15, p_unknown=0.25):
    return rng.choice(np.array([U, O, F], dtype=np.uint8), size=(h, w), p=[p_unknown, p_occ, 1.0 - p_occ - p_unknown])


def full(h, w, state=F):
    return np.full((h, w), state, dtype=np.uint8)


def serpentine(h=50, w=130):
    """a one-cell-wide corridor: the even rows are free, the odd rows walls with one gap at alternating ends"""
    c = full(h, w, O)
    c[0::2, :] = F
    for k, row in enumerate(range(1, h, 2)):
        c[row, w - 1 if k % 2 == 0 else 0] = F
    return c


def comb(h=33, w=129):
    """teeth on the even columns that join only in the last row"""
    c = full(h, w, O)
    c[:, 0::2] = F
    c[h - 1, :] = F
    return c


def two_rooms(door=2):
    """two 30 x 20 rooms in a 65 x 22 window, a wall between them with a door of `door` cells"""
    c = full(22, 65, O)
    c[1:21, 1:31] = F
    c[1:21, 32:64] = F
    c[10:10 + door, 31] = F
    return c


def necked():
    """40 x 12: free above unknown rows; a wall from the top leaves a one-cell passage along the frontier row"""
    c = full(12, 40, F)
    c[8:, :] = U
    c[0:7, 20] = O
    return c


def sparse_walls(length, across):
    """a 2-cell-wide strip `length` long with full walls at irregular places and a few unknown cells"""
    rng = np.random.default_rng(77)
    c = full(2, length, F)
    c[:, np.sort(rng.choice(np.arange(5, length - 5), size=40, replace=False))] = O
    c[1, rng.choice(np.arange(length), size=25, replace=False)] = U
    c[0, 63:66] = O; c[1, 63] = O                            # the top row is cut at a tile border, the bottom row passes by
    return c if across else np.ascontiguousarray(c.T)


def region_cases():
    out = []

    def add(name, cells, radius=0, ox=0, oy=0, padding=U, **params):
        view = lc.view_of(cells, A, K, ox, oy, padding)
        for conn in params.pop("connectivities", (4, 8)):
            out.append(RegionCase(f"{name}, N{conn}", view, radius, dict(params, connectivity=conn)))

    rng = np.random.default_rng(43)
    # ---- window sizes
    add("1 x 1 free", full(1, 1))
    add("1 x 1 occupied", full(1, 1, O))
    add("1 x 1 unknown", full(1, 1, U))
    for w, h in ((1, 7), (7, 1), (64, 16), (65, 17), (129, 33)):
        add(f"{w} x {h} mixed", mixed(rng, h, w))
    rows = full(5, 13)
    rows[1::2, :] = O
    add("13 x 5, free rows between walls, the padding filled with 255", rows, padding=F)
    add("13 x 5 all free, the padding filled with 0", full(5, 13), padding=U)
    # ---- fills
    add("70 x 20 all free", full(20, 70))
    add("70 x 20 all occupied", full(20, 70, O))
    board = full(18, 66, O)
    board[(np.add.outer(np.arange(18), np.arange(66)) % 2) == 0] = F
    add("66 x 18 checkerboard, capped at 100", board, max_regions=100)
    # ---- long chains across seams
    add("130 x 50 serpentine", serpentine())
    add("129 x 33 comb", comb())
    # ---- tile corners
    for name, pair in (("down-right", ((63, 15), (64, 16))), ("down-left", ((64, 15), (63, 16)))):
        c = full(34, 130, O)
        for i, j in pair:
            c[j, i] = F
        add(f"130 x 34, a diagonal pair {name} across a tile corner", c)
    ring = full(34, 130, O)
    ring[14:18, 62:66] = F
    ring[15:17, 63:65] = O
    add("130 x 34, a ring around a tile corner", ring)
    circle = full(20, 30, F)
    circle[4:15, 6:20] = O
    circle[5:14, 7:19] = F
    add("30 x 20, a ring of wall: inside and outside", circle)
    # ---- randoms
    for p_occ in (0.1, 0.4):
        for seed in (1, 2, 3):
            add(f"40 x 50 random, p_occ {p_occ}, seed {seed}", mixed(np.random.default_rng(200 + seed), 50, 40, p_occ), ox=-17, oy=-33)
    add("40 x 50 random, p_occ 0.4, seed 1, minimum 3", mixed(np.random.default_rng(201), 50, 40, 0.4), ox=-17, oy=-33, min_region_cells=3, min_frontier_cells=3)
    # ---- the clearance threshold
    for rc in (0, 2, 5):
        add(f"two rooms and a door of 2 cells, Rc {rc}", two_rooms(), radius=8, min_clearance=rc / K)
    add("two rooms, a field of R 3: FAR members", two_rooms(), radius=3, min_clearance=2 / K)
    # ---- frontiers
    edge = full(9, 20, O)
    edge[:, 0] = F; edge[0, :] = F
    add("free cells at the window's edge, nothing unknown", edge)
    seven = full(9, 20)
    seven[4, 10] = 7
    add("a cell of state 7 is unknown", seven)
    across = full(40, 100)
    across[30:, :] = U
    across[:, 90:] = U
    add("100 x 40, the frontier crosses tile seams both ways", across)
    add("a cluster whose traversable cells lie in two regions, Rc 2", necked(), radius=8, min_clearance=2 / K)
    room = full(12, 30, U)
    room[2:9, 3:14] = O
    room[3:8, 4:13] = F
    room[3:8, 20:26] = F
    add("a closed room beside an open one", room)
    # ---- limits
    add("32768 x 2, sparse walls", sparse_walls(32768, True), radius=4, min_clearance=1 / K)
    add("2 x 32768, sparse walls", sparse_walls(32768, False), radius=4, min_clearance=1 / K)
    return out


def lookup_points(view):
    """world points of the window `view`: cell centres, half-away ties of both signs, one cell outside each side, beyond 2^30 cells"""
    ax, ay, k = view["anchor"][0], view["anchor"][1], view["scale"]
    x0, y0, w, h = view["ox"], view["oy"], view["width"], view["height"]
    cell = lambda i, j: (ax + (x0 + i) / k, ay + (y0 + j) / k)  # noqa: E731
    pts = [cell(i, j) for j in range(0, h, max(1, h // 7)) for i in range(0, w, max(1, w // 7))]
    pts += [(ax + (x0 + 2 + 0.5) / k, ay + (y0 + 3 - 0.5) / k), (ax + (x0 - 0.5) / k, ay + (y0 + 0.5) / k), (ax + (x0 + w - 0.5) / k, ay + (y0 + h - 0.5) / k)]
    pts += [cell(-1, 2), cell(w, 2), cell(2, -1), cell(2, h), (ax + (2.0 ** 30 + 1.0) / k, ay), (ax, ay - (2.0 ** 30 + 1.0) / k), (ax + 2.0 ** 30 / k, ay)]
    return np.array(pts, dtype=np.float64)
