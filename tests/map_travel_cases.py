"""Edge inputs of the travel-cost kernels (csrc/occupancy_travel.hip) as plain numpy data, on the lattice of the region cases
(tests/map_regions_cases.py: anchor A, scale K) and with their builders where they fit: window sizes around the 64 x 16 tile, fills,
the longest chains of tile hand-offs, tile corners, goals of every status, the clearance threshold, the weights' limits, the window
limits.  tests/test_map_travel_rule_oracle.py checks the rule on them against an independent relaxation; tests/test_map_travel_gpu.py
asks the library for the same cases and compares exactly.  A case's `radius` is the field's R; its goals and starts are world points."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import map_field_rule as fr
import map_localize_cases as lc
import map_regions_cases as rcases

U, O, F = lc.U, lc.O, lc.F
A, K = rcases.A, rcases.K
TravelCase = namedtuple("TravelCase", "name view radius params goals starts")
full, mixed, serpentine, comb, two_rooms, sparse_walls, lookup_points = (rcases.full, rcases.mixed, rcases.serpentine, rcases.comb, rcases.two_rooms,
                                                                        rcases.sparse_walls, rcases.lookup_points)
_d2 = {}


def field_values(case):
    """the field's values of a case (computed once per view and radius, shared by the tests of a process)"""
    key = (id(case.view), case.radius)
    if key not in _d2:
        _d2[key] = fr.d2_brute(case.view, case.radius)
    return _d2[key]


def world(view, i, j):
    """the world point of window cell (i, j)"""
    return (view["anchor"][0] + (view["ox"] + i) / view["scale"], view["anchor"][1] + (view["oy"] + j) / view["scale"])


def free_cells(view, every, limit=8):
    """window cells (i, j) of state 255, every `every`-th in row-major order, at most `limit`"""
    jj, ii = np.nonzero(view["cells"][:view["height"], :view["width"]] == F)
    return [(int(i), int(j)) for i, j in zip(ii[::every][:limit], jj[::every][:limit])]


def pose_like(view, cells):
    """starts of a case: the given cells, then a cell that is not free (if any), then a point outside the window"""
    pts = [world(view, i, j) for i, j in cells]
    jj, ii = np.nonzero(view["cells"][:view["height"], :view["width"]] != F)
    if jj.size:
        pts.append(world(view, int(ii[0]), int(jj[0])))
    pts.append(world(view, -3, 1))
    return np.array(pts, dtype=np.float64)


def travel_cases():
    out = []

    def add(name, cells, goals, radius=0, ox=0, oy=0, padding=U, starts=None, connectivities=(4, 8), cuts=(0,), **params):
        view = lc.view_of(cells, A, K, ox, oy, padding)
        goal_xy = np.array([world(view, i, j) for i, j in goals], dtype=np.float64).reshape(-1, 2)
        start_xy = pose_like(view, free_cells(view, max(1, int((view["cells"][:view["height"], :view["width"]] == F).sum()) // 7)) if starts is None else starts)
        for conn in connectivities:
            for cut in cuts:
                tag = f"{name}, N{conn}" + (f", cut {cut}" if len(cuts) > 1 else "")
                out.append(TravelCase(tag, view, radius, dict(params, connectivity=conn, cut_corners=cut), goal_xy, start_xy))

    rng = np.random.default_rng(47)
    # ---- window sizes
    add("1 x 1 free", full(1, 1), [(0, 0)])
    add("1 x 1 occupied", full(1, 1, O), [(0, 0)])
    add("1 x 1 unknown", full(1, 1, U), [(0, 0)])
    for w, h in ((1, 7), (7, 1), (64, 16), (65, 17), (129, 33)):
        cells = mixed(rng, h, w, 0.15, 0.1)
        cells[h - 1, w - 1] = F
        add(f"{w} x {h} mixed", cells, [(w - 1, h - 1), (0, 0)], cuts=(0, 1) if (w, h) == (65, 17) else (0,), goal_snap_cells=1)
    add("13 x 5 all free, the padding filled with 255", full(5, 13), [(12, 4)], padding=F)
    add("13 x 5 all free, the padding filled with 0", full(5, 13), [(12, 0)], padding=U)
    # ---- fills
    add("70 x 20 all free", full(20, 70), [(3, 2)])
    add("70 x 20 all occupied", full(20, 70, O), [(3, 2), (69, 19), (0, 0)], goal_snap_cells=16)
    # ---- the longest chains of tile hand-offs
    add("130 x 50 serpentine, the goal at one end", serpentine(), [(0, 0)])
    add("129 x 33 comb, the teeth join in the last row of the last tile", comb(), [(0, 0)])
    # ---- tile corners
    for name, pair in (("down-right", ((63, 15), (64, 16))), ("down-left", ((64, 15), (63, 16)))):
        c = full(34, 130, O)
        for i, j in pair:
            c[j, i] = F
        add(f"130 x 34, a diagonal pair {name} across a tile corner", c, [pair[0]], cuts=(0, 1), starts=pose_like(lc.view_of(c, A, K), pair))
        add(f"130 x 34, a diagonal pair {name} across a tile corner, from the other end", c, [pair[1]], cuts=(0, 1), starts=pose_like(lc.view_of(c, A, K), pair))
    for corner in ((63, 15), (64, 16), (64, 15), (63, 16)):
        add(f"130 x 34 all free, the goal on a tile's corner cell {corner}", full(34, 130), [corner])
    pocket = full(34, 130, O)
    pocket[15, 63] = F
    pocket[15, 64:70] = F
    pocket[16:20, 69] = F
    add("130 x 34, a goal in a pocket that opens into the next tile only", pocket, [(63, 15)])
    # ---- randoms, goals of every status
    for p_occ in (0.1, 0.4):
        for seed in (1, 2, 3):
            cells = mixed(np.random.default_rng(300 + seed), 50, 40, p_occ, 0.1)
            view = lc.view_of(cells, A, K, -17, -33)
            free = free_cells(view, 11, 4096)
            blocked = [(int(i), int(j)) for j, i in zip(*np.nonzero(cells != F))][:5]
            for n_goals in (1, 3, 4096):
                if n_goals == 1:
                    goals = free[:1]
                elif n_goals == 3:
                    goals = [free[5], blocked[0], (-2, 7)]
                else:
                    pick = np.random.default_rng(seed).integers(0, 40, size=(4096, 2))
                    goals = [free[0], free[0], blocked[1], (40, 3), (3, 50)] + [(int(i), int(j) + 40) for i, j in pick[5:]]      # rows 40 .. 79: mostly outside
                    goals[100] = free[7]
                add(f"40 x 50 random, p_occ {p_occ}, seed {seed}, {n_goals} goals", cells, goals, ox=-17, oy=-33, cuts=(0, 1) if seed == 1 else (0,))
    # ---- the clearance threshold
    for rc in (0, 2):
        add(f"two rooms and a door of 2 cells, Rc {rc}", two_rooms(), [(5, 5)], radius=8, min_clearance=rc / K)
    # ---- the weights
    for cw in (0, 13, 255):
        for neutral in (1, 255):
            add(f"two rooms, cost_weight {cw}, neutral_cost {neutral}", two_rooms(), [(5, 5), (60, 18)], radius=8, connectivities=(8,), cost_weight=cw, neutral_cost=neutral)
    add("two rooms, a field of R 2 below Rt 3 with cost_weight 0", two_rooms(), [(5, 5)], radius=2, connectivities=(8,), cost_weight=0)
    # ---- limits
    add("32768 x 2, sparse walls", sparse_walls(32768, True), [(0, 0), (20000, 1)], radius=4, min_clearance=1 / K)
    add("2 x 32768, sparse walls", sparse_walls(32768, False), [(0, 0), (1, 20000)], radius=4, min_clearance=1 / K)
    return out


# ---------------------------------------------------------------- hand-made grids of the CPU tests
def corridor(n=9):
    """1 x n free"""
    return full(1, n)


def wall_corners():
    """5 x 5: two wall cells that touch at a corner; the diagonal between them is the only way from the lower-left to the upper-right"""
    c = full(5, 5, O)
    c[3:5, 0:2] = F        # lower-left room (rows 3, 4; columns 0, 1)
    c[0:2, 3:5] = F        # upper-right room
    c[2, 2] = F            # the cell between them
    c[3, 2] = O; c[2, 1] = O
    return c


def detour():
    """a one-cell corridor along a wall (short, expensive near the wall) against an open detour (long, cheap): 21 x 30 at R 8"""
    c = full(21, 30)
    c[0, :] = O                    # the wall the corridor runs along
    c[2, 2:28] = O                 # the corridor's other side: row 1 is one cell wide
    return c
