"""TEST INFRASTRUCTURE (not a test): the rule of the travel costs in Python -- what kh_map_travel_* must
compute.  It reads nothing of the library.  The field's values and the cost table are tests/map_field_rule.py's, the lattice cell of a
point tests/map_localize_rule.py's.

  inputs      the field's snapshot of the cell states and its d2 values over the field's window; cells outside the window do not
              exist, columns width .. width_step - 1 are never read
  Rc, Rt      ceil(min_clearance * scale), ceil(inflation_radius * scale): the field's own radius_cells; a field with 0 < R < Rc is
              refused, and with cost_weight > 0 one with 0 < R < Rt
  traversable state 255 and d2 >= Rc * Rc (FAR counts as beyond)
  weight      q(v) = neutral_cost + ((cost_weight * c(v)) >> 4) for a traversable cell, c(v) = table[d2] for d2 <= Rt * Rt, else 0;
              q = 0 for every other cell
  steps       n = 0 .. 7: (+1,0), (0,+1), (-1,0), (0,-1), (+1,+1), (-1,+1), (-1,-1), (+1,-1); connectivity 4 has 0 .. 3 only;
              L(n) = 5 for n < 4, else 7.  u -> v is allowed when v is a traversable window cell; a diagonal step (di, dj) from (i, j)
              only with cut_corners, or when both (i + di, j) and (i, j + dj) are traversable.  The step costs L(n) * q(u).
  values      V = 0 at every goal cell; elsewhere the minimum over allowed steps u -> v of V(v) + L * q(u); FAR where no goal is
              reached and at every cell that is not traversable.  A window with width * height * Lmax * q_max > 0xFFFFFFFE is refused.
  goal        the traversable window cell within Chebyshev distance goal_snap_cells of the point's cell with the smallest key
              dist2 << 32 | window index; GOAL_BLOCKED without one; GOAL_OUTSIDE where the point's own cell is off the window or
              beyond +-2^30 cells
  lookup      the window cell within Chebyshev distance snap_cells of the point's cell with the smallest key V << 32 | window index
              among those with V != FAR: AT_OK, its value and lattice cell; AT_UNREACHED / AT_OUTSIDE: FAR and (0, 0)
  path        the start cell is the lookup's; emit it; while V(cur) != 0 go to the allowed neighbour of the smallest direction index
              with V(v) + L * q(cur) == V(cur); PATH_TRUNCATED when max_cells cells are out and the last is no goal cell
"""
from __future__ import annotations

import heapq
import math

import numpy as np

import map_field_rule as fr
import map_localize_rule as ml

FAR = 0xFFFFFFFF
GOAL_OK, GOAL_BLOCKED, GOAL_OUTSIDE = 0, 1, 2
AT_OK, AT_UNREACHED, AT_OUTSIDE = 0, 1, 2
PATH_OK, PATH_TRUNCATED, PATH_UNREACHED, PATH_OUTSIDE = 0, 1, 2, 3
STEPS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))       # (di, dj) of direction n
LENGTH = (5, 5, 5, 5, 7, 7, 7, 7)
MAX_GOALS, MAX_SNAP, MAX_PATH_CELLS, MAX_PATH_BUFFER = 4096, 16, 65536, 1 << 24
PARAMS = dict(min_clearance=0.0, connectivity=8, cut_corners=0, neutral_cost=50, cost_weight=13, goal_snap_cells=0)
Refused = fr.Refused


def split(params):
    """(the travel parameters over their defaults, the inflation parameters over theirs)"""
    p, inflation = dict(PARAMS), dict(fr.INFLATION)
    for k, v in params.items():
        (inflation if k in inflation else p)[k] = v
    return p, inflation


def params_check(p, inflation, scale):
    """-> (Rc, Rt); Refused in the library's order"""
    if p["connectivity"] not in (4, 8):
        raise Refused("connectivity")
    if p["cut_corners"] not in (0, 1):
        raise Refused("cut_corners")
    if not 1 <= p["neutral_cost"] <= 255:
        raise Refused("neutral_cost")
    if not 0 <= p["cost_weight"] <= 255:
        raise Refused("cost_weight")
    if not 0 <= p["goal_snap_cells"] <= MAX_SNAP:
        raise Refused("goal_snap_cells")
    if not (math.isfinite(p["min_clearance"]) and p["min_clearance"] >= 0.0):
        raise Refused("min_clearance")
    rc = fr.radius_cells(p["min_clearance"], scale)
    try:
        rt = fr.inflation_check(inflation, scale)
    except Refused:
        raise Refused("inflation") from None
    return rc, rt


def q_max(neutral_cost, cost_weight):
    return neutral_cost + ((cost_weight * 253) >> 4)


def overflows(width, height, connectivity, qmax):
    return width * height * (7 if connectivity == 8 else 5) * qmax > 0xFFFFFFFE


def field_check(p, rc, rt, radius, width, height):
    """what is refused once the field is known, in the library's order"""
    if 0 < radius < rc:
        raise Refused("reach of the clearance")
    if p["cost_weight"] > 0 and 0 < radius < rt:
        raise Refused("reach of the inflation")
    if overflows(width, height, p["connectivity"], q_max(p["neutral_cost"], p["cost_weight"])):
        raise Refused("overflow")


def weights(view, d2, rc, rt, p, inflation):
    """(height, width) uint16: q"""
    h, w = view["height"], view["width"]
    win = view["cells"][:h, :w]
    d2 = np.asarray(d2, dtype=np.int64)
    traversable = (win == 255) & (d2 >= rc * rc)
    c = np.zeros((h, w), dtype=np.int64)
    if p["cost_weight"] > 0:
        table = fr.cost_table(view["scale"], **inflation).astype(np.int64)
        c = np.where(d2 <= rt * rt, table[np.minimum(d2, rt * rt)], 0)
    return np.where(traversable, p["neutral_cost"] + ((p["cost_weight"] * c) >> 4), 0).astype(np.uint16)


def step_masks(q, connectivity, cut_corners):
    """(height, width) uint8: bit n set where the step in direction n is allowed from the cell"""
    h, w = q.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = q > 0
    at = lambda di, dj: pad[1 + dj:1 + dj + h, 1 + di:1 + di + w]  # noqa: E731
    out = np.zeros((h, w), dtype=np.uint8)
    for n, (di, dj) in enumerate(STEPS[:connectivity]):
        ok = at(0, 0) & at(di, dj)
        if n >= 4 and not cut_corners:
            ok = ok & at(di, 0) & at(0, dj)
        out |= (ok.astype(np.uint8) << n).astype(np.uint8)
    return out


def opposite(n):
    return (n + 2) % 4 if n < 4 else 4 + (n - 2) % 4


def dijkstra(q, goal_cells, connectivity, cut_corners):
    """(height, width) uint32 values by a heap Dijkstra from the goal cells: settling v relaxes every u with an allowed step u -> v --
    allowedness is symmetric, so those are the cells v may step to -- at V(v) + L * q(u)"""
    h, w = q.shape
    masks = step_masks(q, connectivity, cut_corners).ravel().tolist()
    weight = q.ravel().astype(np.int64).tolist()
    value = [FAR] * (h * w)
    heap = []
    for g in sorted(set(goal_cells)):
        value[g] = 0
        heap.append((0, g))
    offsets = [dj * w + di for di, dj in STEPS]
    while heap:
        d, v = heapq.heappop(heap)
        if d != value[v]:
            continue
        m = masks[v]
        n = 0
        while m:
            if m & 1:
                u = v + offsets[n]
                through = d + LENGTH[n] * weight[u]
                if through < value[u]:
                    value[u] = through
                    heapq.heappush(heap, (through, u))
            m >>= 1
            n += 1
    return np.array(value, dtype=np.uint64).astype(np.uint32).reshape(h, w)


def point_cell(view, x, y):
    """the window column and row of a world point's cell, None where the goal / lookup rule says OUTSIDE"""
    cx, cy = ml.lattice_cell(x, view["anchor"][0], view["scale"]), ml.lattice_cell(y, view["anchor"][1], view["scale"])
    if max(abs(cx), abs(cy)) > 2 ** 30:
        return None
    wx, wy = cx - view["ox"], cy - view["oy"]
    return (wx, wy) if 0 <= wx < view["width"] and 0 <= wy < view["height"] else None


def snap_square(view, wx, wy, snap):
    for j in range(max(0, wy - snap), min(view["height"], wy + snap + 1)):
        for i in range(max(0, wx - snap), min(view["width"], wx + snap + 1)):
            yield i, j


def goal_cells(view, q, goals, snap):
    """-> (status (n,) int32, cell (n,) int64 window index or FAR)"""
    status, cells = [], []
    for x, y in np.asarray(goals, dtype=np.float64).reshape(-1, 2):
        at = point_cell(view, x, y)
        if at is None:
            status.append(GOAL_OUTSIDE); cells.append(FAR)
            continue
        keys = [(((i - at[0]) ** 2 + (j - at[1]) ** 2) << 32) | (j * view["width"] + i) for i, j in snap_square(view, at[0], at[1], snap) if q[j, i] > 0]
        status.append(GOAL_OK if keys else GOAL_BLOCKED); cells.append(min(keys) & 0xFFFFFFFF if keys else FAR)
    return np.array(status, dtype=np.int32), np.array(cells, dtype=np.int64)


def analyse(view, d2, radius, goals, **params):
    """a create and one solve -> dict(values, weights, goal_status, goal_cells, stats)"""
    p, inflation = split(params)
    rc, rt = params_check(p, inflation, view["scale"])
    field_check(p, rc, rt, radius, view["width"], view["height"])
    q = weights(view, d2, rc, rt, p, inflation)
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, 2)
    if not 1 <= len(goals) <= MAX_GOALS or not np.isfinite(goals).all():
        raise Refused("goals")
    status, cells = goal_cells(view, q, goals, p["goal_snap_cells"])
    values = dijkstra(q, [int(c) for c, s in zip(cells, status) if s == GOAL_OK], p["connectivity"], p["cut_corners"])
    reached = values[values != FAR]
    stats = dict(ox=view["ox"], oy=view["oy"], width=view["width"], height=view["height"], clearance_cells=rc, inflation_cells=rt,
                 connectivity=p["connectivity"], n_traversable=int((q > 0).sum()), n_reached=int(reached.size), max_value=int(reached.max()) if reached.size else 0)
    return dict(values=values, weights=q, goal_status=status, goal_cells=cells, stats=stats, params=p)


def lookup(view, values, xy, snap=0):
    """-> (status (n,) int32, value (n,) uint32, cell (n, 2) int32 lattice cells)"""
    status, value, cell = [], [], []
    for x, y in np.asarray(xy, dtype=np.float64).reshape(-1, 2):
        at = point_cell(view, x, y)
        if at is None:
            status.append(AT_OUTSIDE); value.append(FAR); cell.append((0, 0))
            continue
        keys = [(int(values[j, i]) << 32) | (j * view["width"] + i) for i, j in snap_square(view, at[0], at[1], snap) if values[j, i] != FAR]
        if not keys:
            status.append(AT_UNREACHED); value.append(FAR); cell.append((0, 0))
            continue
        index = min(keys) & 0xFFFFFFFF
        status.append(AT_OK); value.append(min(keys) >> 32); cell.append((view["ox"] + index % view["width"], view["oy"] + index // view["width"]))
    return np.array(status, dtype=np.int32), np.array(value, dtype=np.uint32), np.array(cell, dtype=np.int32).reshape(-1, 2)


def paths(view, values, q, xy, snap, max_cells, connectivity, cut_corners):
    """-> a list of dict(status, n_cells, cost, start_cell, cells (n_cells, 2) int32 lattice cells)"""
    w = view["width"]
    masks = step_masks(q, connectivity, cut_corners)
    status, value, cell = lookup(view, values, xy, snap)
    out = []
    for s, v, (cx, cy) in zip(status, value, cell):
        if s != AT_OK:
            out.append(dict(status=PATH_OUTSIDE if s == AT_OUTSIDE else PATH_UNREACHED, n_cells=0, cost=FAR, start_cell=FAR, cells=np.zeros((0, 2), dtype=np.int32)))
            continue
        i, j = int(cx) - view["ox"], int(cy) - view["oy"]
        cells, code = [(i, j)], None
        while code is None:
            here = int(values[j, i])
            if here == 0:
                code = PATH_OK
            elif len(cells) == max_cells:
                code = PATH_TRUNCATED
            else:
                nxt = [n for n in range(8) if (masks[j, i] >> n) & 1 and values[j + STEPS[n][1], i + STEPS[n][0]] != FAR and
                       int(values[j + STEPS[n][1], i + STEPS[n][0]]) + LENGTH[n] * int(q[j, i]) == here]
                assert nxt, "a cell of a solved field that no neighbour explains"
                i, j = i + STEPS[nxt[0]][0], j + STEPS[nxt[0]][1]
                cells.append((i, j))
        lattice = np.array(cells, dtype=np.int32) + np.array([view["ox"], view["oy"]], dtype=np.int32)
        out.append(dict(status=code, n_cells=len(cells), cost=int(v), start_cell=(int(cy) - view["oy"]) * w + int(cx) - view["ox"], cells=lattice))
    return out


def cell_world(view, cells):
    """the world points of lattice cells by the view's rule: anchor + cell / scale, in doubles"""
    cells = np.asarray(cells, dtype=np.int32).reshape(-1, 2)
    ax, ay, scale = float(view["anchor"][0]), float(view["anchor"][1]), float(view["scale"])
    return np.stack([ax + cells[:, 0].astype(np.float64) / scale, ay + cells[:, 1].astype(np.float64) / scale], axis=1)


def rank(view, values, clusters, snap=0):
    """frontier records ordered by (the value at anchor_xy, id), the unreached ones last in id order -> a list of (id, value or None)"""
    if not clusters:
        return []
    status, value, _ = lookup(view, values, [c["anchor_xy"] for c in clusters], snap)
    reached = sorted((int(value[k]), k) for k in range(len(clusters)) if status[k] == AT_OK)
    return [(k, v) for v, k in reached] + [(k, None) for k in range(len(clusters)) if status[k] != AT_OK]


def tile_grid(width, height):
    """the 64 x 16-cell tiles of a window: (tiles across, tiles down)"""
    return (width + 63) // 64, (height + 15) // 16


def flagged(tx, ty, tiles_x, tiles_y, connectivity, lowered):
    """the neighbour tiles tile (tx, ty) flags, as a mask over the directions, from the mask of its lowered perimeter parts"""
    out = 0
    for n, (di, dj) in enumerate(STEPS[:connectivity]):
        if 0 <= tx + di < tiles_x and 0 <= ty + dj < tiles_y and (lowered >> n) & 1:
            out |= 1 << n
    return out


def path_buffer_ok(n, max_cells):
    return n >= 1 and 1 <= max_cells <= MAX_PATH_CELLS and n * max_cells <= MAX_PATH_BUFFER
