"""The cases of a field that follows its map (kh_map_field_update) as plain numpy data: windows before and after
an edit, the rectangle the caller names, and what the update must report -- worked out here from the two windows alone (expected()),
never from the library.  tests/test_map_field_update_rule_oracle.py runs the region rule on them on the CPU,
tests/test_map_field_update_gpu.py the library.  The scale is a power of two, so max_distance = R / scale gives exactly R cells."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import map_field_cases as fc
import map_field_rule as rule
import map_localize_cases as lc

U, O, F = lc.U, lc.O, lc.F
A, K = fc.A, fc.K
SHAPES = [(1, 1), (1, 7), (7, 1), (13, 7), (65, 3), (3, 65), (130, 70)]         # width x height
RADII = (1, 3, 11)
BANDS = (1, 4, 5, 0)                                        # forced band heights; 0: the library's choice
NONE = (0, 0, 0, 0)
Edit = namedtuple("Edit", "name before after radius obstacles rect")           # before / after: view dicts of one window; rect: lattice x, y, w, h or None


def view(cells, ox=0, oy=0):
    return lc.view_of(cells, A, K, ox, oy)


def window_cells(v):
    return v["cells"][:v["height"], :v["width"]]


def box_of(mask):
    """window (x, y, w, h) of the True cells, or None"""
    if not mask.any():
        return None
    j, i = np.nonzero(mask)
    return int(i.min()), int(j.min()), int(i.max() - i.min() + 1), int(j.max() - j.min() + 1)


def clip(rect, width, height):
    """window (x, y, w, h) clipped to the window, or None"""
    x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[0] + rect[2], width), min(rect[1] + rect[3], height)
    return (x0, y0, x1 - x0, y1 - y0) if rect[2] > 0 and rect[3] > 0 and x1 > x0 and y1 > y0 else None


def grow(box, by_x, by_y, width, height):
    return clip((box[0] - by_x, box[1] - by_y, box[2] + 2 * by_x, box[3] + 2 * by_y), width, height)


def lattice(box, v):
    return NONE if box is None else (box[0] + v["ox"], box[1] + v["oy"], box[2], box[3])


def expected(before, after, radius, obstacles, rect=None):
    """what kh_field_update must hold after a region update from `before` to `after` (the same window) with `rect`"""
    w, h = after["width"], after["height"]
    compared = (0, 0, w, h) if rect is None else clip((rect[0] - after["ox"], rect[1] - after["oy"], rect[2], rect[3]), w, h)
    inside = np.zeros((h, w), dtype=bool)
    if compared:
        inside[compared[1]:compared[1] + compared[3], compared[0]:compared[0] + compared[2]] = True
    b, a = window_cells(before), window_cells(after)
    assert (b == a)[~inside].all(), "the caller's promise: cells outside rect equal the snapshot"
    states = box_of((b != a) & inside)
    obst = box_of((rule.obstacle_mask(before, obstacles) != rule.obstacle_mask(after, obstacles)) & inside)
    values = grow(obst, radius, radius, w, h) if obst else None
    return dict(rebuilt=0, relayout=0, cells_box=lattice(states, after), values_box=lattice(values, after),
                cells_recomputed=values[2] * values[3] if values else 0, cells_compared=compared[2] * compared[3] if compared else 0)


def rebuilt(after, relayout=0):
    whole = (after["ox"], after["oy"], after["width"], after["height"])
    return dict(rebuilt=1, relayout=relayout, cells_box=whole, values_box=whole, cells_recomputed=after["width"] * after["height"], cells_compared=0)


def shape_edits():
    """every window shape x R: a mixed window, and the same with a few cells flipped -- among them the last column's last cell"""
    out = []
    rng = np.random.default_rng(77)
    for w, h in SHAPES:
        before = fc.mixed(rng, h, w)
        after = before.copy()
        after[h - 1, w - 1] = F if before[h - 1, w - 1] == O else O
        if w * h > 4:
            after[h // 2, w // 3] = F if before[h // 2, w // 3] == O else O
        for r in RADII:
            out.append(Edit(f"{w} x {h}, R {r}", view(before, -3, 2), view(after, -3, 2), r, rule.OCCUPIED, None))
    return out


PLACES = ["corner 00", "corner w0", "corner 0h", "corner wh", "edge top", "edge bottom", "edge left", "edge right", "middle"]


def place(name, w, h):
    return {"corner 00": (0, 0), "corner w0": (w - 1, 0), "corner 0h": (0, h - 1), "corner wh": (w - 1, h - 1), "edge top": (w // 2, 0),
            "edge bottom": (w // 2, h - 1), "edge left": (0, h // 2), "edge right": (w - 1, h // 2), "middle": (w // 2, h // 2)}[name]


def single_cell_edits(kind, w=21, h=18, r=3):
    """kind: "added" (one obstacle into an empty map), "only removed" (every value becomes FAR), "neighbour removed" (one of two
    adjacent obstacles goes: distances GROW)"""
    out = []
    for name in PLACES:
        i, j = place(name, w, h)
        empty = np.full((h, w), F, dtype=np.uint8)
        one = empty.copy()
        one[j, i] = O
        two = one.copy()
        two[j + (1 if j + 1 < h else -1), i] = O
        before, after = {"added": (empty, one), "only removed": (one, empty), "neighbour removed": (two, one)}[kind]
        out.append(Edit(f"{kind} at {name}", view(before, 5, -40), view(after, 5, -40), r, rule.OCCUPIED, None))
    return out


def state_only_edit(obstacles):
    """unknown -> free in a block: no obstacle changes under OCCUPIED, every cell of the block does under NOT_FREE"""
    rng = np.random.default_rng(5)
    before = fc.mixed(rng, 30, 37)
    before[10:14, 20:26] = U
    after = before.copy()
    after[10:14, 20:26] = F
    return Edit(f"unknown -> free, policy {obstacles}", view(before, -8, 3), view(after, -8, 3), 3, obstacles, None)


def rect_forms():
    """one edit inside columns 20 .. 25, rows 10 .. 13 of a 37 x 30 window at (-8, 3), named by different rectangles"""
    e = state_only_edit(rule.NOT_FREE)
    ox, oy = e.before["ox"], e.before["oy"]
    rects = [("NULL", None), ("the window", (ox, oy, 37, 30)), ("tight", (ox + 20, oy + 10, 6, 4)), ("partly outside", (ox + 18, oy + 8, 100, 100)),
             ("across the low corner", (ox - 50, oy - 50, 77, 65))]
    return [Edit(f"rect {name}", e.before, e.after, e.radius, e.obstacles, rect) for name, rect in rects]


OUTSIDE_RECTS = [(100, 100, 5, 5), (-8 - 10, 3, 10, 30), (-8, 3 + 30, 37, 4), (0, 10, 0, 5), (0, 10, 5, -1)]       # wholly outside the window of rect_forms(), or empty


def random_rounds(density, obstacles, rounds=30, seed=0):
    """40 x 50 at (-17, -33): yields (after view, rect) round by round, each a random rectangle rewritten at `density` occupied"""
    rng = np.random.default_rng(1000 + seed)
    cells = fc.mixed(rng, 50, 40, density)
    yield view(cells, -17, -33), None
    for _ in range(rounds):
        x0, y0 = int(rng.integers(0, 40)), int(rng.integers(0, 50))
        w, h = int(rng.integers(1, 41 - x0)), int(rng.integers(1, 51 - y0))
        cells = cells.copy()
        cells[y0:y0 + h, x0:x0 + w] = fc.mixed(rng, h, w, density)
        yield view(cells, -17, -33), (x0 - 17, y0 - 33, w, h)
