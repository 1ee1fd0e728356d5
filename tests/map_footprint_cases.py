"""TEST INFRASTRUCTURE (not a test): the hand-made views, footprints and poses of the footprint tests, shared by
tests/test_map_footprint_rule_oracle.py (CPU) and tests/test_map_footprint_gpu.py."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_field_rule as fr
import map_footprint_rule as rule
import map_localize_cases as lc

U, O, F = lc.U, lc.O, lc.F
A = (0.5, -0.25)                                             # the anchor of most views
PoseCase = namedtuple("PoseCase", "name view radius obstacles verts poses")
LayerCase = namedtuple("LayerCase", "name view verts n_headings max_status")


def world(view, i, j):
    """the world point of lattice cell (i, j): anchor + cell / scale"""
    return (view["anchor"][0] + i / view["scale"], view["anchor"][1] + j / view["scale"])


def field_values(case):
    return fr.d2_brute(case.view, case.radius, case.obstacles)


def box(x0, x1, y0, y1, scale):
    """the rectangle whose vertex cells at heading 0 are (x0 | x1, y0 | y1) around the pose's cell: x1 - x0 + 1 columns, y1 - y0 + 1 rows"""
    return [(x1 / scale, y1 / scale), (x0 / scale, y1 / scale), (x0 / scale, y0 / scale), (x1 / scale, y0 / scale)]


def polygon(n, radius, phase=0.1):
    return [(radius * math.cos(phase + 2.0 * math.pi * k / n), radius * math.sin(phase + 2.0 * math.pi * k / n)) for k in range(n)]


ONE_CELL = [(0.001, 0.0), (-0.001, 0.001), (-0.001, -0.001)]
SLIVER = [(0.6, 0.01), (-0.6, 0.02), (-0.6, -0.02)]          # at 4 cells / m every vertex rounds onto the pose's row
RECTANGLE = rule.rectangle(1.0, 0.6)
TRIANGLE = [(0.7, 0.0), (-0.4, 0.5), (-0.4, -0.3)]
DIAMOND_255 = [(63.5, 0.0), (0.0, 63.5), (-63.5, 0.0), (0.0, -63.5)]       # at 4 cells / m: 254 cells out, reach 255, 509 rows
LONG_64 = [(15.7, 1.0), (-15.7, 1.0), (-15.7, -1.0), (15.7, -1.0)]         # at 4 cells / m: reach 64
SMALL_2 = [(0.25, 0.0), (-0.2, 0.15), (-0.2, -0.15)]                       # at 4 cells / m: reach 2, the smallest there is


def edge_poses(view, theta=0.3):
    """poses on every edge and corner of the window, inside, and wholly outside"""
    w, h, ox, oy = view["width"], view["height"], view["ox"], view["oy"]
    cells = [(ox, oy), (ox + w - 1, oy), (ox, oy + h - 1), (ox + w - 1, oy + h - 1), (ox + w // 2, oy), (ox + w // 2, oy + h - 1), (ox, oy + h // 2),
             (ox + w - 1, oy + h // 2), (ox + w // 2, oy + h // 2), (ox - 400, oy), (ox + w + 300, oy + h + 300), (ox + w // 3, oy - 1), (ox + w, oy + h // 3)]
    return [world(view, i, j) + (theta * (k - 4),) for k, (i, j) in enumerate(cells)]


def random_view(seed, h, w, scale, ox=0, oy=0, p_free=0.8, p_occ=0.05, anchor=A):
    return lc.view_of(lc.random_cells(np.random.default_rng(seed), h, w, p_free=p_free, p_occ=p_occ), anchor, scale, ox, oy)


def pose_cases():
    out = []
    one = lc.view_of(np.array([[F]]), A, 4.0, 3, -2)
    for state, name in ((F, "free"), (O, "occupied"), (U, "unknown"), (7, "of state 7")):
        v = lc.view_of(np.array([[state]]), A, 4.0, 3, -2)
        out.append(PoseCase(f"1 x 1 {name}, the single cell on it and off it", v, 2, fr.OCCUPIED, ONE_CELL, [world(v, 3, -2) + (0.0,), world(v, 4, -2) + (1.0,)]))
    out.append(PoseCase("1 x 1, the rectangle over it", one, 0, fr.OCCUPIED, RECTANGLE, [world(one, 3, -2) + (0.5,), world(one, 9, -2) + (0.5,)]))
    v35 = random_view(1, 5, 3, 4.0, -1, -2)
    out.append(PoseCase("3 x 5, the sliver and a negative origin", v35, 2, fr.NOT_FREE, SLIVER, edge_poses(v35, 0.0) + [world(v35, 0, 0) + (0.0,)]))
    v65 = random_view(2, 17, 65, 20.0, -7, -3)
    angles = [0.0, math.radians(30), math.radians(45), math.radians(90), math.radians(180), -0.7]
    out.append(PoseCase("65 x 17, the rectangle at six angles, R 3 leaves far values", v65, 3, fr.OCCUPIED, RECTANGLE,
                        [world(v65, 20, 5) + (a,) for a in angles] + edge_poses(v65)))
    v63 = random_view(3, 16, 63, 20.0, 5, 9, p_free=0.6, p_occ=0.02)
    out.append(PoseCase("63 x 16 (a width off the dword), obstacles NOT_FREE, the triangle", v63, 0, fr.NOT_FREE, TRIANGLE, edge_poses(v63)))
    out.append(PoseCase("63 x 16, the triangle wound the other way", v63, 0, fr.NOT_FREE, TRIANGLE[::-1], edge_poses(v63)))
    out.append(PoseCase("65 x 17, a 16-gon", v65, 8, fr.OCCUPIED, polygon(16, 0.45), edge_poses(v65, 0.11)))
    wide = random_view(4, 70, 160, 20.0, -80, -35, p_free=0.9, p_occ=0.01)
    for cols in (63, 64, 65):
        out.append(PoseCase(f"160 x 70, spans {cols} cells wide", wide, 5, fr.OCCUPIED, box(-31, cols - 32, -2, 3, 20.0),
                            [world(wide, 0, 0) + (0.0,), world(wide, -70, 30) + (0.0,), world(wide, 3, -4) + (math.pi,)]))
    for rows in (64, 65):
        out.append(PoseCase(f"160 x 70, {rows} rows", wide, 5, fr.OCCUPIED, box(-3, 2, -31, rows - 32, 20.0),
                            [world(wide, 0, 0) + (0.0,), world(wide, 60, -30) + (0.0,), world(wide, 1, 1) + (-math.pi / 2,)]))
    v4 = random_view(5, 17, 65, 4.0, -30, -8)
    out.append(PoseCase("65 x 17 at 4 cells / m, reach 255: 509 rows", v4, 4, fr.OCCUPIED, DIAMOND_255, [world(v4, 0, 0) + (0.0,), world(v4, 200, -100) + (0.4,),
                        world(v4, 0, 0) + (math.pi / 4,)]))
    return out


def lattice_poses(view):
    """the single-cell footprint on +-2^30 cells and just beyond, in x and in y (anchor and scale 4 of `view`)"""
    ax, ay = view["anchor"]
    on, beyond = 2.0 ** 28, 2.0 ** 28 + 0.25
    return [(ax + on, ay, 0.0), (ax + beyond, ay, 0.0), (ax - on, ay, 0.0), (ax - beyond, ay, 0.0), (ax, ay + on, 0.0), (ax, ay + beyond, 0.0), (ax, ay - on, 0.0),
            (ax, ay - beyond, 0.0), (1e300, 0.0, 0.0), (0.0, -1e300, 1e300)]


def layer_cases():
    out = []
    blocky = np.full((40, 130), F, dtype=np.uint8)
    blocky[12:21, 60:69] = O                                  # the tile edges at column 64 and row 16 run through it
    blocky[30:33, 100:128] = U
    blocky[0:2, 10:30] = 7
    vb = lc.view_of(blocky, A, 20.0, -9, 4)
    for h, ms in ((1, 0), (7, 1), (32, 2), (7, 0), (32, 0)):
        out.append(LayerCase(f"130 x 40 with a block on a tile corner, the rectangle, H {h}, max_status {ms}", vb, RECTANGLE, h, ms))
    v4 = lc.view_of(blocky[:33, :70], A, 4.0, 2, -5)
    for ms in (0, 1, 2):
        out.append(LayerCase(f"70 x 33 at 4 cells / m, reach 2, H 7, max_status {ms}", v4, SMALL_2, 7, ms))
        out.append(LayerCase(f"70 x 33 at 4 cells / m, reach 64, H 7, max_status {ms}", v4, LONG_64, 7, ms))
    narrow = random_view(6, 3, 5, 4.0, 0, 0)
    out.append(LayerCase("5 x 3, narrower than the halo of reach 64, H 32, max_status 2", narrow, LONG_64, 32, 2))
    out.append(LayerCase("5 x 3, reach 2, H 32, max_status 1", narrow, SMALL_2, 32, 1))
    free = lc.view_of(np.full((20, 70), F, dtype=np.uint8), A, 20.0, 0, 0)
    unknown = lc.view_of(np.full((20, 70), U, dtype=np.uint8), A, 20.0, 0, 0)
    for ms in (0, 1, 2):
        out.append(LayerCase(f"70 x 20 all free, H 7, max_status {ms}", free, RECTANGLE, 7, ms))
        out.append(LayerCase(f"70 x 20 all unknown, H 7, max_status {ms}", unknown, RECTANGLE, 7, ms))
    return out
