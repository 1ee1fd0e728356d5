"""The distance field and its region update at the limits their code names (DESIGN.md sections 7o and 7p), as plain numpy data:
windows as wide as kMaxFieldSide, kMaxUncappedSide and around the width at which k_field_rows leaves 64 KiB of LDS, R = Rt = T =
kMaxFieldRadius, and updates whose rectangles take every strided loop of occupancy_field_update.hip through a second trip.  The
obstacles are sparse: tests/map_field_rule.py's d2_brute is the reference (d2_separable builds a width x width matrix).
tests/test_map_field_limits_rule_oracle.py checks on the CPU that every case sits on the edge its name says, from the rule and the
launch arithmetic alone; tests/test_map_field_limits_gpu.py asks the library.  The scale is a power of two, so max_distance = R / scale
gives exactly R cells."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import map_field_cases as fc
import map_field_rule as rule
import map_field_update_cases as uc
import map_localize_cases as lc

U, O, F = lc.U, lc.O, lc.F
A, K = fc.A, fc.K
LimitCase = namedtuple("LimitCase", "name view radius obstacles stats")        # stats: counters of the rule's answer worked out by hand, or {}
LDS_DEFAULT = 64 * 1024                                     # the dynamic LDS a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize
COUNT_THREADS = 2048 * 256                                  # k_field_count: at most 2048 workgroups of 256 threads, a thread a quad of cells
brute = functools.partial(rule.d2_brute, chunk=65536)


def sparse(width, height, obstacles, unknown=()):
    """free cells with obstacles at (column, row) of `obstacles` and unknown cells at those of `unknown`"""
    cells = np.full((height, width), F, dtype=np.uint8)
    for i, j in obstacles:
        cells[j, i] = O
    for i, j in unknown:
        cells[j, i] = U
    return cells


def stride4(width):
    """the row stride of the field's own arrays (map_field_plan.hpp's field_stride)"""
    return (width + 3) & ~3


def rows_lds_bytes(width):
    """the dynamic LDS of k_field_rows: a row of uint16 column distances rounded to 16 bytes, and four waves' three counters"""
    return ((2 * stride4(width) + 15) & ~15) + 4 * 3 * 4


def field_cases():
    out = []

    def add(name, cells, radius, stats=None, ox=0, oy=0):
        out.append(LimitCase(name, uc.view(cells, ox, oy), radius, rule.OCCUPIED, stats or {}))

    add("32768 x 2, R 3", sparse(32768, 2, [(0, 0), (1024, 0), (16384, 0), (1023, 1), (32744, 1), (32767, 1)]), 3, dict(n_far=65484, max_d2=9))
    add("32744 x 1, R 3: the last width within 64 KiB of LDS", sparse(32744, 1, [(0, 0), (16000, 0), (32743, 0)]), 3)
    add("32745 x 1, R 3: the first width beyond 64 KiB of LDS", sparse(32745, 1, [(0, 0), (16000, 0), (32744, 0)]), 3, ox=-5, oy=7)
    line = sparse(32768, 1, [(0, 0), (5000, 0), (32767, 0)])
    add("32768 x 1, R 1024", line, 1024, dict(n_far=28669, max_d2=1048576))
    add("1 x 32768, R 1024", line.T.copy(), 1024, dict(n_far=28669, max_d2=1048576))
    add("4096 x 3, uncapped, the obstacle in a corner", sparse(4096, 3, [(0, 0)]), 0, dict(n_far=0, max_d2=16769029))
    add("3 x 4096, uncapped, the obstacle in a corner", sparse(3, 4096, [(2, 4095)]), 0, dict(n_far=0, max_d2=16769029))
    return out


# ---------------------------------------------------------------- R = Rt = T = 1024 on one window
REACH_INFLATION = dict(inscribed_radius=1.0, inflation_radius=256.0, cost_scaling_factor=0.01)     # Rt = 1024 cells at scale 4: 1024^2 + 1 table entries
REACH_RECTS = [(0, 0, 2100, 3), (1021, 0, 7, 3), (3, 1, 1030, 1), (2099, 2, 1, 1)]                   # window x, y, w, h of the costs_rect calls


def reach_case():
    """2100 x 3 at (-40, 9): one obstacle at (0, 1), one unknown cell at (1500, 2); R = 1024"""
    return LimitCase("2100 x 3, R 1024", uc.view(sparse(2100, 3, [(0, 1)], [(1500, 2)]), -40, 9), 1024, rule.OCCUPIED, {})


def reach_scan(n_beams):
    """a scan whose beams all leave the cell (2, 1) of reach_case() along +x (a fan of 1e-5 rad a beam) and end between columns 40 and
    2090: -> (laser, ranges, sensor pose)"""
    laser = lc.CaseLaser(n_beams, 0.0, 1e-5, 0.1, 600.0, 550.0)
    view = reach_case().view
    pose = np.array([A[0] + (view["ox"] + 2) / K, A[1] + (view["oy"] + 1) / K, 0.0])
    columns = np.linspace(40.0, 2090.0, n_beams) if n_beams > 1 else np.array([900.0])
    return laser, (columns - 2.0) / K, pose


# ---------------------------------------------------------------- updates beyond one workgroup's stride
def wide_edit():
    """1300 x 12 at (-3, 2), R 3: `before`, `after` with the cells (6, 2) and (1289, 9) flipped -- a box of changed obstacles 1284
    columns wide that begins off a multiple of 4 -- and `third`, `after` with cells of columns 600 .. 610 flipped"""
    rng = np.random.default_rng(1300)
    before = fc.mixed(rng, 12, 1300, 0.01)
    flip = lambda cells, j, i: O if cells[j, i] != O else F     # noqa: E731
    after = before.copy()
    after[2, 6], after[9, 1289] = flip(before, 2, 6), flip(before, 9, 1289)
    third = after.copy()
    third[4, 600], third[7, 610] = flip(after, 4, 600), flip(after, 7, 610)
    return tuple(uc.view(c, -3, 2) for c in (before, after, third))


WIDE_BANDS = (1, 5, 0)


def widest_edit():
    """32768 x 3, R 3: the cells (2, 0) and (32765, 2) flipped; the row pass stages the whole row, 65 536 bytes"""
    before = sparse(32768, 3, [(100, 1), (20000, 0), (32765, 2)])
    after = before.copy()
    after[0, 2], after[2, 32765] = O, F
    return uc.view(before), uc.view(after)


def count_edit():
    """2052 x 1024 at (11, -6), R 8: six obstacles, then one more cell toggled.  513 x 1024 quads: k_field_count's threads take a
    second trip"""
    before = sparse(2052, 1024, [(0, 0), (2051, 0), (0, 1023), (2051, 1023), (1026, 512), (2000, 700)])
    after = before.copy()
    after[300, 777] = O
    return uc.view(before, 11, -6), uc.view(after, 11, -6)
