"""Inputs of the map change layer's kernels (k_map_observe, k_map_diff, k_map_changed, k_map_decay in csrc/occupancy_changes.hip) as plain numpy
data, and the changed world of its end-to-end test.  tests/test_map_changes_gpu.py asks the library and tests/map_changes_rule.py for
the same cases and compares exactly; tests/test_map_changes_rule_oracle.py checks the changed world's three geometric statements with
the rule alone.

The capped launches.  The changed-cell list is built by k_map_changed on min(ceil(n_units / 4), 1024) workgroups of four waves, a wave
a unit of 64 cells of a row, so a wave's strided loop takes a second trip from 4097 units on; k_map_changed_scan is one workgroup of
1024 threads with ceil(n_units / 1024) units each, more than one from 1025 units on.  unit_cases() holds views of 1023 .. 35 200 units
around both thresholds (a 2000 x 2000 map has 64 000); test_unit_case_sits_on_its_edges asserts with the rule that each of them
puts changes on the first and last unit of every trip and of three threads' ranges.  (The end-to-end tests' small map holds 4592
units, so they reach a second trip too -- with whatever changed cells the world puts there, none at a threshold.)  k_map_diff and k_map_decay launch one thread per
cell of the strided window without a cap."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_localize_cases as mlc
import map_localize_rule as ml

U, O, F = mlc.U, mlc.O, mlc.F
ObserveCase = namedtuple("ObserveCase", "name view laser ranges poses tolerance")
TOLERANCES = (0, 1, 2, 4)


def observe_cases():
    """the views, lasers and poses of map_localize_cases.fit_cases() with "pose" read as "scan": scan 0 has the case's readings, every
    further scan a random vector of its own between the case's smallest and largest finite reading; the tolerance cycles through 0, 1, 2, 4"""
    rng = np.random.default_rng(29)
    out = []
    for k, c in enumerate(mlc.fit_cases()):
        finite = c.ranges[np.isfinite(c.ranges)]
        ranges = [c.ranges]
        for _ in range(1, len(c.poses)):
            ranges.append(rng.uniform(finite.min(), finite.max(), size=c.ranges.shape) if finite.size and finite.min() < finite.max() else c.ranges)
        out.append(ObserveCase(c.name.replace("poses", "scans"), c.view, c.laser, np.array(ranges), c.poses, TOLERANCES[k % 4]))
    return out


def spot_laser():
    """one beam of (almost) no length: the sensor's cell is the end cell, visited by the line and once more as the hit -- pass 2, hits 1"""
    return mlc.circle(1, min_range=0.0)


def spots(view, cells):
    """the poses that put one zero-length beam on each lattice cell of `cells` (scale 4, a cell's centre), and their readings"""
    poses = np.array([(view["anchor"][0] + i / view["scale"], view["anchor"][1] + j / view["scale"], 0.0) for i, j in cells])
    return np.full((len(cells), 1), 1e-9), poses


def wide_view(width=130, height=3, ox=-7, oy=11, fill=F):
    """a window whose width is no multiple of 64: units 0 .. 63, 64 .. 127 and the ragged 128 .. 129 in every row"""
    return mlc.view_of(np.full((height, width), fill, dtype=np.uint8), (-1.0, 0.5), 4.0, ox, oy)


def corner_view():
    """13 x 9 free cells with occupied cells two cells from the first and three cells from the last corner: the neighbourhood of an end
    cell in a corner is clipped on two sides, and the tolerance decides"""
    cells = np.full((9, 13), F, dtype=np.uint8)
    cells[2, 2] = O
    cells[5, 9] = O
    return mlc.view_of(cells, (0.0, 0.0), 4.0, -6, -4, padding=O)


# ---------------------------------------------------------------- unit counts around the capped launch of the list kernels
# k_map_changed runs on min(ceil(n_units / 4), 1024) workgroups of four waves, a wave a unit: TRIP_UNITS units per trip of its strided
# loop.  k_map_changed_scan is one workgroup of SCAN_THREADS threads, thread t summing the units [t per, (t + 1) per) clamped to n_units,
# per = ceil(n_units / SCAN_THREADS).  The hand-made views above hold nine units at the most.
TRIP_UNITS, SCAN_THREADS = 4096, 1024
UnitCase = namedtuple("UnitCase", "name view laser ranges poses min_pass threshold caps n_units")
UNIT_SHAPES = ((1, 1023), (1, 1024), (65, 512), (1, 1025), (65, 513), (1, 2048), (65, 1024), (1, 2049), (1, 4095), (1, 4096), (65, 2048),
               (1, 4097), (65, 2049), (1, 8193), (2048, 1100))
DECAY_CASE, ROOM_CASE = "4097 units (1 x 4097)", "4098 units (65 x 2049)"


def units_of(width, height):
    return -(-width // 64) * height


def scan_range(t, n_units):
    """[lo, hi): the units thread t of the scan sums"""
    per = -(-n_units // SCAN_THREADS)
    lo = min(t * per, n_units)
    return lo, min(lo + per, n_units)


def edge_units(n_units):
    """the first and the last unit of every trip, and of the scan's first, middle and last non-empty thread"""
    out = []
    for first in range(0, n_units, TRIP_UNITS):
        out += [first, min(first + TRIP_UNITS, n_units) - 1]
    last_thread = (n_units - 1) // -(-n_units // SCAN_THREADS)
    for t in (0, last_thread // 2, last_thread):
        lo, hi = scan_range(t, n_units)
        out += [lo, hi - 1]
    return sorted(set(out))


def unit_counts(view, changed):
    """changed (height, width) bool -> the number of set cells per unit, row-major"""
    h, w = view["height"], view["width"]
    padded = np.zeros((h, -(-w // 64) * 64), dtype=np.int64)
    padded[:, :w] = changed[:h, :w]
    return padded.reshape(h, -1, 64).sum(axis=2).ravel()


def unit_view(width, height, seed, ox=0, oy=0, padding=U):
    """random states, half of them free; on a view of more than one column every seventh row all free and every seventh all occupied;
    then an occupied cell into every edge unit that holds no other state than free"""
    rng = np.random.default_rng(seed)
    cells = mlc.random_cells(rng, height, width, p_free=0.5, p_occ=0.3)
    if width > 1:
        rows = np.arange(height)
        cells[rows % 7 == 3] = F
        cells[rows % 7 == 5] = O
    per_row = -(-width // 64)
    for u in edge_units(per_row * height):
        row, x0 = u // per_row, 64 * (u % per_row)
        span = min(64, width - x0)
        if (cells[row, x0:x0 + span] == F).all():
            cells[row, x0 + int(rng.integers(span))] = O
    return mlc.view_of(cells, (-1.0, 0.5), 4.0, ox, oy, padding)


def column_scans(view):
    """one scan per column of the view: a single beam along +y from the centre of the column's first cell to the centre of its last.
    Every cell is passed once, the end cell twice with one hit: at min_pass_through 0 and threshold 0.6 every cell is observed free, so
    the changed cells are the cells of another state than free."""
    h, k = view["height"], view["scale"]
    laser = mlc.CaseLaser(1, math.pi / 2.0, 0.1, 0.1, (h + 20) / k, (h + 10) / k)
    i = np.arange(view["width"])
    poses = np.stack([view["anchor"][0] + (view["ox"] + i) / k, np.full(i.size, view["anchor"][1] + view["oy"] / k), np.zeros(i.size)], axis=1)
    return laser, np.full((i.size, 1), (h - 1) / k), poses


def unit_cases():
    """caps: None, 0, then -- above one trip -- the prefix at unit 4096 exactly and a cap that ends inside the first unit of trip two
    that holds two changes (on a view of one column: behind the first that holds one); else such a cap three quarters into the units"""
    if "units" in _cache:
        return _cache["units"]
    out = []
    for k, (w, h) in enumerate(UNIT_SHAPES):
        ox, oy, padding = ((0, 0, U), (-7, -1000, O), (3, -5, O), (-40, 11, U))[k % 4]
        view = unit_view(w, h, 100 + k, ox, oy, padding)
        laser, ranges, poses = column_scans(view)
        n_units = units_of(w, h)
        counts = unit_counts(view, view["cells"] != F)
        prefix = np.concatenate([[0], np.cumsum(counts)])
        need = 2 if w > 1 else 1
        if n_units > TRIP_UNITS:
            u = TRIP_UNITS + int(np.argmax(counts[TRIP_UNITS:] >= need))
            caps = (None, 0, int(prefix[TRIP_UNITS]), int(prefix[u]) + 1)
        else:
            u = 3 * n_units // 4 - int(np.argmax(counts[3 * n_units // 4::-1] >= need))
            caps = (None, 0, int(prefix[u]) + 1)
        out.append(UnitCase(f"{n_units} units ({w} x {h})", view, laser, ranges, poses, 0, 0.6, caps, n_units))
    _cache["units"] = out
    return out


# ---------------------------------------------------------------- the changed world of the end-to-end test
# tests/relocalize_cases.py's small map (eight scans along the aisle x = 2.5, y = 3 .. 7 of synth.make_world) stays the map.  The world
# changes: a pallet is left across the aisle beyond the last node, and the first rack (x 4 .. 5, y 6 .. 14; 275 beams of the held-out
# scan end on it) is gone.  The scan is ray-cast without noise at the held-out pose.
# The pallet was chosen with the rule alone: a smaller one beside the aisle (0.8, 4.0) .. (1.3, 4.5) left one NOVEL beam that is not the
# pallet's -- a grazing reading on the far wall x = 0 at y = 20.1, 14.8 m away, where the map's wall is one sparse cell wide -- and the
# pallet across the aisle stands in that beam's way.
PALLET = (1.0, 8.0, 2.3, 8.5)
DELETED_RECT = 1                                            # make_world's rectangle 1 (rectangle 0 is the outer wall)
ChangedWorld = namedtuple("ChangedWorld", "pose ranges on_pallet pallet_cells footprint")
_cache = {}


def changed_world():
    if "world" not in _cache:
        import relocalize_cases as rc
        from common import LASER
        from slam_toolbox_amd import synth
        sm, m = mlc.small_map()
        world = synth.make_world(rc.WORLD_SEED)
        gone = world[4 * DELETED_RECT:4 * DELETED_RECT + 4]
        pallet = np.asarray(synth._rect(*PALLET), dtype=np.float64)
        changed = np.vstack([np.delete(world, slice(4 * DELETED_RECT, 4 * DELETED_RECT + 4), axis=0), pallet])
        pose = sm.true_pose.copy()
        ranges = synth.make_scan(changed, pose, np.random.default_rng(0), LASER, noise=0, p_inf=0, p_nan=0)
        alone = synth.raycast(pallet, pose, LASER)
        on_pallet = np.isfinite(alone) & (alone == synth.raycast(changed, pose, LASER))
        a, k = m.view["anchor"], m.view["scale"]
        cells = (ml.lattice_cell(PALLET[0], a[0], k), ml.lattice_cell(PALLET[1], a[1], k), ml.lattice_cell(PALLET[2], a[0], k),
                 ml.lattice_cell(PALLET[3], a[1], k))
        footprint = (gone[:, [0, 2]].min(), gone[:, [1, 3]].min(), gone[:, [0, 2]].max(), gone[:, [1, 3]].max())
        _cache["world"] = ChangedWorld(pose, ranges, on_pallet, cells, footprint)
    return _cache["world"]


def outline_distance(i, j, rect):
    """Chebyshev distance of lattice cell (i, j) from the outline of the lattice rectangle rect = (x0, y0, x1, y1)"""
    x0, y0, x1, y1 = rect
    dx, dy = max(x0 - i, 0, i - x1), max(y0 - j, 0, j - y1)
    if dx or dy:
        return max(dx, dy)
    return min(i - x0, x1 - i, j - y0, y1 - j)


def check_changed_world(view, laser, cw, labels, diff):
    """the three geometric statements, on anybody's labels (n_beams, 2) at tolerance 1 and diff of the one scan"""
    import map_changes_rule as rule
    from oracle import karto
    cells = diff["cells"]
    appeared = cells[cells[:, 2] == rule.APPEARED]
    assert len(appeared) > 0 and all(outline_distance(i, j, cw.pallet_cells) <= 1 for i, j, _ in appeared), "appeared cells off the pallet's outline"
    vanished = cells[cells[:, 2] == rule.VANISHED]
    x, y = view["anchor"][0] + vanished[:, 0] / view["scale"], view["anchor"][1] + vanished[:, 1] / view["scale"]
    x0, y0, x1, y1 = cw.footprint
    assert ((x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)).any(), "no vanished cell inside the deleted rack"
    want = np.zeros(laser.n_beams, dtype=bool)
    points = karto.scan_points(cw.ranges, cw.pose, laser)
    for i in np.nonzero(cw.on_pallet)[0]:
        kept, hit, end = ml.gate(cw.ranges[i], points[i], cw.pose, laser)
        if kept and hit:
            ex, ey = ml.lattice_cell(end[0], view["anchor"][0], view["scale"]), ml.lattice_cell(end[1], view["anchor"][1], view["scale"])
            want[i] = not rule.chebyshev_near(view, ex, ey, 1)
    assert want.any() and np.array_equal(labels[:, 0] == rule.NOVEL, want), "the NOVEL beams are not the pallet's"
