"""CPU: the rule of the map change layer (tests/map_changes_rule.py) against the occupancy oracle and against hand-made lanes.

  counters   for a window at the lattice origin the rule's pass / hits after observing k scans are oracle.karto.occupancy_from_scans'
             of those scans on the same lattice, and the patched cells its cell states wherever pass > min_pass_through
  labels     corridors of free cells, seven cells high, one beam each: every class, the tolerance, blocked
  decay      on odd counters
  bound      at 2^32 - 1 exactly, and one above it
"""
import math

import numpy as np
import pytest

import map_changes_cases as cc
import map_changes_rule as rule
import map_localize_cases as cases
import map_match_rule as mr
from common import LASER

U, O, F = cases.U, cases.O, cases.F
TOP = 2 ** 32 - 1


def test_counters_and_patched_cells_are_the_occupancy_oracle(oracle_lib):
    from oracle import karto
    sm, m = cases.small_map()
    blank = mr.view_dict(np.zeros_like(m.view["cells"]), m.offset, 1.0 / cases.RESOLUTION, 0, 0, m.width)
    scans = [karto.Scan(r, p, LASER) for r, p in zip(sm.ranges, sm.poses)]
    layer = rule.Layer(blank)
    for k in (3, 8):                                           # the first three scans, then all eight
        done = layer.scans
        layer.observe(LASER, np.array(sm.ranges[done:k]), sm.poses[done:k])
        for min_pass, threshold in ((2, 0.1), (0, 0.5), (5, 0.02)):
            cells, passes, hits = karto.occupancy_from_scans(m.width, m.height, m.offset, cases.RESOLUTION, scans[:k], LASER, min_pass, threshold)
            assert np.array_equal(layer.passes[:, :m.width], passes[:, :m.width]) and np.array_equal(layer.hits[:, :m.width], hits[:, :m.width])
            assert not layer.passes[:, m.width:].any() and not layer.hits[:, m.width:].any(), "the padding is no cell"
            d = layer.diff(min_pass, threshold)
            seen = passes[:, :m.width] > min_pass
            assert seen.any() and np.array_equal(d["patched"][:, :m.width][seen], cells[:, :m.width][seen])
            assert np.array_equal(d["patched"][:, :m.width][~seen], blank["cells"][:, :m.width][~seen])
            # on a map of unknown cells everything observed is discovered
            assert d["counts"][rule.UNOBSERVED] == (~seen).sum() and d["counts"][[rule.CONFIRMED, rule.APPEARED, rule.VANISHED]].sum() == 0
            assert d["counts"][rule.DISCOVERED_OCCUPIED] == (cells[:, :m.width] == O).sum() and len(d["cells"]) == seen.sum()
    assert layer.bound == 2 * LASER.n_beams * 8 and layer.scans == 8 and layer.beams == 8 * LASER.n_beams
    # the map those scans built, observed by them: nothing changed (what the library must reproduce on the GPU)
    same = rule.Layer(m.view)
    same.observe(LASER, np.array(sm.ranges), sm.poses)
    d = same.diff()
    assert len(d["cells"]) == 0 and d["counts"][rule.CONFIRMED] == (m.view["cells"][:, :m.width] != U).sum()
    assert np.array_equal(rule.nav_of(d["patched"], m.width), m.nav)


# ---------------------------------------------------------------- hand-made lanes
# 0.25 m cells; the sensor in column 4, beams along +x; row 1 ends in an unknown cell, row 3 in an occupied one, row 5 is free, row 7 holds
# an occupied cell in column 15
def lanes():
    cells = np.full((9, 24), F, dtype=np.uint8)
    cells[1, 20] = U
    cells[3, 20] = O
    cells[7, 15] = O
    return cases.view_of(cells, (0.0, 0.0), 4.0)


def label(row, r, t, **gates):
    laser = cases.circle(1, **gates)
    layer = rule.Layer(lanes())
    got = layer.observe(laser, [[r]], [(1.0, 0.25 * row, math.pi)], t)
    return tuple(int(v) for v in got[0, 0]), layer


def test_labels_on_hand_made_lanes(oracle_lib):
    (cls, blocked), layer = label(3, 4.0, 0)
    assert (cls, blocked) == (rule.EXPLAINED, 0), "a free corridor that ends in an occupied cell"
    assert layer.passes[3, 4:20].tolist() == [1] * 16 and layer.passes[3, 20] == 2 and layer.hits[3, 20] == 1 and layer.hits.sum() == 1
    assert label(3, 3.75, 0)[0] == (rule.NOVEL, 0), "the end one cell short of the obstacle, no tolerance"
    assert label(3, 3.75, 1)[0] == (rule.EXPLAINED, 0), "... and with one cell of tolerance"
    for t in (0, 1, 4):
        assert label(5, 1.0, t)[0] == (rule.NOVEL, 0), "the end in the middle of free space"
        assert label(7, 4.0, t)[0] == (rule.THROUGH, 1), "an occupied cell five cells before the end"
    assert label(1, 4.0, 0)[0] == (rule.UNKNOWN, 0), "the end on an unknown cell"
    (cls, blocked), layer = label(5, 4.0, 1, range_threshold=3.0)
    assert (cls, blocked) == (rule.CLEAR, 0) and layer.hits.sum() == 0 and layer.passes[5, 4:17].tolist() == [1] * 13, "a clipped beam"
    assert label(7, 4.0, 0, range_threshold=3.0)[0] == (rule.THROUGH, 1), "a clipped beam through an obstacle: through, hit or not"
    assert label(7, 4.0, 1, range_threshold=3.0)[0] == (rule.CLEAR, 0), "... which lies within the tolerance of the clipped end"
    (cls, blocked), layer = label(5, 6.0, 1, range_threshold=10.0, max_range=12.0)
    assert (cls, blocked) == (rule.UNKNOWN, 0) and layer.hits.sum() == 0 and layer.passes[5, 4:24].tolist() == [1] * 20, "the end outside the window"
    assert label(5, 0.05, 1)[0] == (rule.DROPPED, 0) and label(5, math.nan, 1)[0] == (rule.DROPPED, 0)
    # the obstacle two rows below the end cell counts as near from a tolerance of two cells on
    assert label(1, 4.0, 1)[0] == (rule.UNKNOWN, 0) and label(1, 4.0, 2)[0] == (rule.EXPLAINED, 0)
    # the tolerance takes from blocked what lies near the end: the beam of row 7, its end five cells to one cell past the obstacle
    assert [label(7, 4.0 - 0.25 * k, 2)[0] for k in range(5)] == [(rule.THROUGH, 1)] * 3 + [(rule.EXPLAINED, 0)] * 2


def test_decay_on_odd_counters():
    layer = rule.Layer(cases.view_of(np.full((2, 5), F, dtype=np.uint8), (0.0, 0.0), 4.0))
    layer.passes[0, :5] = [0, 1, 3, 7, TOP]
    layer.hits[1, :5] = [1, 2, 5, 9, TOP - 1]
    layer.bound = TOP
    layer.decay(1)
    assert layer.passes[0, :5].tolist() == [0, 0, 1, 3, 2 ** 31 - 1] and layer.hits[1, :5].tolist() == [0, 1, 2, 4, 2 ** 31 - 1]
    assert layer.bound == 2 ** 31 - 1 and layer.passes.dtype == np.uint32
    layer.decay(2)
    assert layer.passes[0, :5].tolist() == [0, 0, 0, 0, 2 ** 29 - 1] and layer.bound == 2 ** 29 - 1
    layer.decay(31)
    assert not layer.passes.any() and not layer.hits.any() and layer.bound == 0
    for shift in (0, 32, -1):
        with pytest.raises(rule.Refused):
            layer.decay(shift)


def test_overflow_bound_at_the_top_and_one_above(oracle_lib):
    assert rule.bound_after(TOP - 2, 1, 1) == TOP and rule.bound_after(TOP - 2 * 1081 * 3, 3, 1081) == TOP
    for bound, n_scans, n_beams in ((TOP - 1, 1, 1), (TOP - 2 * 1081 * 3 + 1, 3, 1081), (TOP, 1, 1), (0, 2 ** 31, 1)):
        with pytest.raises(rule.Refused):
            rule.bound_after(bound, n_scans, n_beams)
    laser = cases.circle(16)
    layer = rule.Layer(cases.view_of(np.full((41, 41), F, dtype=np.uint8), (0.0, 0.0), 4.0))
    layer.bound = TOP - 2 * 16
    layer.observe(laser, [np.full(16, 3.1)], [(5.0, 5.0, 0.0)])
    assert layer.bound == TOP and layer.hits.sum() == 16
    layer.bound = TOP - 2 * 16 + 1
    before = layer.passes.copy(), layer.hits.copy()
    with pytest.raises(rule.Refused):
        layer.observe(laser, [np.full(16, 3.1)], [(5.0, 5.0, 0.0)])
    assert np.array_equal(layer.passes, before[0]) and np.array_equal(layer.hits, before[1]) and layer.bound == TOP - 2 * 16 + 1 and layer.scans == 1


def test_diff_codes_and_thresholds():
    """every code, the strict comparisons, a map state that is none of the three"""
    cells = np.array([[F, F, O, O, U, U, U, 7, 7, F, F]], dtype=np.uint8)
    layer = rule.Layer(cases.view_of(cells, (0.0, 0.0), 4.0, ox=-3, oy=5))
    #                      confirmed appeared confirmed vanished disc.occ disc.free unobs  disc.free disc.occ  pass == min  ratio == threshold
    layer.passes[0, :11] = [10,      10,      10,       10,      10,      10,       0,     10,       10,       2,          8]
    layer.hits[0, :11] = [0,         5,       5,        0,       5,       0,        0,     0,        5,        2,          1]
    d = layer.diff(2, 0.125)
    assert d["codes"][0, :11].tolist() == [1, 2, 1, 3, 4, 5, 0, 5, 4, 0, 1]
    assert d["patched"][0].tolist() == [F, O, O, F, O, F, U, F, O, F, F] + [0] * 5, "the padding is zero"
    assert d["counts"].tolist() == [2, 3, 1, 1, 2, 2]
    assert d["cells"].tolist() == [[-2, 5, 2], [0, 5, 3], [1, 5, 4], [2, 5, 5], [4, 5, 5], [5, 5, 4]]
    d = layer.diff(1, math.nextafter(0.125, 0.0))
    assert d["codes"][0, 9:11].tolist() == [2, 2], "pass above min_pass_through; the ratio above the threshold"
    # an unobserved cell of state 7 stays 7 in the patched grid
    assert rule.Layer(layer.view).diff()["patched"][0, 7] == 7


UNIT_CASES = cc.unit_cases()


def test_unit_case_table_holds_every_count_and_both_shapes(oracle_lib):
    counts = [c.n_units for c in UNIT_CASES]
    assert set(counts) >= {1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 8193} and max(counts) == 32 * 1100 == 35200
    assert [cc.units_of(w, h) for w, h in cc.UNIT_SHAPES] == counts
    one = {c.n_units for c in UNIT_CASES if c.view["width"] == 1}
    assert one == {1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 8193}, "every count by the narrowest view that reaches it"
    assert {c.view["height"] for c in UNIT_CASES if c.view["width"] == 65} >= {512, 513, 1024, 2048, 2049}
    assert sum(c.view["ox"] < 0 and c.view["oy"] < 0 for c in UNIT_CASES) >= 2
    assert sum(c.view["cells"].shape[1] > c.view["width"] and (c.view["cells"][:, c.view["width"]:] == O).all() for c in UNIT_CASES) >= 2
    assert {c.name for c in UNIT_CASES} >= {cc.DECAY_CASE, cc.ROOM_CASE} and len({c.name for c in UNIT_CASES}) == len(UNIT_CASES)
    # the launches: ceil(n_units / 4) workgroups capped at 1024, per = ceil(n_units / 1024)
    trips = lambda n: -(-n // (4 * min(-(-n // 4), 1024)))      # noqa: E731
    assert cc.TRIP_UNITS == 4 * 1024 and [trips(n) for n in (4096, 4097, 8193, 35200)] == [1, 2, 3, 9]
    assert [-(-n // cc.SCAN_THREADS) for n in (1024, 1025, 2048, 2049, 35200)] == [1, 2, 2, 3, 35]
    assert cc.scan_range(512, 1025) == (1024, 1025) and cc.scan_range(513, 1025) == (1025, 1025), "per = 2: threads 513 and up are empty"
    # the largest hand-made view before this table
    assert cc.units_of(cc.wide_view()["width"], cc.wide_view()["height"]) == 9
    # ... and the end-to-end tests' small map, which lies past one trip but puts nothing on a threshold
    small = cases.small_map()[1]
    assert cc.units_of(small.width, small.height) == 4592 > cc.TRIP_UNITS


@pytest.mark.parametrize("case", UNIT_CASES, ids=[c.name for c in UNIT_CASES])
def test_unit_case_sits_on_its_edges(oracle_lib, case):
    """from the rule alone: the unit count of the name; a change in the first and in the last unit of every trip of k_map_changed and of
    three threads' ranges of k_map_changed_scan, the last non-empty thread among them; a quarter of the units with a change; varied
    counts; the caps where the case says they are"""
    view = case.view
    w, h, n_units = view["width"], view["height"], case.n_units
    per_row = -(-w // 64)
    assert case.name.startswith(f"{n_units} units") and n_units == per_row * h
    layer = rule.Layer(view)
    layer.observe(case.laser, case.ranges, case.poses)
    assert (layer.passes[:, :w] >= 1).all() and layer.hits.sum() == w, "every cell passed, one hit per column"
    d = layer.diff(case.min_pass, case.threshold)
    cells = d["cells"]
    unit = (cells[:, 1] - view["oy"]).astype(np.int64) * per_row + (cells[:, 0] - view["ox"]) // 64
    assert (np.diff(unit) >= 0).all(), "row-major: ascending units"
    counts = np.bincount(unit, minlength=n_units)
    assert np.array_equal(counts, cc.unit_counts(view, view["cells"] != F)), "the changed cells are those of another state than free"
    prefix = np.concatenate([[0], np.cumsum(counts)])
    for first in range(0, n_units, cc.TRIP_UNITS):
        assert counts[first] > 0 and counts[min(first + cc.TRIP_UNITS, n_units) - 1] > 0, f"trip {first // cc.TRIP_UNITS}"
    per = -(-n_units // cc.SCAN_THREADS)
    ranges = [cc.scan_range(t, n_units) for t in range(cc.SCAN_THREADS)]
    full = [t for t, (lo, hi) in enumerate(ranges) if hi > lo and counts[lo] > 0 and counts[hi - 1] > 0]
    last = max(t for t, (lo, hi) in enumerate(ranges) if hi > lo)
    assert len(full) >= 3 and last in full and last == (n_units - 1) // per
    assert (n_units > cc.SCAN_THREADS) == (per > 1) and (ranges[-1][0] == ranges[-1][1]) == (last < cc.SCAN_THREADS - 1)
    assert 4 * np.count_nonzero(counts) >= n_units
    values = set(counts.tolist())
    if w == 1:
        assert values == {0, 1}, "a unit of one cell"
    else:
        assert len(values) >= 3 and {0, 64} <= values and (1 in set(counts[1::per_row].tolist()) or w % 64 != 1)
    # the caps
    assert case.caps[:2] == (None, 0) and all(0 < c < len(cells) or n_units == cc.TRIP_UNITS + 1 for c in case.caps[2:])
    inside = case.caps[-1]
    u = int(np.searchsorted(prefix, inside, side="left")) - 1               # prefix[u] < inside <= prefix[u + 1]
    if n_units > cc.TRIP_UNITS:
        assert case.caps[2] == prefix[cc.TRIP_UNITS] and len(case.caps) == 4 and u >= cc.TRIP_UNITS
    else:
        assert len(case.caps) == 3
    assert prefix[u] < inside and (inside < prefix[u + 1] if w > 1 else inside == prefix[u + 1])


def test_changed_world_statements_hold_for_the_rule(oracle_lib):
    """tests/map_changes_cases.py's changed world with the rule alone: every appeared cell within one cell of the pallet's outline, a
    vanished cell inside the deleted rack, the NOVEL beams exactly the pallet's without an occupied map cell near their end, and the
    patched map the occupancy oracle's of the scan wherever it was observed"""
    import map_changes_cases as cc
    from oracle import karto
    sm, m = cases.small_map()
    cw = cc.changed_world()
    layer = rule.Layer(m.view)
    labels = layer.observe(LASER, [cw.ranges], [cw.pose], 1)[0]
    d = layer.diff()
    cc.check_changed_world(m.view, LASER, cw, labels, d)
    cells, passes, _ = karto.occupancy_from_scans(m.width, m.height, m.offset, cases.RESOLUTION, [karto.Scan(cw.ranges, cw.pose, LASER)], LASER)
    seen = passes[:, :m.width] > 2
    assert np.array_equal(d["patched"][:, :m.width][seen], cells[:, :m.width][seen])
    assert np.array_equal(d["patched"][:, :m.width][~seen], m.view["cells"][:, :m.width][~seen])
    assert d["counts"][rule.APPEARED] > 0 and d["counts"][rule.VANISHED] > 0 and (labels[:, 0] == rule.THROUGH).any()
