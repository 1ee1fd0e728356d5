"""CPU: tests/map_footprint_rule.py against an independent restatement -- Python sets of the second Bresenham of the tests
(occupancy_cases.bresenham), filled per row, counted cell by cell -- and against hand values.  No GPU, nothing of the library."""
import math

import numpy as np
import pytest

import map_footprint_cases as cases
import map_footprint_rule as rule
import map_localize_cases as lc
import map_localize_rule as ml
from occupancy_cases import bresenham

POSE_CASES = cases.pose_cases()
LAYER_CASES = cases.layer_cases()


def covered_again(cells):
    """the covered set, once more: the outline as a set of cells, each row filled between its extreme outline cells"""
    outline = set()
    for k in range(len(cells)):
        outline |= set(bresenham(*cells[k], *cells[(k + 1) % len(cells)]))
    out = set()
    for j in range(min(c[1] for c in cells), max(c[1] for c in cells) + 1):
        row = [i for i, y in outline if y == j]
        assert row, "no row of the range is empty"
        out |= {(i, j) for i in range(min(row), max(row) + 1)}
    assert outline <= out
    return out


def record_again(view, d2, cells):
    if cells is None:
        return (rule.LATTICE, 0, 0, 0, 0, 0, rule.FAR, 0)
    n = dict(free=0, occupied=0, unknown=0, outside=0)
    least = rule.FAR
    for i, j in covered_again(cells):
        state = ml.state_at(view, i, j)
        n["outside" if state is None else "occupied" if state == 100 else "free" if state == 255 else "unknown"] += 1
        if state is not None:
            least = min(least, int(d2[j - view["oy"], i - view["ox"]]))
    status = rule.COLLISION if n["occupied"] else rule.OUTSIDE if n["outside"] else rule.UNKNOWN if n["unknown"] else rule.FREE
    return (status, sum(n.values()), n["free"], n["occupied"], n["unknown"], n["outside"], least, 0)


def test_the_rectangle_s_hand_values():
    view = lc.view_of(np.full((40, 60), lc.F, dtype=np.uint8), (0.0, 0.0), 20.0, -30, -20)
    d2 = np.full((40, 60), 7, dtype=np.uint32)
    counts = []
    for degrees in (0, 30, 45, 90):
        cells = rule.pose_cells(cases.RECTANGLE, (0.0, 0.0, math.radians(degrees)), (0.0, 0.0), 20.0)
        i, j = rule.covered(cells)
        assert set(zip(i.tolist(), j.tolist())) == covered_again(cells)
        counts.append(len(i))
    assert counts == [273, 269, 247, 273] and 273 == 13 * 21
    flat = rule.pose_cells(cases.RECTANGLE, (0.0, 0.0, 0.0), (0.0, 0.0), 20.0)
    assert sorted(flat) == [(-10, -6), (-10, 6), (10, -6), (10, 6)]
    # a wall one cell inside a corner of the 30-degree rectangle: COLLISION there, FREE at 0 degrees
    turned = rule.pose_cells(cases.RECTANGLE, (0.0, 0.0, math.radians(30)), (0.0, 0.0), 20.0)
    corner = turned[0]
    inside = (corner[0] - 1, corner[1] - 1)
    assert inside in covered_again(turned) and inside not in covered_again(flat)
    view["cells"][inside[1] + 20, inside[0] + 30] = lc.O
    records = rule.check(view, d2, cases.RECTANGLE, [(0.0, 0.0, 0.0), (0.0, 0.0, math.radians(30))])
    assert records["status"].tolist() == [rule.FREE, rule.COLLISION] and records["n_occupied"].tolist() == [0, 1]
    assert records["n_cells"].tolist() == [273, 269] and records["min_d2"].tolist() == [7, 7]


def test_the_single_cell_on_every_kind_of_cell():
    wants = {"free": (rule.FREE, 1, 1, 0, 0, 0), "occupied": (rule.COLLISION, 1, 0, 1, 0, 0), "unknown": (rule.UNKNOWN, 1, 0, 0, 1, 0), "of state 7": (rule.UNKNOWN, 1, 0, 0, 1, 0)}
    seen = 0
    for case in POSE_CASES:
        for name, want in wants.items():
            if case.name == f"1 x 1 {name}, the single cell on it and off it":
                got = rule.check(case.view, np.array([[5]], dtype=np.uint32), case.verts, case.poses)
                assert tuple(int(got[0][k]) for k in rule.FIELDS[:6]) == want and got[0]["min_d2"] == 5
                assert tuple(int(got[1][k]) for k in rule.FIELDS) == (rule.OUTSIDE, 1, 0, 0, 0, 1, rule.FAR, 0), "off the window"
                seen += 1
    assert seen == 4


@pytest.mark.parametrize("case", POSE_CASES, ids=[c.name for c in POSE_CASES])
def test_records_equal_the_restatement(case):
    d2 = cases.field_values(case)
    got = rule.check(case.view, d2, case.verts, case.poses)
    reach = rule.create_check(case.verts, case.view["scale"])
    for pose, r in zip(case.poses, got):
        cells = rule.pose_cells(case.verts, pose, case.view["anchor"], case.view["scale"])
        assert tuple(int(r[k]) for k in rule.FIELDS) == record_again(case.view, d2, cells), pose
        assert r["n_cells"] == r["n_free"] + r["n_occupied"] + r["n_unknown"] + r["n_outside"]
        own = (ml.lattice_cell(pose[0], case.view["anchor"][0], case.view["scale"]), ml.lattice_cell(pose[1], case.view["anchor"][1], case.view["scale"]))
        assert all(max(abs(c[0] - own[0]), abs(c[1] - own[1])) <= reach for c in cells), "the reach bounds every vertex cell"


def test_lattice_poses():
    view = cases.random_view(7, 5, 9, 4.0)
    got = rule.check(view, np.zeros((5, 9), dtype=np.uint32), cases.ONE_CELL, cases.lattice_poses(view))
    assert got["status"].tolist() == [rule.OUTSIDE, rule.LATTICE] * 4 + [rule.LATTICE] * 2
    for r in got[got["status"] == rule.LATTICE]:
        assert tuple(int(r[k]) for k in rule.FIELDS) == (rule.LATTICE, 0, 0, 0, 0, 0, rule.FAR, 0)
    with pytest.raises(rule.Refused):
        rule.check(view, np.zeros((5, 9), dtype=np.uint32), cases.ONE_CELL, [(0.0, math.nan, 0.0)])
    with pytest.raises(rule.Refused):
        rule.check(view, np.zeros((5, 9), dtype=np.uint32), cases.ONE_CELL, np.zeros((0, 3)))


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c.name for c in LAYER_CASES])
def test_the_layer_s_bit_is_the_pose_rule_at_the_offsets(case):
    view = case.view
    masks, summary = rule.layer(view, case.verts, case.n_headings, case.max_status)
    d2 = np.zeros((view["height"], view["width"]), dtype=np.uint32)
    h_, w_ = view["height"], view["width"]
    reach = rule.create_check(case.verts, view["scale"])
    win = view["cells"][:h_, :w_]
    codes = np.full((h_ + 2 * reach, w_ + 2 * reach), rule.OUTSIDE, dtype=np.int64)
    codes[reach:reach + h_, reach:reach + w_] = np.where(win == 100, rule.COLLISION, np.where(win == 255, rule.FREE, rule.UNKNOWN))
    rng = np.random.default_rng(1)
    for h in range(case.n_headings):
        offsets = rule.heading_offsets(case.verts, h, case.n_headings, view["scale"])
        stencil = covered_again(offsets)
        assert stencil == set(zip(*(v.tolist() for v in rule.covered(offsets))))
        # every cell: the worst code under the stencil's cells, one shifted copy of the window per stencil cell
        worst = np.zeros((h_, w_), dtype=np.int64)
        for di, dj in stencil:
            worst = np.maximum(worst, codes[reach + dj:reach + dj + h_, reach + di:reach + di + w_])
        assert np.array_equal(((masks >> np.uint32(h)) & 1).astype(bool), worst <= case.max_status), h
        # ... and rule.record_of itself at (i, j) + O_h, at some cells
        for i, j in zip(rng.integers(0, w_, 12).tolist(), rng.integers(0, h_, 12).tolist()):
            cells = [(view["ox"] + i + a, view["oy"] + j + b) for a, b in offsets]
            r = rule.record_of(view, d2, cells)
            assert int(r["status"]) == worst[j, i] and (int(r["status"]) <= case.max_status) == bool((int(masks[j, i]) >> h) & 1), (h, i, j)
    full = (1 << case.n_headings) - 1
    assert summary["n_any"] == int((masks != 0).sum()) and summary["n_all"] == int((masks == full).sum())
    assert [int(v) for v in summary["n_fit"]] == [int(((masks >> np.uint32(h)) & 1).sum()) for h in range(case.n_headings)]
    assert int(masks.max()) <= full


def test_an_all_free_window_fits_nowhere_near_its_edge_and_everywhere_with_max_status_2():
    by_name = {c.name: c for c in LAYER_CASES}
    m0, s0 = rule.layer(*(by_name["70 x 20 all free, H 7, max_status 0"][k] for k in (1, 2, 3, 4)))
    m2, s2 = rule.layer(*(by_name["70 x 20 all free, H 7, max_status 2"][k] for k in (1, 2, 3, 4)))
    assert s2["n_all"] == 70 * 20 and np.all(m2 == 127)
    assert m0[0, 0] == 0 and m0[10, 35] & 1 and 0 < s0["n_any"] < 70 * 20
    mu, su = rule.layer(*(by_name["70 x 20 all unknown, H 7, max_status 0"][k] for k in (1, 2, 3, 4)))
    assert su["n_any"] == 0
    m1, s1 = rule.layer(*(by_name["70 x 20 all unknown, H 7, max_status 1"][k] for k in (1, 2, 3, 4)))
    assert np.array_equal(m1, m0), "unknown cells allowed: an all-unknown window is an all-free one"


def test_path_poses_repeat_the_last_heading():
    xy = [(0.0, 0.0), (1.0, 0.0), (1.0, 2.0), (0.0, 2.0)]
    poses = rule.path_poses(xy)
    assert poses[:, 2].tolist() == [0.0, math.pi / 2, math.pi, math.pi] and np.array_equal(poses[:, :2], np.array(xy))
    assert rule.path_poses([(3.0, 4.0)]).tolist() == [[3.0, 4.0, 0.0]]
    from slam_toolbox_amd.map_footprint import MapFootprint
    assert np.array_equal(MapFootprint.path_poses(xy), poses)
