"""CPU: the rule of kh_map_raycast (tests/map_raycast_rule.py) against its own edge cases and against TraceLine.  Every case of
tests/map_raycast_cases.py sits on the edge its name says; the cells of every beam of every case are the cells of
tests/occupancy_cases.bresenham, ordered outward; on the small map the cast at the held-out pose is the scan taken there, within a
cell or two for most beams."""
import numpy as np
import pytest

import map_localize_cases as lc
import map_localize_rule as ml
import map_raycast_cases as cases
import map_raycast_rule as rule
import occupancy_cases as oc
from common import LASER

RAY_CASES = cases.ray_cases()


@pytest.mark.parametrize("case", RAY_CASES, ids=[c.name for c in RAY_CASES])
def test_case_sits_on_its_edge(oracle_lib, case):
    got = rule.cast_poses(case.view, case.laser, case.poses, case.max_unknown, case.no_return)
    assert got.codes.shape == (len(case.poses), case.laser.n_beams)
    no_return = rule.default_no_return(case.laser) if case.no_return is None else case.no_return
    miss = got.codes != rule.HIT
    assert np.array_equal(got.ranges[miss], np.full(int(miss.sum()), no_return), equal_nan=True)
    assert (got.ranges[~miss] >= 0).all() and (got.ranges[~miss] <= case.laser.range_threshold + 1.0 / case.view["scale"]).all()
    case.check(got)


@pytest.mark.parametrize("case", RAY_CASES, ids=[c.name for c in RAY_CASES])
def test_beam_cells_are_trace_line_outward(oracle_lib, case):
    v = case.view
    for pose in case.poses:
        c0 = (ml.lattice_cell(pose[0], v["anchor"][0], v["scale"]), ml.lattice_cell(pose[1], v["anchor"][1], v["scale"]))
        for p in rule.far_points(case.laser, pose):
            c1 = (ml.lattice_cell(p[0], v["anchor"][0], v["scale"]), ml.lattice_cell(p[1], v["anchor"][1], v["scale"]))
            x, y = rule.beam_cells(c0, c1)
            got = list(zip(x.tolist(), y.tolist()))
            want = oc.bresenham(c0[0], c0[1], c1[0], c1[1])
            assert sorted(got) == sorted(want) and len(got) == max(abs(c1[0] - c0[0]), abs(c1[1] - c0[1])) + 1
            assert got[0] == c0 and got[-1] == c1 and got in (want, want[::-1]), "TraceLine's own order, or its reverse"


def test_a_swapped_line_is_not_its_mirror_image():
    true, mirrored = cases.mirror_cells((25, 10), (13, 19))
    assert len(true) == len(mirrored) == 13 and true != mirrored
    same, _ = cases.mirror_cells((13, 19), (25, 10))
    assert same == true, "TraceLine visits the same cells from either end"


def test_default_no_return():
    assert rule.default_no_return(LASER) == np.nextafter(LASER.range_threshold, np.inf) > LASER.range_threshold
    tight = lc.CaseLaser(4, 0.0, 0.1, 0.1, 5.0, 5.0)
    assert np.isnan(rule.default_no_return(tight)), "no reading lies above range_threshold and below max_range"
    # what the gates make of it: dropped from the point readings (InRange is inclusive), kept and clipped by AddScan, no hit
    r = rule.default_no_return(LASER)
    assert not (LASER.min_range <= r <= LASER.range_threshold)
    kept, hit, _ = ml.gate(r, (1.0, 0.0), (0.0, 0.0, 0.0), LASER)
    assert kept and not hit


def test_refused():
    v = lc.view_of(np.full((4, 4), lc.F, dtype=np.uint8), (0.0, 0.0), 4.0)
    assert rule.cast_refused(v, lc.circle(4), (0.0, 0.0, 0.0), -2) and not rule.cast_refused(v, lc.circle(4), (0.0, 0.0, 0.0), -1)
    for pose in lc.REFUSED_POSES:
        assert rule.cast_refused(v, lc.circle(4), pose, 0)


def test_cast_at_the_held_out_pose_is_the_scan_taken_there(oracle_lib):
    sm, m = lc.small_map()
    for budget, want in cases.SMALL_MAP_COUNTS.items():
        got = rule.cast(m.view, LASER, sm.true_pose, budget)
        print(f"budget {budget}: FREE, HIT, UNKNOWN = {cases.counts(got.codes)}")
        assert cases.counts(got.codes) == want
    got = rule.cast(m.view, LASER, sm.true_pose, -1)
    both = (got.codes == rule.HIT) & (sm.query >= LASER.min_range) & (sm.query <= LASER.range_threshold)
    d = np.abs(got.ranges[both] - sm.query[both])
    print(f"{int(both.sum())} beams hit in both: |cast - scan| median {np.median(d):.3f} m, 90th percentile {np.percentile(d, 90):.3f} m, max {d.max():.2f} m")
    assert both.sum() > 850
    # a cell's half diagonal plus the scan's noise for the median; two cells for nine beams in ten
    assert np.median(d) <= 0.5 * np.sqrt(2.0) * lc.RESOLUTION + 0.03 and np.percentile(d, 90) <= 2 * lc.RESOLUTION
    fit = ml.fit(m.view, LASER, got.ranges, sm.true_pose)
    print(f"fit of the cast scan at its own pose: {fit['score']:.5f}, {fit['conflict']} conflicts")
    assert fit["score"] > 0.99
