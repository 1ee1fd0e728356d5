"""CPU: the rule of the distance field (tests/map_field_rule.py) against itself and against hand-checked values -- the two ways of
computing d2 agree on every case of tests/map_field_cases.py and with scipy's Euclidean transform where scipy is installed; every
case sits on the edge its name says; the cost table's four branches; the score with its beams as arrays equals the score beam by
beam; the refinement on the small map recovers a displaced pose.  No library, no GPU."""
import math

import numpy as np
import pytest

import map_field_cases as cases
import map_field_rule as rule
import map_localize_cases as lc
from common import LASER

FIELD_CASES = cases.field_cases()


def test_brute_force_equals_the_separable_form_on_every_case():
    for c in FIELD_CASES:
        brute, separable = rule.d2_brute(c.view, c.radius, c.obstacles), rule.d2_separable(c.view, c.radius, c.obstacles)
        assert brute.dtype == np.uint32 and brute.shape == (c.view["height"], c.view["width"])
        assert np.array_equal(brute, separable), c.name
        c.check(brute)
    names = [c.name for c in FIELD_CASES]
    assert len(set(names)) == len(names)


def test_both_equal_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for c in FIELD_CASES:
        mask = rule.obstacle_mask(c.view, c.obstacles)
        want = rule.d2_separable(c.view, 0, c.obstacles)
        if mask.any():
            edt = np.rint(ndimage.distance_transform_edt(~mask) ** 2).astype(np.int64)
            assert np.array_equal(want.astype(np.int64), edt), c.name
            assert np.array_equal(rule.d2_separable(c.view, c.radius, c.obstacles), rule.capped(edt, c.radius)), c.name
        else:
            assert (want == rule.FAR).all(), c.name


def one(cells, r, obstacles=rule.OCCUPIED):
    return rule.d2_brute(lc.view_of(np.asarray(cells, dtype=np.uint8), cases.A, cases.K), r, obstacles)


def test_hand_checked_fields():
    cells = np.full((8, 8), 255, dtype=np.uint8)
    cells[0, 0] = 100
    d2 = one(cells, 5)
    assert d2[3, 4] == d2[4, 3] == 25, "the 3-4-5 triangle lies exactly on the radius and is kept"
    assert d2[1, 5] == d2[5, 1] == rule.FAR and one(cells, 0)[1, 5] == 26, "its neighbour at d2 = 26 is not"
    assert d2[0, 0] == 0 and d2[0, 5] == 25 and d2[0, 6] == rule.FAR
    j, i = np.mgrid[0:8, 0:8]
    assert np.array_equal(one(cells, 0), (i * i + j * j).astype(np.uint32)), "a single obstacle: the squared distance to it"
    free = np.full((5, 9), 255, dtype=np.uint8)
    assert (one(free, 0) == rule.FAR).all() and (one(free, 3) == rule.FAR).all(), "no obstacle at all"
    assert rule.stats(one(free, 0)) == dict(n_obstacles=0, n_far=45, max_d2=0)
    assert rule.stats(d2) == dict(n_obstacles=1, n_far=int((i * i + j * j > 25).sum()), max_d2=25)
    m = rule.metres(d2, 4.0)
    assert m[3, 4] == 5.0 / 4.0 and m[1, 5] == math.inf and m[0, 0] == 0.0 and m[1, 1] == math.sqrt(2.0) / 4.0


def test_hand_checked_cost_table():
    t = rule.cost_table(4.0, inscribed_radius=0.5, inflation_radius=1.0, cost_scaling_factor=2.0)     # 2 and 4 cells
    assert t.size == 17
    assert t[0] == 254, "the obstacle itself"
    assert t[1] == t[2] == t[4] == 253, "within the inscribed radius, its edge included"
    assert t[5] == int(252.0 * math.exp(-2.0 * (math.sqrt(5.0) / 4.0 - 0.5))) == 223
    assert t[16] == int(252.0 * math.exp(-2.0 * 0.5)) == 92, "the edge of the inflation radius still decays"
    view = lc.view_of(np.array([[100, 255, 255, 255, 255, 255, 0, 0]], dtype=np.uint8), cases.A, 4.0)
    d2 = rule.d2_brute(view, 0)
    assert d2.tolist() == [[0, 1, 4, 9, 16, 25, 36, 49]]
    kw = dict(inscribed_radius=0.5, inflation_radius=1.0, cost_scaling_factor=2.0)
    assert rule.costs(view, d2, 0, track_unknown=0, **kw).tolist() == [[254, 253, 253, int(t[9]), 92, 0, 0, 0]], "beyond the radius: 0"
    assert rule.costs(view, d2, 0, track_unknown=1, **kw).tolist() == [[254, 253, 253, int(t[9]), 92, 0, 255, 255]]
    near = lc.view_of(np.array([[100, 0, 0, 0, 0, 0]], dtype=np.uint8), cases.A, 4.0)
    n2 = rule.d2_brute(near, 0)
    assert rule.costs(near, n2, 0, track_unknown=1, inflate_unknown=0, **kw).tolist() == [[254, 253, 253, 255, 255, 255]], "lethal and inscribed costs win over unknown"
    assert rule.costs(near, n2, 0, track_unknown=1, inflate_unknown=1, **kw).tolist() == [[254, 253, 253, int(t[9]), 92, 255]]
    assert rule.costs(near, n2, 0, track_unknown=0, inflate_unknown=1, **kw).tolist() == [[254, 253, 253, int(t[9]), 92, 0]]
    with pytest.raises(rule.Refused):
        rule.costs(near, rule.d2_brute(near, 3), 3, **kw)      # a field of 3 cells does not reach 4


def test_clearance_codes():
    c = next(c for c in FIELD_CASES if c.name == "40 x 50 random, p_occ 0.02, seed 1, R 4")
    d2 = rule.d2_brute(c.view, c.radius)
    m, status, v = rule.clearance(c.view, d2, cases.clearance_points(c.view, d2))
    assert set(status.tolist()) == {rule.OK, rule.CLEAR_FAR, rule.OUTSIDE}
    assert (status[-9:] == rule.OUTSIDE).all() and np.isinf(m[status != rule.OK]).all() and (v[status != rule.OK] == rule.FAR).all()
    assert status[0] != rule.OUTSIDE and status[1] != rule.OUTSIDE, "the window's first and last cell"
    ok = status == rule.OK
    assert np.array_equal(m[ok], np.sqrt(v[ok].astype(np.float64)) / c.view["scale"])
    # half-way between cells 0 and 1 is cell 1, half-way between 0 and -1 is cell -1: away from zero
    ax, k = c.view["anchor"][0], c.view["scale"]
    assert rule.ml.lattice_cell(ax + 0.5 / k, ax, k) == 1 and rule.ml.lattice_cell(ax - 0.5 / k, ax, k) == -1


def test_score_by_beam_equals_score_by_arrays(oracle_lib):
    for case in lc.fit_cases():
        r = 6
        d2 = rule.d2_separable(case.view, r)
        for pose in case.poses:
            for t in (0, 3):
                assert rule.score(case.view, d2, r, case.laser, case.ranges, pose, t) == rule.score_arrays(case.view, d2, r, case.laser, case.ranges, pose, t), case.name
    with pytest.raises(rule.Refused):
        rule.score(case.view, d2, 0, case.laser, case.ranges, case.poses[0], 0)
    for pose in lc.REFUSED_POSES:
        with pytest.raises(rule.Refused):
            rule.score_arrays(case.view, d2, r, case.laser, case.ranges, pose)


def test_refinement_on_the_small_map(oracle_lib):
    """poses displaced by a few cells and a hundredth of a radian descend to a minimum of the compass.  (The query scan sees walls the
    eight mapped scans did not: their ends cost T^2 wherever the scan stands, and the minimum need not lie at the true pose.)"""
    sm, m = lc.small_map()
    r = 40
    d2 = rule.d2_separable(m.view, r)
    truth = np.asarray(sm.true_pose, dtype=np.float64)
    at_truth = rule.score_arrays(m.view, d2, r, LASER, sm.query, truth)
    starts = [truth + [0.12, -0.08, 0.015], truth, truth + [-0.2, 0.15, -0.03]]
    out = rule.refine(m.view, d2, r, LASER, sm.query, starts)
    for start, res in zip(starts, out):
        print(f"start offset {np.round(start - truth, 3)}: cost {res.cost_start} -> {res.cost} in {res.rounds} rounds, {res.halvings} halvings, "
              f"status {res.status}, end offset {np.round(res.pose - truth, 4)}; cost at the true pose {at_truth['cost']}")
        assert res.status == rule.CONVERGED and res.halvings == 4 and res.cost <= res.cost_start and res.n_hit == at_truth["n_hit"]
        assert res.cost_start == rule.score(m.view, d2, r, LASER, sm.query, start)["cost"]
    # a converged start is a minimum of the compass at the last steps: beam by beam, none of its 27 neighbours scores lower
    s, a = 2.0 / m.view["scale"] / 16, 0.02 / 16
    around = [rule.score(m.view, d2, r, LASER, sm.query, rule.candidate(tuple(out[0].pose), s, a, c))["cost"] for c in range(27)]
    assert min(around) == around[13] == out[0].cost
    assert out[1].cost <= at_truth["cost"] == out[1].cost_start, "from the true pose the search only descends"
    assert out[0].cost < out[0].cost_start and out[2].cost < out[2].cost_start, "the integer cost has a slope where the counters of the fit are flat"
    # truncated at 6 cells an end that the map does not explain costs little, and the minimum lies within a cell (and within the first
    # heading step) of the pose the scan was taken at
    for res in rule.refine(m.view, d2, r, LASER, sm.query, starts, truncate_cells=6):
        print(f"truncated at 6 cells: cost {res.cost_start} -> {res.cost} in {res.rounds} rounds, end offset {np.round(res.pose - truth, 4)}")
        assert res.status == rule.CONVERGED and np.abs(res.pose[:2] - truth[:2]).max() < 1.0 / m.view["scale"] and abs(res.pose[2] - truth[2]) < 0.02
    two = rule.refine(m.view, d2, r, LASER, sm.query, starts[:1], max_rounds=2)[0]
    assert two.status == rule.MAX_ROUNDS and two.rounds == 2
