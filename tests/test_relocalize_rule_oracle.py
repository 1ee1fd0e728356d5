"""CPU: the relocalization rule (tests/relocalize_rule.py) pinned on its own -- the seed lattice, the bases
and their stride rule at their edges, the case table of tests/relocalize_cases.py, and one end-to-end run on the small map with
oracle.karto.Matcher.  Nothing of the library is read."""
import math

import numpy as np
import pytest

import relocalize_cases as rc
import relocalize_rule as rr

CASES = rc.cases()


def test_every_vertex_shares_a_cell_with_exactly_one_seed_and_seeds_are_cell_minima():
    for case in CASES:
        if case.poses.shape[0] == 0:
            continue
        s = rr.seeds(case.poses, case.spacing)                   # (no region: the cover itself)
        assert (np.diff(s) > 0).all()
        c = rr.cells(case.poses, case.spacing)
        same = (c[:, None, 0] == c[None, s, 0]) & (c[:, None, 1] == c[None, s, 1])           # vertex x seed
        assert (same.sum(axis=1) == 1).all(), case.name
        owner = s[same.argmax(axis=1)]
        assert (owner <= np.arange(case.poses.shape[0])).all(), case.name                     # no vertex before its cell's seed
        assert np.array_equal(owner[s], s), case.name


def test_cells_are_the_floor_of_the_fp64_quotient():
    sp = 1.5
    below = math.nextafter
    pts = [(-0.0, 0.0), (0.0, -0.0), (3 * sp, -3 * sp), (below(3 * sp, 0.0), below(-3 * sp, -math.inf)), (-0.2, -1.5), (-1.6, 4.49999)]
    assert rr.cells(pts, sp).tolist() == [[-0.0, 0.0], [0.0, -0.0], [3.0, -3.0], [2.0, -4.0], [-1.0, -1.0], [-2.0, 2.0]]
    assert rr.seeds([(-0.0, 0.0), (0.0, -0.0), (0.1, 0.1), (-0.1, 0.1)], sp).tolist() == [0, 3]            # the zeros are one cell
    # not towards zero: -0.2 and +0.2 are different cells
    assert rr.seeds([(0.2, 0.2), (-0.2, 0.2), (-0.2, -0.2), (0.2, -0.2)], sp).tolist() == [0, 1, 2, 3]


def test_bases_are_ascending_and_respect_the_range_at_the_tolerance():
    lo, hi = rc.edge_of(rc.MAX_D * rc.MAX_D + rr.KT_TOLERANCE)
    lo_minus, hi_minus = rc.edge_of(rc.MAX_D * rc.MAX_D - rr.KT_TOLERANCE)
    assert hi_minus < rc.MAX_D < lo                                  # the range reaches PAST max_distance by the tolerance
    poses = [(0.0, 0.0), (hi, 0.0), (lo, 0.0), (0.0, -hi_minus), (0.0, -rc.MAX_D), (100.0, 0.0)]
    assert rr.base(poses, 0, rc.MAX_D, 40).tolist() == [0, 2, 3, 4]
    for case in CASES:
        s, begin, idx = rr.candidates(case.poses, case.spacing, case.max_distance, case.max_base, case.center, case.radius)
        for k in range(s.size):
            b = idx[begin[k]:begin[k + 1]]
            assert (np.diff(b) > 0).all() and 1 <= b.size <= case.max_base, case.name
            assert (rr.dist_sq(case.poses[b], case.poses[s[k]]) < case.max_distance ** 2 + rr.KT_TOLERANCE).all(), case.name


@pytest.mark.parametrize("count,kept", [(5, [0, 1, 2, 3, 4]), (6, [0, 2, 4]), (10, [0, 2, 4, 6, 8]), (11, [0, 3, 6, 9])])
def test_stride_rule(count, kept):
    """max_base 5: all of c = 5; of 6 and of 2 * 5 every second; of 2 * 5 + 1 every third"""
    poses = np.stack([0.01 * np.arange(count), np.zeros(count)], axis=1)
    assert rr.base(poses, 0, rc.MAX_D, 5).tolist() == kept


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_sits_on_its_edge(case):
    case.check(*rr.candidates(case.poses, case.spacing, case.max_distance, case.max_base, case.center, case.radius))


def test_headings():
    assert rr.default_n_headings(0.349) == 10                          # nine windows of +-0.349 rad fall short of a turn
    assert 9 * 2 * 0.349 < 2 * math.pi < 10 * 2 * 0.349
    h = rr.headings(10)
    assert h[0] == -math.pi and h[5] == -math.pi + 5 * (2 * math.pi / 10) and h.size == 10 and (np.diff(h) > 0).all() and h[-1] < math.pi


def test_the_rule_alone_finds_the_held_out_pose():
    """The small map (tests/relocalize_cases.py): 8 scans of an aisle, the query taken at the held-out node's position with the robot
    turned 0.885 rad from the heading of every scan of the map.  24 hypotheses (3 seeds x 8 headings), oracle matchers, loop search space
    4 m at 5 cm.  Seeds tried: world / scan noise (12345, 1), (12345, 2), (7, 1); all three satisfy the test, (12345, 2) is used.

    Measured with the rule alone (this test prints it): 6 hypotheses pass the coarse gate, 5 are accepted; the best is hypothesis 23
    (seed = list index 5, the cell next to the held-out pose's, heading 7), fine response 0.8207; its robot pose lies
    RECORDED_DISTANCE = 0.0 m from the true position (x and y are met to the last bit: both lie on the fine search's centimetre
    lattice) and 0.00121 rad from the true heading.  The assertion is that distance plus one fine cell."""
    sm = rc.small_map()
    r = rc.rule_on_small_map()
    assert len(r.hyps) == 24 and r.seeds.tolist() == [0, 3, 5]
    heading_gap = np.abs((sm.true_pose[2] - sm.poses[:, 2] + math.pi) % (2 * math.pi) - math.pi)
    assert (heading_gap > 2 * 0.349).all()                             # more than one coarse window from every scan of the map
    assert sum(h.passed for h in r.hyps) > len(r.ranking) >= 2          # the gate and the acceptance are told apart
    best = r.hyps[r.ranking[0]]
    seed_cell = rr.cells(sm.poses[best.seed, :2], rc.SPACING)[0]
    true_cell = rr.cells(sm.true_pose[:2], rc.SPACING)[0]
    assert np.abs(seed_cell - true_cell).max() <= 1
    robot = rr.robot_at(best.fine_mean)
    distance = math.hypot(robot[0] - sm.true_pose[0], robot[1] - sm.true_pose[1])
    print(f"best {best.index} seed {best.seed} fine {best.fine_response!r} coarse {best.coarse_response!r} distance {distance!r} "
          f"heading error {abs(robot[2] - sm.true_pose[2])!r} passed {sum(h.passed for h in r.hyps)} accepted {len(r.ranking)}")
    assert distance <= RECORDED_DISTANCE + FINE_CELL
    assert abs(robot[2] - sm.true_pose[2]) < 0.349
    # the ranking is by fine response, then coarse response, then index
    keys = [(-r.hyps[i].fine_response, -r.hyps[i].coarse_response, i) for i in r.ranking]
    assert keys == sorted(keys)


RECORDED_DISTANCE = 0.0            # metres, measured by the test above with the rule alone
FINE_CELL = 0.01                   # correlation_search_space_resolution: the quantum of the fine search
