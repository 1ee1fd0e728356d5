"""CPU: the rule of kh_map_visibility_* (tests/map_visibility_rule.py) against an independent restatement -- per beam the cells of
map_localize_rule.line_cells cut at the step kh_map_raycast's rule reports, gathered in python sets, with none of the rule's arrays --
on every case of tests/map_visibility_cases.py, and against values worked out by hand.  No GPU."""
import numpy as np
import pytest

import map_localize_cases as lc
import map_localize_rule as ml
import map_raycast_rule as rr
import map_visibility_cases as cases
import map_visibility_rule as rule
from map_localize_cases import F, O, U
from map_raycast_cases import row_case

VIS_CASES = cases.vis_cases()
SELECT_CASES = cases.select_cases()
BY_NAME = {c.name: c for c in VIS_CASES}


def restated_seen(view, laser, pose, budget):
    """-> (the set of seen window cells as lattice (i, j), the cells visited in all, the codes)"""
    cast = rr.cast(view, laser, pose, budget)
    ax, ay, scale = view["anchor"][0], view["anchor"][1], view["scale"]
    c0 = (ml.lattice_cell(pose[0], ax, scale), ml.lattice_cell(pose[1], ay, scale))
    cells, visited = set(), 0
    for b, p in enumerate(rr.far_points(laser, np.asarray(pose, dtype=np.float64))):
        c1 = (ml.lattice_cell(p[0], ax, scale), ml.lattice_cell(p[1], ay, scale))
        x, y = ml.line_cells(c0[0], c0[1], c1[0], c1[1])
        steep = abs(c1[1] - c0[1]) > abs(c1[0] - c0[0])
        for i, j in zip(x.tolist(), y.tolist()):
            if abs(j - c0[1] if steep else i - c0[0]) <= int(cast.steps[b]):
                visited += 1
                if ml.state_at(view, i, j) is not None:
                    cells.add((i, j))
    return cells, visited, cast.codes


def restated_record(view, cells, covered, codes, params):
    def by_state(group):
        states = [ml.state_at(view, i, j) for i, j in group]
        return sum(s == F for s in states), sum(s == O for s in states), sum(s not in (F, O) for s in states)
    seen, new = by_state(cells), by_state(cells - covered)
    p = dict(rule.PARAMS, **params)
    gain = p["w_unknown"] * new[2] + p["w_free"] * new[0] + p["w_occupied"] * new[1]
    return seen + new + (gain,) + tuple(int((codes == c).sum()) for c in (rr.FREE, rr.HIT, rr.UNKNOWN))


def mask_of(view, cells):
    out = np.zeros((view["height"], view["width"]), dtype=bool)
    for i, j in cells:
        out[j - view["oy"], i - view["ox"]] = True
    return out


@pytest.mark.parametrize("case", VIS_CASES, ids=[c.name for c in VIS_CASES])
def test_the_rule_equals_the_restatement(oracle_lib, case):
    """gain from a cleared mask, commit of every second pose, gain again: records and the mask"""
    vis = rule.Visibility(case.view, case.laser, **case.params)
    budget = vis.params["max_unknown"]
    sets = [restated_seen(case.view, case.laser, pose, budget) for pose in case.poses]
    covered = set()
    for step in range(2):
        got = vis.gain(case.poses)
        for k, (cells, _, codes) in enumerate(sets):
            assert tuple(int(got[k][f]) for f in rule.FIELDS) == restated_record(case.view, cells, covered, codes, case.params), (case.name, k, step)
        assert np.array_equal(vis.mask, mask_of(case.view, covered))
        vis.commit(case.poses[::2])
        for cells, _, _ in sets[::2]:
            covered |= cells
    vis.clear()
    assert not vis.mask.any()


def record_of(view, laser, pose, **params):
    return rule.Visibility(view, laser, **params).gain([pose])[0]


def test_a_single_beam_along_a_row_counts_each_cell_once(oracle_lib):
    view, laser, poses = row_case([F] * 20 + [O])
    r = record_of(view, laser, poses[0], max_unknown=-1)
    assert (r["seen_free"], r["seen_occupied"], r["seen_unknown"]) == (20, 1, 0), "s_end + 1 = 21 cells"
    assert (r["new_free"], r["new_occupied"], r["new_unknown"], r["gain"]) == (20, 1, 0, 0) and (r["beams_free"], r["beams_hit"], r["beams_unknown"]) == (0, 1, 0)
    r = record_of(view, laser, poses[0], max_unknown=-1, w_unknown=0, w_free=2, w_occupied=5)
    assert r["gain"] == 45
    # 64 beams along the same row would count the row 64 times as a per-beam sum: the set counts it once
    v2, l2, p2 = BY_NAME["all eight octants and both axis directions, inside a ring"][1:4]
    dense = lc.circle(512)
    one, many = record_of(v2, l2, p2[0], max_unknown=-1), record_of(v2, dense, p2[0], max_unknown=-1)
    assert many["seen_free"] <= 23 * 23 and many["seen_free"] > one["seen_free"], "no cell is counted twice however many beams cross it"


def test_two_identical_poses_committed_leave_nothing_new(oracle_lib):
    case = BY_NAME["65 beams, 2 poses, budget 2"]
    vis = rule.Visibility(case.view, case.laser, **case.params)
    before = vis.gain(case.poses[:1])[0]
    vis.commit([case.poses[0], case.poses[0]])
    after = vis.gain(case.poses[:1])[0]
    assert all(after[f] == 0 for f in ("new_free", "new_occupied", "new_unknown", "gain"))
    assert all(after[f] == before[f] for f in rule.FIELDS if f.startswith(("seen", "beams"))) and before["new_free"] == before["seen_free"] > 0


def test_sixteen_beams_inside_the_ring(oracle_lib):
    case = BY_NAME["all eight octants and both axis directions, inside a ring"]
    r = record_of(case.view, case.laser, case.poses[0], **case.params)
    assert r["seen_occupied"] == 16 and r["beams_hit"] == 16 and r["seen_unknown"] == 0


def test_one_unknown_cell_before_a_wall(oracle_lib):
    want = {-1: (4, 1, 1, (0, 1, 0)), 0: (2, 0, 1, (0, 0, 1)), 1: (4, 1, 1, (0, 1, 0))}      # free, occupied, unknown, beams: section 7m's table
    for budget, (n_free, n_occ, n_unk, beams) in want.items():
        case = BY_NAME[f"one unknown cell before a wall, budget {budget}"]
        r = record_of(case.view, case.laser, case.poses[0], **case.params)
        assert (r["seen_free"], r["seen_occupied"], r["seen_unknown"]) == (n_free, n_occ, n_unk), budget
        assert (r["beams_free"], r["beams_hit"], r["beams_unknown"]) == beams and r["gain"] == n_unk


def test_a_sensor_outside_the_window_and_one_far_off(oracle_lib):
    case = BY_NAME["a negative lattice origin, the sensor inside, beside each side and far off, budget -1"]
    got = rule.Visibility(case.view, case.laser, **case.params).gain(case.poses)
    for k in range(1, 5):
        cells, visited, _ = restated_seen(case.view, case.laser, case.poses[k], -1)
        n = int(got[k]["seen_free"]) + int(got[k]["seen_occupied"]) + int(got[k]["seen_unknown"])
        assert 0 < n == len(cells) < visited, "only the window cells among the visited ones are counted"
    far = got[5]
    assert all(far[f] == 0 for f in rule.FIELDS if not f.startswith("beams")) and (far["beams_free"], far["beams_hit"], far["beams_unknown"]) == (32, 0, 0)
    stopped = BY_NAME["a negative lattice origin, the sensor inside, beside each side and far off, budget 0"]
    got = rule.Visibility(stopped.view, stopped.laser, **stopped.params).gain(stopped.poses)
    assert all(got[k][f] == 0 for k in range(1, 6) for f in rule.FIELDS if not f.startswith("beams")) and (got["beams_unknown"][1:] == 32).all()


def test_nothing_of_the_padding_is_counted(oracle_lib):
    for fill in (O, F):
        case = BY_NAME[f"a width of 13, padding filled with {fill}"]
        got = rule.Visibility(case.view, case.laser, **case.params).gain(case.poses)
        assert (got["seen_occupied"] == 0).all() and (got["seen_unknown"] == 0).all() and (got["seen_free"] <= 13 * 9).all() and (got["seen_free"] > 13).all()
        assert case.view["cells"].shape[1] == 16 and (case.view["cells"][:, 13:] == fill).all()


def covered_by(vis, poses, picks):
    out = np.zeros_like(vis.mask)
    for k in picks:
        out |= vis.seen(poses[k])[0]
    return out


@pytest.mark.parametrize("case", SELECT_CASES, ids=[c.name for c in SELECT_CASES])
def test_select_cases(oracle_lib, case):
    vis = rule.Visibility(case.view, case.laser, **case.params)
    vis.commit(case.committed)
    before = vis.mask.copy()
    picks, gains = vis.select(case.poses, case.k, case.min_gain)
    assert len(picks) == len(set(picks.tolist())) <= case.k and (gains >= case.min_gain).all()
    assert np.array_equal(vis.mask, before | covered_by(vis, case.poses, picks)), "the mask is left holding the picks"
    # the restatement: each round by brute force over python sets
    budget = vis.params["max_unknown"]
    sets = [restated_seen(case.view, case.laser, pose, budget) for pose in case.poses]
    covered = set()
    for pose in case.committed:
        covered |= restated_seen(case.view, case.laser, pose, budget)[0]
    left, want = list(range(len(case.poses))), []
    for _ in range(case.k):
        g = {i: restated_record(case.view, sets[i][0], covered, sets[i][2], case.params)[6] for i in left}
        best = min(left, key=lambda i: (-g[i], i))
        if g[best] < case.min_gain:
            break
        want.append((best, g[best]))
        covered |= sets[best][0]
        left.remove(best)
    assert list(zip(picks.tolist(), gains.tolist())) == want
    if len(case.poses) >= 2:
        # k = 2 from a cleared mask: greedy's two picks cover at least what the two largest individual gains cover
        fresh = rule.Visibility(case.view, case.laser, **case.params)
        alone = fresh.gain(case.poses)["gain"].astype(np.int64)
        top = sorted(range(len(alone)), key=lambda i: (-alone[i], i))[:2]
        two, _ = fresh.select(case.poses, 2, 1)

        def weight(mask):
            cells = case.view["cells"][:, :case.view["width"]]
            p = fresh.params
            return int(p["w_occupied"] * (mask & (cells == O)).sum() + p["w_free"] * (mask & (cells == F)).sum() + p["w_unknown"] * (mask & (cells != O) & (cells != F)).sum())
        assert weight(covered_by(fresh, case.poses, two)) >= weight(covered_by(fresh, case.poses, top)), "the k = 2 invariant"


def test_an_early_stop_and_a_tie(oracle_lib):
    by = {c.name: c for c in SELECT_CASES}
    stop = by["an early stop: 5 candidates of 2 distinct poses, k 5"]
    vis = rule.Visibility(stop.view, stop.laser, **stop.params)
    picks, gains = vis.select(stop.poses, stop.k, stop.min_gain)
    assert len(picks) == 2 and sorted(picks.tolist()) == [0, 2], "the selection ends once both distinct poses are picked, each by its first copy"
    assert vis.gain(stop.poses)["gain"].max() == 0 < stop.min_gain
    tie = by["a tie between two identical candidates"]
    alone = rule.Visibility(tie.view, tie.laser, **tie.params).gain(tie.poses)["gain"]
    assert alone[0] == alone[2] and alone[1] == alone[3]
    picks, _ = rule.Visibility(tie.view, tie.laser, **tie.params).select(tie.poses, tie.k, tie.min_gain)
    assert picks[0] == (0 if alone[0] >= alone[1] else 1) and set(picks.tolist()) <= {0, 1}, "a tie goes to the smaller index; the twin adds nothing afterwards"


def test_refusals_and_the_reach():
    v = cases.vis_cases()[0].view
    assert rule.reach_of(cases.reach_laser(511), cases.K) == 511 and rule.reach_of(cases.reach_laser(363), cases.K) == 363
    assert rule.reach_of(lc.circle(4, range_threshold=0.2), cases.K) == 2, "the smallest reach there is"
    assert [rule.bitmap_bytes(r) for r in (0, 1, 361, 362, 363, 511)] == [4, 4, 65344, 65704, 66068, 130820]
    rule.Visibility(v, cases.reach_laser(511))
    for laser, params, why in ((cases.reach_laser(512), {}, "reach"), (lc.circle(16), dict(max_unknown=-2), "max_unknown"), (lc.circle(16), dict(w_unknown=0), "weights"),
                               (lc.circle(16), dict(w_free=256), "weights"), (lc.circle(16), dict(w_occupied=-1), "weights"), (lc.CaseLaser(0, -3.0, 0.1, 0.1, 7.5, 5.0), {}, "laser"),
                               (lc.circle(16, range_threshold=2.0 ** 20), {}, "laser"), (cases.reach_laser(512), dict(w_unknown=0, max_unknown=-2), "max_unknown")):
        with pytest.raises(rule.Refused) as e:
            rule.Visibility(v, laser, **params)
        assert str(e.value) == why
    for n, k, min_gain, why in ((0, 1, 1, "n"), (65537, 1, 1, "n"), (5, 0, 1, "k"), (5, 6, 1, "k"), (65536, 4097, 1, "k"), (5, 5, 0, "min_gain")):
        with pytest.raises(rule.Refused) as e:
            rule.select_check(n, k, min_gain)
        assert str(e.value) == why
    rule.select_check(65536, 4096, 1)


def test_the_small_map_sees_the_walls_its_beams_hit(oracle_lib):
    """for each of the eight poses, seen_occupied = the distinct HIT cells of the cast: an occupied cell is seen exactly where a beam ends on it"""
    from common import LASER
    sm, m = lc.small_map()
    vis = rule.Visibility(m.view, LASER, max_unknown=20)
    got = vis.gain(sm.poses)
    for k, pose in enumerate(np.asarray(sm.poses, dtype=np.float64)):
        cast = rr.cast(m.view, LASER, pose, 20)
        hits = {tuple(c) for c, code in zip(cast.cells.tolist(), cast.codes.tolist()) if code == rr.HIT}
        assert got[k]["seen_occupied"] == len(hits) > 0 and got[k]["beams_hit"] == int((cast.codes == rr.HIT).sum())
