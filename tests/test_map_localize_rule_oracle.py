"""CPU: the rule of the map localizer (tests/map_localize_rule.py) against the oracle and against its own edge cases.  Every case of
tests/map_localize_cases.py sits on the edge its name says; on a view whose window starts at the lattice origin the rule's fit is
oracle.karto.occupancy_from_scans of the one scan masked by state; on the small map the rule finds the held-out pose."""
import math

import numpy as np
import pytest

import map_localize_cases as cases
import map_localize_rule as rule
import merge_fit_rule as fr
import relocalize_cases as rc
from common import LASER, OFFLINE_PARAMS

SEED_CASES, FIT_CASES = cases.seed_cases(), cases.fit_cases()


@pytest.mark.parametrize("case", SEED_CASES, ids=[c.name for c in SEED_CASES])
def test_seed_case_sits_on_its_edge(case):
    cells, xy = rule.seeds(case.view, case.spacing, case.center, case.radius)
    assert cells.shape == xy.shape and cells.shape[1] == 2
    v = case.view
    for (i, j), (x, y) in zip(cells, xy):
        assert rule.state_at(v, int(i), int(j)) == cases.F, "a seed is a free cell of the window"
        assert (x, y) == (v["anchor"][0] + float(i) / v["scale"], v["anchor"][1] + float(j) / v["scale"])
        assert (rule.lattice_cell(x, v["anchor"][0], v["scale"]), rule.lattice_cell(y, v["anchor"][1], v["scale"])) == (i, j)
    case.check(cells, xy)


def test_seed_rule_by_brute_force():
    """the vectorised rule against the sentence it states, cell by cell"""
    case = next(c for c in SEED_CASES if c.name.startswith("negative origin"))
    v, p = case.view, rule.pitch_of(case.spacing, case.view["scale"])
    best = {}
    for wy in range(v["height"]):
        for wx in range(v["width"]):
            if v["cells"][wy, wx] != cases.F:
                continue
            i, j = wx + v["ox"], wy + v["oy"]
            bx, by = i // p, j // p
            key = ((2 * i - (2 * bx * p + p - 1)) ** 2 + (2 * j - (2 * by * p + p - 1)) ** 2, j, i)
            if (by, bx) not in best or key < best[by, bx]:
                best[by, bx] = key
    want = [[best[b][2], best[b][1]] for b in sorted(best)]
    assert rule.seeds(v, case.spacing)[0].tolist() == want


def test_pitch_rule():
    assert [rule.pitch_of(s, 20.0) for s in (1.0, 1.5, 1.55, 2.0, 0.001)] == [21, 31, 31, 41, 1]
    for bad in (0.0, -1.0, math.inf, math.nan, 4096.5 / 20.0):
        with pytest.raises(ValueError):
            rule.pitch_of(bad, 20.0)
    assert rule.pitch_of(4095.4 / 20.0, 20.0) == 4095


@pytest.mark.parametrize("case", FIT_CASES, ids=[c.name for c in FIT_CASES])
def test_fit_case_sits_on_its_edge(case):
    fits = [rule.fit(case.view, case.laser, case.ranges, pose) for pose in case.poses]
    for f in fits:
        assert f["known"] == f["agree"] + f["conflict"] and 0.0 <= f["score"] <= 1.0
    case.check(fits)


def test_line_cells_is_trace_line():
    """the rule's closed form of TraceLine against the step-by-step restatement of tests/occupancy_cases.py"""
    import occupancy_cases as oc
    rng = np.random.default_rng(9)
    lines = [(0, 0, 0, 0), (3, -2, 3, 9), (3, 9, 3, -2), (-5, 4, 6, 4), (6, 4, -5, 4), (0, 0, 7, 7), (7, 7, 0, 0), (0, 0, 7, -7), (0, 0, 2, 1), (0, 0, 1, 2),
             (0, 0, 4, 2), (0, 0, 2, 4), (0, 0, -4, 2), (0, 0, 2, -4), (-3, -3, 4, -2), (-3, -3, -2, 4)]
    lines += [tuple(int(v) for v in rng.integers(-60, 60, size=4)) for _ in range(400)]
    for line in lines:
        x, y = rule.line_cells(*line)
        assert list(zip(x.tolist(), y.tolist())) == oc.bresenham(*line), line


def test_refused_poses():
    v = cases.view_of(np.full((4, 4), cases.F, dtype=np.uint8), (0.0, 0.0), 4.0)
    for pose in cases.REFUSED_POSES:
        assert rule.fit_refused(v, cases.circle(4), pose)
    assert not rule.fit_refused(v, cases.circle(4), (2.0 ** 30 / 4.0, 0.0, 0.0))
    assert rule.fit_refused(v, cases.circle(4, range_threshold=(2 ** 20 - 1) / 4.0, max_range=1e9), (0.0, 0.0, 0.0))


def test_fit_is_the_occupancy_oracle_masked_by_state():
    from oracle import karto
    sm, m = cases.small_map()
    for pose in (sm.true_pose, sm.true_pose + np.array([0.35, -0.2, 0.4]), np.array([m.offset[0] - 2.0, m.offset[1] + 3.0, 0.2])):
        scan = karto.Scan(sm.query, pose, LASER)
        _, p, h = karto.occupancy_from_scans(m.width, m.height, m.offset, cases.RESOLUTION, [scan], LASER)
        cells = m.view["cells"]
        p, h = p.copy(), h.copy()
        p[:, m.width:] = 0                                    # (the oracle's grid has no padding cells either)
        h[:, m.width:] = 0
        want = fr.derive(fr.count(cells, p, h))
        got = rule.fit(m.view, LASER, sm.query, pose)
        assert got == want and got["known"] > 0


def test_small_map_is_found():
    sm, m = cases.small_map()
    occupied, free = int((m.nav == 100).sum()), int((m.nav == 0).sum())
    print(f"small map {m.width} x {m.height}, {occupied} occupied, {free} free")
    assert occupied > 500 and free > 20000
    res = cases.rule_on_small_map()
    assert rule.pitch_of(cases.PITCH * cases.RESOLUTION, 1.0 / cases.RESOLUTION) == cases.PITCH
    n_passed = sum(h.passed for h in res.hyps)
    print(f"{len(res.cells)} seeds, {len(res.hyps)} hypotheses, {n_passed} passed, {len(res.accepted)} accepted, {len(res.duplicates)} duplicates, "
          f"{len(res.kept)} kept")
    assert len(res.accepted) >= 1 and res.kept[0] == res.accepted[0]
    best = res.hyps[res.kept[0]]
    d = math.hypot(best.fine_mean[0] - sm.true_pose[0], best.fine_mean[1] - sm.true_pose[1])
    dh = abs(rule.normalize_angle(best.fine_mean[2] - sm.true_pose[2]))
    f = res.fits[res.kept[0]]
    print(f"best: fine response {best.fine_response:.4f}, {d:.4f} m and {dh:.5f} rad from the truth, fit agree {f['agree']} conflict {f['conflict']} "
          f"score {f['score']:.5f}")
    # half a map-cell diagonal plus one fine step; the fine angle search's half width
    assert d <= 0.5 * math.sqrt(2.0) * cases.RESOLUTION + 0.01 and dh <= OFFLINE_PARAMS["fine_search_angle_offset"]
    truth = rule.fit(m.view, LASER, sm.query, sm.true_pose)
    print(f"fit at the true pose: agree {truth['agree']} conflict {truth['conflict']} score {truth['score']:.5f}")
    assert truth["score"] > 0.95


def test_even_pitch_is_made_odd():
    """30 cells asked for are 31: the same seeds, hence the same answer -- the odd pitch is the rule, not luck"""
    sm, m = cases.small_map()
    scale = 1.0 / cases.RESOLUTION
    assert rule.pitch_of(30 * cases.RESOLUTION, scale) == 31 == rule.pitch_of(31 * cases.RESOLUTION, scale)
    center = (sm.true_pose[0] + cases.CENTER_OFFSET[0], sm.true_pose[1] + cases.CENTER_OFFSET[1])
    a = rule.seeds(m.view, 30 * cases.RESOLUTION, center, cases.RADIUS)
    b = rule.seeds(m.view, 31 * cases.RESOLUTION, center, cases.RADIUS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) >= 4
    # neighbouring seeds alternate lattice phase: the coarse search steps by two cells
    assert len({(int(i) % 2, int(j) % 2) for i, j in a[0]}) > 1
