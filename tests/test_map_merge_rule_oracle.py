"""CPU: the rule of the map merge (tests/map_merge_rule.py) pinned on its own -- an identity warp reproduces the moving map, the table
of all nine (T, M) combinations under each policy, every case of tests/map_merge_cases.py on the edge its name says -- and on the real
pair of tests/map_align_cases.py: merged under the true correction it agrees better, with itself and with the map built from all
eight scans, than under each of three perturbed corrections, and it knows cells the target lacks.

Measured with this rule (footprint 1, grow 1, policy OCCUPIED):

                                  truth      +0.05 m x   +0.10 m y   +0.02 rad
    agreement                     0.99658    0.98720     0.99039     0.97946
    against the eight-scan map    0.99790    0.99264     0.99402     0.99045
    moving_only cells             3392
"""
import numpy as np
import pytest

import map_localize_cases as lc
import map_merge_cases as cases
import map_merge_rule as rule
import relocalize_cases as rc
from map_localize_cases import F, O, U

MERGE_CASES = cases.merge_cases()


def test_identity_warp_reproduces_the_moving_cells():
    rng = np.random.default_rng(3)
    for ox, oy, w, h in ((0, 0, 13, 9), (-7, 4, 30, 21), (5, -30, 8, 1)):
        moving = lc.view_of(lc.random_cells(rng, h, w, p_free=0.4, p_occ=0.2), (0.5, -0.25), 20.0, ox, oy)
        blank = lc.view_of(np.zeros((h, w), dtype=np.uint8), (0.5, -0.25), 20.0, ox, oy)
        r = rule.merge(blank, moving, (0.0, 0.0, 0.0), footprint=1, grow=0)
        assert np.array_equal(r.cells[:, :w], moving["cells"][:, :w]) and tuple(r.window) == (ox, oy, w, h, lc.align8(w))
        assert (r.cells[:, w:] == 0).all() and r.overlap == 0 and r.counters["moving_only"] == int((moving["cells"][:, :w] != U).sum())
        grown = rule.merge(blank, moving, (0.0, 0.0, 0.0), footprint=1, grow=1)
        j0, i0 = oy - grown.window.oy, ox - grown.window.ox
        assert np.array_equal(grown.cells[j0:j0 + h, i0:i0 + w], moving["cells"][:, :w]) and grown.counters == r.counters


def test_the_table_of_all_nine_combinations():
    t, m = cases.table_pair()
    N, T, M, A, MO, MF = rule.NEITHER, rule.TARGET_ONLY, rule.MOVING_ONLY, rule.AGREE, rule.MOVING_OCCUPIED, rule.MOVING_FREE
    codes = [[N, M, M], [T, A, MF], [T, MO, A]]                # row: T = U, O, F; column: M = U, O, F
    by_policy = {rule.CONFLICT_TARGET: (O, F), rule.CONFLICT_MOVING: (F, O), rule.CONFLICT_OCCUPIED: (O, O), rule.CONFLICT_UNKNOWN: (U, U)}
    for conflict, (t_occ_m_free, t_free_m_occ) in by_policy.items():
        r = rule.merge(t, m, (0.0, 0.0, 0.0), footprint=1, conflict=conflict, grow=0)
        assert r.codes[:, :3].tolist() == codes, conflict
        assert r.cells[:, :3].tolist() == [[U, O, F], [O, O, t_occ_m_free], [F, t_free_m_occ, F]], conflict
        assert r.counters == dict(target_only=2, moving_only=2, agree_free=1, agree_occupied=1, conflict_moving_occupied=1, conflict_moving_free=1)
        assert r.overlap == 4 and r.agreement == 0.5 and tuple(r.window) == (0, 0, 3, 3, 8) and r.known_box == (1, 0, 2, 2)


@pytest.mark.parametrize("case", MERGE_CASES, ids=[c.name for c in MERGE_CASES])
def test_cases_sit_on_their_edges(case):
    r = rule.merge(case.target, case.moving, case.correction, case.footprint, case.conflict, case.grow)
    case.check(r)
    assert r.overlap == sum(r.counters[k] for k in rule.COUNTERS[2:]) and sum(r.counters.values()) + int((r.codes == rule.NEITHER).sum()) == r.codes.size
    assert (r.cells[:, r.window.width:] == 0).all() and set(np.unique(r.cells)) <= {U, O, F}


def against(view, full):
    """the share of equal cells among the lattice cells known in both `view` and the view `full`"""
    assert view["anchor"] == full["anchor"] and view["scale"] == full["scale"], "one lattice: indices compare directly"
    x0, y0 = max(view["ox"], full["ox"]), max(view["oy"], full["oy"])
    x1, y1 = min(view["ox"] + view["width"], full["ox"] + full["width"]), min(view["oy"] + view["height"], full["oy"] + full["height"])
    a = view["cells"][y0 - view["oy"]:y1 - view["oy"], x0 - view["ox"]:x1 - view["ox"]]
    b = full["cells"][y0 - full["oy"]:y1 - full["oy"], x0 - full["ox"]:x1 - full["ox"]]
    both = (a != U) & (b != U)
    return float((a[both] == b[both]).sum()) / float(both.sum())


def test_the_real_pair_agrees_best_under_the_true_correction(oracle_lib):
    from common import LASER
    target, moving, truth = cases.real_pair()
    sm = rc.small_map()
    full = lc.occupancy_map(sm.ranges[0:8], sm.poses[0:8], LASER)
    assert tuple(target.offset) == tuple(full.offset), "the merged map lies on the anchor of the map built from all eight scans"
    share = against(truth.view, full.view)
    print(f"truth: agreement {truth.agreement:.5f}, against the eight-scan map {share:.5f}, counters {truth.counters}, window {tuple(truth.window)}")
    for name, correction in cases.PERTURBED.items():
        r = rule.merge(target.view, moving.view, correction, footprint=1, conflict=rule.CONFLICT_OCCUPIED, grow=1)
        other = against(r.view, full.view)
        print(f"{name}: agreement {r.agreement:.5f}, against the eight-scan map {other:.5f}")
        assert truth.agreement > r.agreement, name
        assert share > other, name
    t = target.view
    known_in_target = np.zeros(truth.cells.shape, dtype=bool)
    j0, i0 = t["oy"] - truth.window.oy, t["ox"] - truth.window.ox
    known_in_target[j0:j0 + t["height"], i0:i0 + t["width"]] = t["cells"][:, :t["width"]] != U
    gained = int(((truth.cells != U) & ~known_in_target).sum())
    print(f"{gained} cells known in the merged map and not in the target")
    assert gained == truth.counters["moving_only"] > 0
