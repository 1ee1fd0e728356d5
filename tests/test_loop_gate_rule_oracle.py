"""CPU: the numpy restatement of the covariance gate (tests/loop_gate_rule.py) against oracle/loops.py where the two must agree --
D = 0 and chi2 = 0 on the golden graph of the reference -- at its exact boundary, and the mapper's host preparation of a row; and
every case of tests/loop_gate_cases.py against its own claim."""
import os

import numpy as np
import pytest

import loop_gate_cases as lgc
import loop_gate_rule as rule
from oracle import loops

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "loop_candidates.npz"))
CASES = list(lgc.cases())


def test_null_gate_is_the_oracle_on_the_golden_graph():
    """D = 0 with any chi2, and chi2 = 0 with any D: x * 1, x - 0 and x / 1 are exact, so the chains are the plain ones"""
    xy, ptr, idx = G["ref_xy"], G["adj_ptr"], G["adj_idx"]
    n = xy.shape[0]
    d, m = float(G["loop_search_maximum_distance"]), int(G["loop_match_minimum_chain_size"])
    rng = np.random.default_rng(3)
    some = lgc.random_rows(rng, 1, n, 4.0)[0]
    zeros = np.zeros((n, 3, 3))
    n_chains = 0
    for q in range(n):
        assert np.array_equal(rule.gated_sq_all(q, xy, d, 5.991, zeros), [loops.squared_distance(xy[i], xy[q]) for i in range(n)])
        for start in (0, 1, q // 2, q, n - 1):
            want = loops.find_possible_loop_closures(q, xy, ptr, idx, d, m, start=start)
            assert rule.find_loop_candidates(q, xy, ptr, idx, d, m, 5.991, zeros, start=start) == want, (q, start)
            assert rule.find_loop_candidates(q, xy, ptr, idx, d, m, 0.0, some, start=start) == want, (q, start)
            n_chains += len(want)
    assert n_chains > 50


def test_the_exact_boundary():
    """r = 2, chi2 = 4, Dxx = 3: s = 1, a = 4, det = 4 and a scan at (4, 0) has q = 16 / 4 = 4.0 = r * r exactly"""
    s = rule.gate_s(4.0, 2.0)
    assert s == 1.0
    q = rule.gated_sq(4.0, 0.0, s, 3.0, 0.0, 0.0)
    assert q == 4.0
    assert q < 4.0 + rule.KT_TOLERANCE and not q <= 4.0 - rule.KT_TOLERANCE            # in range, not visitable
    assert not rule.gated_sq(4.000001, 0.0, s, 3.0, 0.0, 0.0) < 4.0 + rule.KT_TOLERANCE
    assert not rule.gated_sq(0.0, 2.000001, s, 3.0, 0.0, 0.0) < 4.0 + rule.KT_TOLERANCE
    assert rule.gated_sq(0.0, 2.0, s, 3.0, 0.0, 0.0) == 4.0                              # the minor axis is the plain radius


def test_rows_that_are_no_covariance_are_tested_plainly():
    for row in ((-1.0, 0.0, 2.0), (2.0, 0.0, -1.0), (np.nan, 0.0, 1.0), (1.0, np.nan, 1.0), (1.0, 0.0, np.nan), (np.inf, 0.0, 1.0), (1.0, np.inf, 1.0),
                (1.0, 5.0, 1.0)):                                      # (the last: det(I + s D) = 1.7 * 1.7 - 3.5 * 3.5 < 0)
        assert rule.gated_sq(1.5, -2.5, 0.7, *row) == 1.5 * 1.5 + 2.5 * 2.5, row
    assert rule.gated_sq(1.5, -2.5, rule.gate_s(1.0, 0.0), 1.0, 0.0, 1.0) == 1.5 * 1.5 + 2.5 * 2.5          # r = 0: s is infinite
    assert rule.gated_sq(1.5, -2.5, 0.7, 1.0, 0.0, 1.0) < 1.5 * 1.5 + 2.5 * 2.5


def test_the_capped_row_never_reaches_beyond_max_reach():
    rng = np.random.default_rng(9)
    r, chi2 = 3.0, 5.991
    for max_reach in (7.0, 3.5, 3.0, 2.0):
        D = lgc.random_rows(rng, 1, 400, 1.0)[0] * rng.uniform(0.0, 60.0, size=(400, 1, 1))
        rows = rule.prepare_rows(D, r, chi2, 1.0, max_reach)
        reach = np.array([rule.semi_axis(g, r, chi2) for g in rows])
        assert reach.max() <= max(max_reach, r), (max_reach, reach.max())
        raw = np.array([rule.semi_axis(g, r, chi2) for g in D])
        assert (raw > max_reach).sum() > 50                                            # the cap had work to do
        untouched = chi2 / (r * r) * (D[:, 0, 0] + D[:, 1, 1]) <= max(0.0, (max_reach / r) ** 2 - 1.0)
        assert np.array_equal(rows[untouched], D[untouched])
        if max_reach > r:
            assert untouched.any()
            k = int(np.argmax(raw))                                                    # a scaled row keeps its shape
            assert np.allclose(rows[k] / rows[k][0, 0], D[k] / D[k][0, 0], rtol=1e-12)
        else:
            assert not rows.any()                                                      # no room beyond the plain disk: D = 0
    assert np.array_equal(rule.prepare_rows(D, r, chi2, 0.0, 7.0), np.zeros_like(D))
    assert np.array_equal(rule.prepare_rows(D, r, 0.0, 1.0, 7.0), D)                   # chi2 = 0: s = 0, nothing to cap


def test_the_jump_test():
    C = np.diag([0.01, 0.01, 0.0004])
    D3 = np.diag([0.25, 0.04, 0.001])
    e = np.array([1.0, 0.0, 0.0])
    assert rule.jump_rejects(e, np.zeros((3, 3)), C, 1.0, 7.815)                       # 100 > 7.815
    assert not rule.jump_rejects(e, D3, C, 1.0, 7.815)                                 # 1 / 0.26 = 3.85
    assert rule.jump_rejects(e, D3, C, 0.0, 7.815)                                     # covariance_scale 0: the matcher's alone
    assert rule.jump_rejects(np.array([0.0, 1.0, 0.0]), D3, C, 1.0, 7.815)             # 1 / 0.05 = 20: the ellipse is narrow that way
    assert not rule.jump_rejects(e, np.zeros((3, 3)), C, 1.0, 1e300)
    assert rule.jump_rejects(1e-9 * e, D3, C, 1.0, 1e-300)
    assert rule.jump_rejects(0.0 * e, np.diag([1.0, -1.0, 1.0]), C, 1.0, 7.815)        # not positive definite
    assert rule.jump_rejects(0.0 * e, np.diag([1.0, np.nan, 1.0]), C, 1.0, 7.815)


def test_column_passes_of_a_log():
    log = ["N 0 0 0 0", "N 1 0 0 0", "C 0 1", "N 2 0 0 0", "N 3 0 0 0", "X 4 0.1", "P 1 0 0 0", "K", "N 4 0 0 0", "N 5 0 0 0", "N 6 0 0 0"]
    assert rule.column_passes(log, 1) == 6 + 1                 # scans 1-6, and once more behind the closure
    assert rule.column_passes(log, 3) == 1 + 1 + 1             # scan 1 (owed), behind the closure, scan 6 (three calls later)
    assert rule.column_passes(log, 50) == 2


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_shows_what_its_name_says(case):
    assert case.gate.shape == (case.queries.size, case.ref_xy.shape[0], 3, 3)
    case.check(lgc.rule_chains(case), case)
    # the null gates of every case are its plain chains
    assert lgc.rule_chains(case, gate=np.zeros_like(case.gate)) == lgc.plain_chains(case)
    assert lgc.rule_chains(case, chi2=0.0, gate=np.where(np.isfinite(case.gate), case.gate, 0.0)) == lgc.plain_chains(case)
