"""tests/cell_maxima_cases.py on the CPU: the searches picked for tests/test_cell_maxima_gpu.py sit where that test needs them, shown
on the CPU oracle's response volumes.

* With the penalties on, at least one case has a cell whose best angle by penalised response is NOT its best angle by raw sum: a
  per-cell maximum taken over sums (or over unpenalised responses) instead of over responses shows there.
* "every reading invalid" gives an all-zero lattice: what the same-slot-twice test relies on.
* The angle cases include odd counts: the last workgroup of k_score_lds then has a dead second angle.

One edge that looks missing cannot be reached: "a response at or below 1e-6 skips the penalty" needs sum <= P * 1e-4, and on the
LDS-staged path (P <= 2048) that is sum = 0 only."""
import numpy as np
import pytest

import cell_maxima_cases as cm
import lds_cases as lc

CASES = cm.picked()


@pytest.fixture(scope="module")
def matchers(oracle_lib):
    cache = {}

    def get(case):
        if case.geometry() not in cache:
            cache[case.geometry()] = case.oracle_matcher()
        return cache[case.geometry()]
    return get


def test_the_groups_are_all_there():
    kinds = {c.kind for c in CASES}
    assert {"lattice", "angles", "tails", "fallback", "invalid runs"} == kinds
    assert [c.name for c in CASES if c.kind == "invalid runs"] == [cm.ALL_INVALID]
    assert not any(c.fine for c in CASES) and cm.BIG not in {c.name for c in CASES}
    lattices = {c.want[:3] for c in CASES if c.kind == "lattice"}
    assert {(2, 64, 1), (61, 64, 1), (31, 64, 2), (30, 16, 2)} <= lattices, "every instance: one and two cells, up to and beyond 32 rows"
    # rows per angle team: 1, 2 and 4 waves share them (the partial and the full merge of k_score_lds)
    assert {lc.lds_row_waves(c.want[1]) for c in CASES if c.kind == "lattice"} == {1, 2, 4}
    assert any(True in c.pens for c in CASES) and any(False in c.pens for c in CASES)


def test_angle_cases_include_odd_counts():
    counts = sorted(c.want[3] for c in CASES if c.kind == "angles")
    assert counts == [1, 2, 3, 9]
    assert any(n % 2 == 1 and n > 1 for n in counts), "a dead second angle beside live workgroups"


def test_all_invalid_case_has_a_zero_lattice(matchers):
    case = next(c for c in CASES if c.name == cm.ALL_INVALID)
    om = matchers(case)
    for pen in case.pens:
        lc.run_oracle(om, case, pen)
        lat = cm.expected_lattice(om)
        assert lat.shape == (case.want[1], case.want[0]) and not lat.any()


def test_some_cell_is_best_at_another_angle_with_the_penalties_on(matchers):
    found = []
    for case in CASES:
        if True not in case.pens or False not in case.pens or case.want[3] < 2:
            continue
        om = matchers(case)
        lc.run_oracle(om, case, True)
        pen = om.volume()[..., 0].copy()
        lc.run_oracle(om, case, False)
        raw = om.volume()[..., 0].copy()              # sum / (100 P): ordered like the raw sums
        # cells whose largest raw sum is reached at an angle where the penalised response is NOT the cell's largest
        by_raw = np.take_along_axis(pen, raw.argmax(axis=2)[..., None], axis=2)[..., 0]
        differ = int((by_raw < pen.max(axis=2)).sum())
        if differ:
            found.append((case.name, differ))
    print(found)
    assert found, "no picked case separates the maximum over responses from the maximum over sums"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_non_zero_lattices(matchers, case):
    """every picked case but the all-invalid one has a lattice that is not all zeros (a result block left at K2's zero would show)"""
    om = matchers(case)
    for pen in case.pens:
        lc.run_oracle(om, case, pen)
        lat = cm.expected_lattice(om)
        assert lat.shape == (case.want[1], case.want[0])
        assert lat.any() == (case.name != cm.ALL_INVALID)
