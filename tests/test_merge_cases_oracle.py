"""CPU only: every case of tests/merge_cases.py sits on the edge its name says, shown with tests/merge_rule.py and
tests/merge_fit_rule.py alone -- the numpy restatement of the session merge that ends at the occupancy oracle.  Nothing of the library
is loaded; tests/test_merge_edges_gpu.py puts the library next to the same answers."""
import numpy as np
import pytest

import merge_cases as mc
import merge_fit_rule as fr
import merge_rule as rule

TRACE, FIT = mc.trace_cases(), mc.fit_cases()
_cache = {}


def rule_subs(subs):
    return [mc.rule_submap(s) for s in subs]


def trace_answer(case):
    """(rule submaps, merged_grid's dict) of a trace case, computed once per process"""
    if case.name not in _cache:
        subs = rule_subs(case.subs)
        _cache[case.name] = (subs, rule.merged_grid(subs, case.transforms, case.resolution, case.min_pass, case.threshold))
    return _cache[case.name]


def fit_answer(case):
    """(rule's moving submap, reference grid, fits) of a fit case"""
    key = ("fit", case.name)
    if key not in _cache:
        ref_key = ("reference", id(case.others), tuple(case.transforms), case.resolution, case.min_pass, case.threshold)
        if ref_key not in _cache:
            _cache[ref_key] = fr.reference_grid(rule_subs(case.others), case.transforms, case.resolution, case.min_pass, case.threshold)
        moving = mc.rule_submap(case.moving)
        _cache[key] = (moving, _cache[ref_key], fr.fit_on(moving, case.candidates, _cache[ref_key], case.resolution))
    return _cache[key]


def test_the_names_are_distinct():
    for cases in (TRACE, FIT):
        assert len({c.name for c in cases}) == len(cases)


def test_the_frame_makes_the_grid_the_cases_count_on():
    g = rule.merged_grid(rule_subs([mc.FRAME]), [mc.IDENTITY], mc.RES, 0, 0.1)
    assert (g["width"], g["height"]) == (mc.W, mc.H) and g["offset"].tolist() == [0.0, 0.0]
    g = fr.reference_grid(rule_subs(mc.REFERENCE[0]), mc.REFERENCE[1], mc.RES, 0, 0.1)
    assert (g["width"], g["height"]) == (mc.W, mc.H) and g["offset"].tolist() == [0.0, 0.0]
    hist = np.bincount(g["cells"][:, :mc.W].reshape(-1), minlength=256)
    assert hist[0] > 400 and hist[100] > 40 and hist[255] > 200, "the reference of the fits holds all three states"


@pytest.mark.parametrize("case", TRACE, ids=[c.name for c in TRACE])
def test_trace_case_sits_on_its_edge(case):
    subs, grid = trace_answer(case)
    assert all(len(s.scans) <= 6 and s.laser.n_beams <= 130 for s in case.subs)
    case.check(mc.Ctx(case, subs, grid))


@pytest.mark.parametrize("case", TRACE, ids=[c.name for c in TRACE])
def test_build_bound(case):
    """kh_merge_build has no walk guard: its grid is made of the boxes of the scans it traces, so every sensor cell and every end
    cell lies within range_threshold * scale + 2 cells of the grid -- and within the int32 lattice, the grid being capped"""
    subs, grid = trace_answer(case)
    assert mc.build_bound(case, subs, grid) >= 1


@pytest.mark.parametrize("case", FIT, ids=[c.name for c in FIT])
def test_fit_case_sits_on_its_edge(case):
    moving, grid, fits = fit_answer(case)
    assert len(case.moving.scans) <= 6 and case.moving.laser.n_beams <= 130
    assert fr.fit_refused(moving, case.candidates, grid, case.resolution) is None
    case.check(fits, grid)


def test_fit_layout_covers_every_remainder_and_count():
    seen = {}
    for sub in mc.layout_moving():
        n = sub.laser.n_beams
        seen.setdefault(n, set()).add((len(sub.scans) * ((n + 63) // 64)) % 4)
    assert seen == {1: {1, 3}, 63: {2}, 64: {3}, 65: {2}, 130: {3, 2, 1}}
    assert set(seen) == set(mc.BEAM_COUNTS)
    assert {len(c.candidates) for c in FIT if "candidates" in c.name and "workgroup" in c.name} == {1, 2, 5, 70}


def test_the_bound_of_the_fit():
    """the sensor cell at exactly +-2^30 from the offset is accepted and counts nothing, a metre outward is refused, FAR is accepted;
    the long laser at the fine resolution is refused whatever the candidate"""
    moving = mc.rule_submap(mc.ORIGIN_RAY)
    grid = fr.reference_grid(rule_subs(mc.REFERENCE[0]), mc.REFERENCE[1], mc.RES, 0, 0.1)
    for c in mc.ACCEPTED[:4]:
        sx, sy = rule.transform_point(c, 0.0, 0.0)
        cells = ((sx - grid["offset"][0]) * mc.SCALE, (sy - grid["offset"][1]) * mc.SCALE)
        assert max(abs(v) for v in cells) == 2.0 ** 30
    assert fr.fit_refused(moving, mc.ACCEPTED, grid, mc.RES) is None
    for f in fr.fit_on(moving, mc.ACCEPTED, grid, mc.RES):
        assert all(f[k] == 0 for k in fr.FIELDS[:-1]) and f["score"] == 0.0
    for k, c in enumerate(mc.REFUSED):
        assert fr.fit_refused(moving, [mc.IDENTITY] * k + [c] + [mc.IDENTITY], grid, mc.RES) == ("pose", k)
    fine = fr.reference_grid(rule_subs([mc.TINY]), [mc.IDENTITY], mc.FINE_RES, 0, 0.1)
    assert 100 < fine["width"] < 1000 and 100 < fine["height"] < 1000
    long_laser = mc.rule_submap(mc.LONG_LASER)
    assert fr.fit_refused(long_laser, [mc.IDENTITY], fine, mc.FINE_RES) == ("laser", -1)
    assert fr.fit_refused(long_laser, [mc.IDENTITY], grid, mc.RES) is None, "the same laser on 0.25 m cells is fine"
    assert len(mc.NOT_FINITE) == 9 and all(sum(not np.isfinite(v) for v in t) == 1 for t in mc.NOT_FINITE)
