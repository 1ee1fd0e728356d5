"""CPU: the fit and alignment rule (tests/merge_fit_rule.py, DESIGN.md section 7a "Fit and alignment") pinned on its own -- the GPU
tests (tests/test_merge_fit_gpu.py, tests/test_merge_align_gpu.py) then pin the library to this rule exactly."""
import math

import numpy as np

import merge_fit_rule as fr
import merge_rule as rule
from test_merge_rule_oracle import RES, _close, _lattice_submap, _matrix, _of_matrix, _scan

FAR = (1000.0, 1000.0, 0.0)          # 20000 cells from any grid of the synthetic world: every beam of every scan is outside


def test_the_six_counters_are_all_of_the_moving_submaps_visits():
    """every visit inside the grid falls on a cell in exactly one of the three states"""
    others, moving = [_lattice_submap(6)], _lattice_submap(3)
    moving["scans"] = moving["scans"][1:]
    grid = fr.reference_grid(others, [rule.IDENTITY], RES)
    assert set(np.unique(grid["cells"]).tolist()) == {0, 100, 255}
    for c in (rule.IDENTITY, (0.4, -0.3, 0.2), (3.0, -2.0, 0.7)):
        p, h = rule.submap_counters(moving, c, grid["width"], grid["height"], grid["offset"], RES)
        f = fr.fit_on(moving, [c], grid, RES)[0]
        assert f["pass_unknown"] + f["pass_occupied"] + f["pass_free"] == int(p.sum(dtype=np.uint64)) > 0
        assert f["hits_unknown"] + f["hits_occupied"] + f["hits_free"] == int(h.sum(dtype=np.uint64)) > 0
        # a hit's cell has been passed by its own line: twice the hits never exceed the visits, state by state
        assert all(f[f"pass_{s}"] >= 2 * f[f"hits_{s}"] for s, _ in fr.STATES)
        assert f["known"] == f["agree"] + f["conflict"] and f["score"] == f["agree"] / f["known"]


def test_a_session_fits_itself_best_under_the_identity():
    sm = _lattice_submap(8, 360)
    # a quarter turn about the origin (it leaves the grid: nothing known) and one about the centre of the session's own grid
    centre = rule.initial_location(sm, RES)
    about_centre = rule.compose(rule.compose(centre, (0.0, 0.0, math.pi / 2)), rule.inverse(centre))
    same, shifted, turned, spun = fr.fit(sm, [rule.IDENTITY, (0.5, 0.0, 0.0), (0.0, 0.0, math.pi / 2), about_centre], [sm], [rule.IDENTITY], RES)
    print(f"identity {same['score']!r} ({same['agree']} / {same['known']}), 0.5 m {shifted['score']!r}, quarter turn {turned['score']!r}, "
          f"quarter turn about the centre {spun['score']!r} ({spun['agree']} / {spun['known']})")
    assert same["hits_occupied"] > 0 and spun["known"] > 0
    assert same["score"] > shifted["score"] and same["score"] > turned["score"] and same["score"] > spun["score"]


def test_a_correction_that_leaves_the_grid_counts_nothing():
    sm = _lattice_submap(4)
    f = fr.fit(sm, [FAR], [sm], [rule.IDENTITY], RES)[0]
    assert all(f[k] == 0 for k in fr.FIELDS) and f["score"] == 0.0 and math.copysign(1.0, f["score"]) == 1.0


def test_no_other_submap_is_refused():
    for others in ([], [{"laser": None, "scans": []}]):
        try:
            fr.reference_grid(others, [rule.IDENTITY] * len(others), RES)
        except ValueError:
            continue
        raise AssertionError("accepted")


def _fit(agree, conflict):
    return {"agree": agree, "conflict": conflict, "known": agree + conflict, "score": agree / (agree + conflict) if agree + conflict else 0.0}


def test_ranking():
    #        0: 0.75      1: 0.75, more agree  2: 0.9 on little  3: = 1         4: nothing known   5: 0.5
    fits = [_fit(30, 10), _fit(60, 20), _fit(9, 1), _fit(60, 20), _fit(0, 0), _fit(50, 50)]
    assert fr.ranking(fits) == [2, 1, 3, 0, 5, 4]                 # score, then agree, then index (1 before 3)
    assert fr.ranking(fits, min_known=40) == [1, 3, 0, 5, 2, 4]   # 2 and 4 know too little: last, ranked among themselves
    assert fr.ranking(fits, min_known=10 ** 6) == fr.ranking(fits)
    assert fr.ranking([_fit(0, 0)] * 3) == [0, 1, 2]


def test_candidate_composition_agrees_with_homogeneous_matrices():
    rng = np.random.default_rng(11)
    for _ in range(200):
        t, p, q = (np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3.1, 3.1)]) for _ in range(3))
        assert _close(fr.candidate(t, p, q), _of_matrix(_matrix(t) @ _matrix(p) @ np.linalg.inv(_matrix(q))))
    # the probe itself: at Q in its own session, the candidate carries it to T . P
    assert _close(rule.compose(fr.candidate(t, p, q), q), rule.compose(t, p))


def test_probe_entries():
    n_probes = 4
    assert fr.probe_entries(1, n_probes) == [0]
    assert fr.probe_entries(3, n_probes) == [0, 1, 2]
    assert fr.probe_entries(n_probes, n_probes) == [0, 1, 2, 3]
    assert fr.probe_entries(n_probes + 1, n_probes) == [0, 1, 2, 3]
    assert fr.probe_entries(10, n_probes) == [0, 2, 5, 7] and fr.probe_entries(10, 1) == [0] and fr.probe_entries(0, n_probes) == []


def test_candidate_list():
    """candidate 0 is the current correction; then the probes in order, each one's hypotheses in rank order, cut at top_k, no
    de-duplication"""
    ids, corrected = [3, 4, 8, 9, 12], np.array([[k, 2.0 * k, 0.1 * k] for k in range(5)], dtype=np.float64)
    answers = {0: [((1.0, 2.0, 0.3), 0.9), ((1.0, 2.0, 0.3), 0.8), ((5.0, 5.0, 0.0), 0.7)], 2: []}
    current, target = (0.5, 0.25, -0.1), (2.0, -1.0, 0.5)
    got = fr.candidates(current, target, ids, corrected, 2, 2, lambda entry: answers[entry])
    assert [(c.probe_scan, c.hypothesis, c.fine_response) for c in got] == [(-1, -1, 0.0), (3, 0, 0.9), (3, 1, 0.8)]
    assert np.array_equal(got[0].correction, np.array(current)) and np.array_equal(got[1].correction, got[2].correction)
    assert np.array_equal(got[1].correction, fr.candidate(target, (1.0, 2.0, 0.3), corrected[0]))


def test_alignment_by_the_rule_alone_on_the_small_map():
    """relocalize_rule end to end into the candidates and the fit: the held-out scan of tests/relocalize_cases.py's small map as a
    session of one scan that believes itself at Q, aligned to the map.  Every candidate carries the probe to its hypothesis' pose
    (to 1e-12, the tolerance of the composition above); the current correction leaves the scan off the map's grid and knows
    nothing; the first-ranked candidate puts the scan where test_relocalize_rule_oracle.py found the best hypothesis, within that
    test's own bounds (its recorded distance plus one fine cell; one coarse angle window)."""
    import relocalize_cases as rc
    from common import LASER
    from test_relocalize_rule_oracle import FINE_CELL, RECORDED_DISTANCE
    sm = rc.small_map()
    hyps = fr.hypotheses_of(rc.rule_on_small_map())
    assert len(hyps) >= 2
    q = np.array([10.0, -4.0, 1.0])
    moving = {"laser": LASER, "scans": [_scan(sm.query, q, LASER)]}
    target = {"laser": LASER, "scans": [_scan(r, p, LASER) for r, p in zip(sm.ranges, sm.poses)]}
    cands = fr.candidates(rule.IDENTITY, rule.IDENTITY, [0], [q], 4, 8, lambda entry: hyps)
    assert [(c.probe_scan, c.hypothesis) for c in cands] == [(-1, -1)] + [(0, k) for k in range(min(8, len(hyps)))]
    for c in cands[1:]:
        assert _close(rule.compose(c.correction, q), hyps[c.hypothesis][0]) and c.fine_response == hyps[c.hypothesis][1]
    fits = fr.fit(moving, [c.correction for c in cands], [target], [rule.IDENTITY], RES)
    order = fr.ranking(fits)
    assert fits[0]["known"] == 0 and order[-1] == 0 and fits[order[0]]["known"] > 0
    placed = rule.compose(cands[order[0]].correction, q)
    distance, heading = math.hypot(placed[0] - sm.true_pose[0], placed[1] - sm.true_pose[1]), abs(placed[2] - sm.true_pose[2])
    print(f"first-ranked candidate {order[0]} (hypothesis {cands[order[0]].hypothesis}) score {fits[order[0]]['score']!r}: the probe lands {distance!r} m "
          f"and {heading!r} rad from where it was taken; order {order}")
    assert distance <= RECORDED_DISTANCE + FINE_CELL and heading < 0.349
