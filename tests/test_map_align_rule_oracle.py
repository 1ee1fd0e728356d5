"""CPU: the rule of kh_map_align (tests/map_align_rule.py) end to end with the oracle matcher, on the two maps of
tests/map_align_cases.py: scans 2 .. 7 of the small map moved by G against scans 0 .. 5.  The first-ranked candidate must undo G within
half the sequential matcher's search window at the moving map's centre (section 7a's bound) and one coarse angle step in heading."""
import numpy as np

import map_align_cases as cases
import map_align_rule as rule
import map_localize_cases as lc
import map_localize_rule as ml
import relocalize_cases as rc
import relocalize_rule as rr
from common import LASER, OFFLINE_PARAMS

N_PROBES = cases.SETTING["n_probes"]                         # (with two the first-ranked candidate is the next aisle, 0.43 m off: aisles repeat)


def test_probes_are_the_seeds_that_see_most(oracle_lib):
    _, moving = cases.maps()
    cells, hits, probes = rule.probes_of(moving.view, LASER, cases.SETTING["probe_spacing"], 3, cases.SETTING["max_unknown"])
    print(f"{len(cells)} seeds, hits {hits}, probes {[p.seed for p in probes]}")
    assert len(cells) == len(hits) > 3 and [p.seed for p in probes] == rule.pick_probes(hits, 3)
    assert all(p.hits == hits[p.seed] and p.hits >= max(h for k, h in enumerate(hits) if k not in [q.seed for q in probes]) for p in probes)
    assert min(p.hits for p in probes) > LASER.n_beams // 2, "a probe sees walls on most of its beams"
    assert all(ml.state_at(moving.view, int(cells[p.seed][0]), int(cells[p.seed][1])) == lc.F and p.robot[2] == 0.0 for p in probes)
    assert rule.pick_probes([0, 0], 3) == [] and rule.pick_probes([2, 5, 5, 0, 1], 2) == [1, 2]


def test_alignment_undoes_the_known_motion(oracle_lib):
    from oracle import karto
    target, moving = cases.maps()
    coarse = karto.Matcher(*lc.COARSE, LASER.range_threshold, OFFLINE_PARAMS, threads=8)
    fine = karto.Matcher(*lc.FINE, LASER.range_threshold, OFFLINE_PARAMS, threads=8)

    def relocalize(ranges):
        res = ml.relocalize(target.view, ranges, LASER, coarse, fine, OFFLINE_PARAMS, rc.GATES, cases.RELOCALIZE["seed_spacing"],
                            cases.RELOCALIZE["n_headings"])
        return [(rr.robot_at(res.hyps[k].fine_mean), res.hyps[k].fine_response) for k in res.kept]

    res = rule.align(target.view, moving.view, LASER, relocalize, **dict(cases.SETTING, n_probes=N_PROBES))
    assert len(res.probes) == N_PROBES and len(res.candidates) > 1
    assert np.array_equal(res.candidates[0].correction, np.zeros(3)) and res.candidates[0].probe_seed == -1
    for i in res.order:
        c, f = res.candidates[i], res.fits[i]
        d, dh = cases.from_the_truth(c.correction, moving)
        print(f"candidate {i} (probe {c.probe_seed}, hypothesis {c.hypothesis}, fine {c.fine_response:.4f}): score {f['score']:.5f} agree {f['agree']} "
              f"known {f['known']}; {d:.3f} m and {dh:.4f} rad from the truth")
    best = res.order[0]
    d, dh = cases.from_the_truth(res.candidates[best].correction, moving)
    assert best != 0 and res.fits[best]["score"] > res.fits[0]["score"]
    assert d <= lc.FINE[0] / 2 and dh <= OFFLINE_PARAMS["coarse_angle_resolution"]
