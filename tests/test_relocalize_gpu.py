"""GPU: Mapper.relocalize (kh_mapper_relocalize) on the small map of tests/relocalize_cases.py against the rule
(tests/relocalize_rule.py with oracle.karto.Matcher): the same hypotheses, gate and acceptance, bit-equal matches, the same
ranking; truncation; the region; the mapper left as it was; the round trip load -> relocalize -> ProcessAgainstNodesNearBy; a
mapper on two members."""
import math

import numpy as np
import pytest

import relocalize_cases as rc
import relocalize_rule as rr
from common import LASER, bits
from test_relocalize_rule_oracle import FINE_CELL, RECORDED_DISTANCE

pytestmark = pytest.mark.gpu
NH = rc.N_HEADINGS


def make_mapper(devices=None, gates=rc.GATES):
    """the small map in a mapper: the scans enter through Process (matching on, as in a saved session) and are then put exactly at
    the map's poses, so the library and the rule see the same map"""
    from slam_toolbox_amd.mapper import Mapper
    sm = rc.small_map()
    m = Mapper(LASER, max_candidates=16, devices=devices, do_loop_closing=0, minimum_travel_distance=0.2,
               loop_match_minimum_response_coarse=gates[0], loop_match_maximum_variance_coarse=gates[1], loop_match_minimum_response_fine=gates[2],
               **rc.MAPPER_PARAMS)
    for k, (r, p) in enumerate(zip(sm.ranges, sm.poses)):
        assert m.Process(r, p, float(k))[0]
    for k, p in enumerate(sm.poses):
        m.set_scan_pose(k, p)
    return m


@pytest.fixture(scope="module")
def mapper(kartohip_lib):
    m = make_mapper()
    yield m
    m.close()


def same_hypothesis(got, want, seeds):
    assert got.index == want.index and got.seed_scan == seeds[want.index // NH] == want.seed
    assert bits([got.heading])[0] == bits([want.heading])[0]
    for name in ("coarse_mean", "coarse_cov", "fine_mean", "fine_cov"):
        assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), (want.index, name)
    assert bits([got.coarse_response])[0] == bits([want.coarse_response])[0] and bits([got.fine_response])[0] == bits([want.fine_response])[0]
    assert np.array_equal(bits(got.robot_pose), bits(rr.robot_at(want.fine_mean)))


def check_against(hyps, summary, want, cap=None):
    passed = [h for h in want.hyps if h.passed]
    assert (summary["n_seeds"], summary["n_headings"], summary["n_hypotheses"]) == (want.seeds.size, NH, len(want.hyps))
    assert (summary["n_passed"], summary["n_accepted"]) == (len(passed), len(want.ranking))
    expect = want.ranking if cap is None else want.ranking[:cap]
    assert summary["n_returned"] == len(hyps) == len(expect) and [h.index for h in hyps] == expect
    for h in hyps:
        same_hypothesis(h, want.hyps[h.index], want.seeds)


def test_library_equals_the_rule(mapper):
    sm = rc.small_map()
    want = rc.rule_on_small_map()
    hyps, summary = mapper.relocalize(sm.query, cap=64, n_headings=NH, top_k=0)
    assert len(want.ranking) >= 2 and summary["n_passed"] > summary["n_accepted"]
    check_against(hyps, summary, want)
    assert summary["kernel_ms"] > 0 and summary["total_ms"] >= summary["batch_ms"] > 0


def test_every_hypothesis_with_open_gates(kartohip_lib):
    """thresholds that let everything through: all 24 hypotheses come back, so every coarse and every fine match -- what the gate
    and the acceptance are computed from -- is compared bit for bit"""
    sm = rc.small_map()
    want = rc.rule_on_small_map(gates=rc.OPEN_GATES)
    m = make_mapper(gates=rc.OPEN_GATES)
    hyps, summary = m.relocalize(sm.query, cap=64, n_headings=NH, top_k=0)
    m.close()
    assert len(hyps) == 24 == len(want.ranking)
    check_against(hyps, summary, want)
    # ... and the real thresholds applied to those numbers give the real run's flags
    real = rc.rule_on_small_map()
    by_index = {h.index: h for h in hyps}
    for w in real.hyps:
        g = by_index[w.index]
        passed = g.coarse_response > rc.GATES[0] and g.coarse_cov[0, 0] < rc.GATES[1] and g.coarse_cov[1, 1] < rc.GATES[1]
        assert passed == w.passed and (passed and g.fine_response >= rc.GATES[2]) == w.accepted


def test_top_k_and_cap_truncate_but_the_summary_does_not(mapper):
    sm = rc.small_map()
    want = rc.rule_on_small_map()
    assert len(want.ranking) > 2
    for kwargs, n in ((dict(cap=2, top_k=0), 2), (dict(cap=64, top_k=1), 1), (dict(cap=1, top_k=3), 1), (dict(cap=0, top_k=0), 0)):
        hyps, summary = mapper.relocalize(sm.query, n_headings=NH, **kwargs)
        check_against(hyps, summary, want, cap=n)


def test_default_heading_count(mapper):
    """n_headings 0: ceil(2 pi / (2 * 0.349)) = 10 headings per seed"""
    _, summary = mapper.relocalize(rc.small_map().query, cap=0, center_xy=(2.5, 3.0), radius=0.1)
    assert (summary["n_seeds"], summary["n_headings"], summary["n_hypotheses"]) == (1, 10, 10)


def test_region_selects_the_rules_seeds(mapper):
    sm = rc.small_map()
    center, radius = (float(sm.poses[5, 0]), float(sm.poses[5, 1])), 1.6          # seeds 3 (1.5 m away) and 5, not seed 0 (3 m)
    want = rc.rule_on_small_map(center=center, radius=radius)
    assert want.seeds.tolist() == [3, 5]
    hyps, summary = mapper.relocalize(sm.query, cap=64, n_headings=NH, top_k=0, center_xy=center, radius=radius)
    check_against(hyps, summary, want)
    _, none = mapper.relocalize(sm.query, cap=64, n_headings=NH, center_xy=(500.0, 500.0), radius=1.0)
    assert (none["n_seeds"], none["n_hypotheses"], none["n_accepted"], none["n_returned"]) == (0, 0, 0, 0)


def test_relocalize_leaves_the_mapper_as_it_was(kartohip_lib, tmp_path):
    sm = rc.small_map()
    m, twin = make_mapper(), make_mapper()
    m.save(tmp_path / "before.khms")
    before = (m.num_scans(), m.num_edges(), m.poses().copy(), m.alive().copy(), m.stats()["matches"])
    hyps, _ = m.relocalize(sm.query, n_headings=NH)
    assert hyps
    m.save(tmp_path / "after.khms")
    assert (tmp_path / "before.khms").read_bytes() == (tmp_path / "after.khms").read_bytes()
    assert (m.num_scans(), m.num_edges(), m.stats()["matches"]) == (before[0], before[1], before[4])
    assert np.array_equal(bits(m.poses()), bits(before[2])) and np.array_equal(m.alive(), before[3])
    # the next Process: the scan of the held-out node, driven on from the last node of the map
    nxt = sm.poses[-1] + (0.0, 0.4, 0.05)
    got, ref = m.Process(sm.query, nxt, 100.0), twin.Process(sm.query, nxt, 100.0)
    assert got[0] and ref[0] and np.array_equal(bits(got[1]), bits(ref[1])) and np.array_equal(bits(got[2]), bits(ref[2]))
    assert np.array_equal(bits(m.poses()), bits(twin.poses())) and m.num_edges() == twin.num_edges()
    m.close()
    twin.close()


def test_round_trip_load_relocalize_process_near_by(mapper, tmp_path):
    from slam_toolbox_amd.mapper import Mapper
    sm = rc.small_map()
    mapper.save(tmp_path / "map.khms")
    m = Mapper.load(tmp_path / "map.khms", max_candidates=16)
    hyps, summary = m.relocalize(sm.query, n_headings=NH)
    check_against(hyps, summary, rc.rule_on_small_map(), cap=8)
    n = m.num_scans()
    accepted, pose, _ = m.ProcessAgainstNodesNearBy(sm.query, hyps[0].robot_pose, 50.0)
    distance = math.hypot(pose[0] - sm.true_pose[0], pose[1] - sm.true_pose[1])
    print(f"relocalized at {hyps[0].robot_pose}, corrected to {pose}, true {sm.true_pose}: {distance!r} m")
    assert accepted and m.num_scans() == n + 1
    assert distance <= RECORDED_DISTANCE + FINE_CELL
    m.close()


def test_two_members_give_the_same_answer(mapper):
    """hypothesis i on member i % 2, each member on its own matcher pair (the same device listed twice)"""
    sm = rc.small_map()
    one, s1 = mapper.relocalize(sm.query, cap=64, n_headings=NH, top_k=0)
    m2 = make_mapper(devices=[0, 0])
    two, s2 = m2.relocalize(sm.query, cap=64, n_headings=NH, top_k=0)
    m2.close()
    counts = ("n_seeds", "n_headings", "n_hypotheses", "n_passed", "n_accepted", "n_returned")
    assert [s1[k] for k in counts] == [s2[k] for k in counts] and [h.index for h in one] == [h.index for h in two]
    for a, b in zip(one, two):
        for x, y in zip(a, b):
            assert np.array_equal(bits(np.asarray(x, dtype=np.float64)), bits(np.asarray(y, dtype=np.float64)))


def test_empty_map_is_ok_with_zero_everything(kartohip_lib):
    from slam_toolbox_amd.mapper import Mapper
    m = Mapper(LASER, max_candidates=4, **rc.MAPPER_PARAMS)
    hyps, summary = m.relocalize(rc.small_map().query)
    m.close()
    assert hyps == [] and all(summary[k] == 0 for k in ("n_seeds", "n_hypotheses", "n_passed", "n_accepted", "n_returned"))
