"""GPU: the map localizer (kh_map_localizer_*, csrc/map_localizer.cpp) against tests/map_localize_rule.py: relocalization on the small
map hypothesis by hypothesis -- means, covariances and responses bit for bit, fit counters, ranking, duplicates, summary -- and
tracking step by step.  The map is the occupancy oracle's, handed over as cell states in memory of the test's own, and once more as
nav values."""
import math

import numpy as np
import pytest

import map_localize_cases as cases
import map_localize_rule as rule
import map_match_rule as mr
import relocalize_cases as rc
import relocalize_rule as rr
from common import LASER, OFFLINE_PARAMS, bits
from slam_toolbox_amd import capi, synth
from slam_toolbox_amd.map_localizer import MapLocalizer
from test_map_fit_gpu import same_fit
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

SPACING = cases.PITCH * cases.RESOLUTION
PARAMS = dict(loop_search_space_dimension=cases.COARSE[0], loop_search_space_resolution=cases.COARSE[1],
              loop_search_space_smear_deviation=cases.COARSE[2], correlation_search_space_dimension=cases.FINE[0],
              correlation_search_space_resolution=cases.FINE[1], correlation_search_space_smear_deviation=cases.FINE[2])


def center():
    sm, _ = cases.small_map()
    return (sm.true_pose[0] + cases.CENTER_OFFSET[0], sm.true_pose[1] + cases.CENTER_OFFSET[1])


def region(gates=rc.GATES, **kw):
    return dict(dict(seed_spacing=SPACING, n_headings=cases.N_HEADINGS, center_xy=center(), radius=cases.RADIUS,
                     minimum_response_coarse=gates[0], maximum_variance_coarse=gates[1], minimum_response_fine=gates[2]), **kw)


@pytest.fixture(scope="module")
def small(kartohip_lib, oracle_lib):
    """the small map in device memory of the test's own, and a localizer on it"""
    sm, m = cases.small_map()
    d = DeviceView(m.view)
    loc = MapLocalizer(PARAMS, LASER, max_batch=24).set_map(d.v)
    yield sm, m, d, loc
    loc.close()
    d.close()


def same_hypothesis(got, want, want_fit):
    assert got.index == want.index and tuple(got.seed_cell) == tuple(want.seed_cell)
    assert np.array_equal(bits(got.heading), bits(want.heading))
    for a, b in ((got.coarse_mean, want.coarse_mean), (got.coarse_cov, want.coarse_cov), (got.coarse_response, want.coarse_response),
                 (got.fine_mean, want.fine_mean), (got.fine_cov, want.fine_cov), (got.fine_response, want.fine_response)):
        assert np.array_equal(bits(a), bits(b)), (got.index, a, b)
    assert np.array_equal(bits(got.robot_pose), bits(rr.robot_at(want.fine_mean)))
    same_fit(got.fit, want_fit)


def same_answer(hyps, summary, want, top=None):
    kept = want.kept if top is None else want.kept[:top]
    assert [h.index for h in hyps] == [want.hyps[k].index for k in kept]
    for h, k in zip(hyps, kept):
        same_hypothesis(h, want.hyps[k], want.fits[k])
    counts = {k: summary[k] for k in ("n_seeds", "n_headings", "n_hypotheses", "n_passed", "n_accepted", "n_rejected_fit", "n_duplicates", "n_returned")}
    assert counts == dict(n_seeds=len(want.cells), n_headings=len(want.headings), n_hypotheses=len(want.hyps), n_passed=sum(h.passed for h in want.hyps),
                          n_accepted=len(want.accepted), n_rejected_fit=len(want.rejected_fit), n_duplicates=len(want.duplicates), n_returned=len(kept))


def test_region_equals_the_rule(small):
    sm, m, d, loc = small
    before = d.download()
    hyps, summary = loc.relocalize(sm.query, **region())
    want = cases.rule_on_small_map()
    same_answer(hyps, summary, want)
    assert summary["n_duplicates"] >= 1 and summary["n_accepted"] > summary["n_returned"] >= 1
    best = hyps[0]
    dist = math.hypot(best.robot_pose[0] - sm.true_pose[0], best.robot_pose[1] - sm.true_pose[1])
    assert dist <= 0.5 * math.sqrt(2.0) * cases.RESOLUTION + 0.01
    assert abs(rule.normalize_angle(best.robot_pose[2] - sm.true_pose[2])) <= OFFLINE_PARAMS["fine_search_angle_offset"]
    assert summary["seed_kernel_ms"] > 0 and summary["fit_kernel_ms"] > 0 and summary["total_ms"] >= summary["coarse_ms"] + summary["fine_ms"]
    assert np.array_equal(d.download(), before), "the localizer wrote the view's cells"
    st = loc.stats()
    assert st["relocalizations"] >= 1 and st["hypotheses"] >= summary["n_hypotheses"] and st["poses_fitted"] >= summary["n_accepted"]


def test_open_gates_return_every_hypothesis(small):
    """8 seeds x 8 headings: with every gate open and no suppression all 64 come back, both matches of each compared bit for bit"""
    sm, m, d, loc = small
    hyps, summary = loc.relocalize(sm.query, cap=100, top_k=0, **region(rc.OPEN_GATES, merge_distance=0.0))
    want = cases.rule_on_small_map(gates=rc.OPEN_GATES, merge_distance=0.0)
    assert len(want.cells) * cases.N_HEADINGS == len(want.hyps) == len(want.kept) == len(hyps) == 64
    same_answer(hyps, summary, want)
    # the gates applied afterwards give the gated run's counts
    gated = cases.rule_on_small_map()
    by_index = {h.index: h for h in hyps}
    passed = [i for i, h in by_index.items() if h.coarse_response > rc.GATES[0] and h.coarse_cov[0, 0] < rc.GATES[1] and h.coarse_cov[1, 1] < rc.GATES[1]]
    assert sorted(passed) == sorted(h.index for h in gated.hyps if h.passed)


def test_top_k_and_cap_truncate_the_answer_not_the_summary(small):
    sm, m, d, loc = small
    want = cases.rule_on_small_map()
    assert len(want.kept) >= 3
    for kw, n in ((dict(top_k=2), 2), (dict(cap=1), 1), (dict(cap=3, top_k=0), 3), (dict(cap=0), 0), (dict(cap=2, top_k=5), 2)):
        hyps, summary = loc.relocalize(sm.query, **region(), **kw)
        assert len(hyps) == n == summary["n_returned"]
        same_answer(hyps, summary, want, top=n)
        assert summary["n_accepted"] == len(want.accepted) and summary["n_duplicates"] == len(want.duplicates)


def test_min_fit_score_around_the_best(small):
    sm, m, d, loc = small
    want = cases.rule_on_small_map()
    best = want.fits[want.kept[0]]["score"]
    above, below = math.nextafter(best, math.inf), math.nextafter(best, -math.inf)
    hyps, summary = loc.relocalize(sm.query, **region(min_fit_score=above))
    same_answer(hyps, summary, cases.rule_on_small_map(min_fit_score=above))
    assert summary["n_rejected_fit"] >= 1 and want.hyps[want.kept[0]].index not in [h.index for h in hyps]
    for score in (best, below):
        hyps, summary = loc.relocalize(sm.query, **region(min_fit_score=score))
        same_answer(hyps, summary, cases.rule_on_small_map(min_fit_score=score))
        assert hyps[0].index == want.hyps[want.kept[0]].index


def test_no_suppression_returns_the_duplicates(small):
    sm, m, d, loc = small
    want = cases.rule_on_small_map(merge_distance=0.0)
    hyps, summary = loc.relocalize(sm.query, **region(merge_distance=0.0))
    same_answer(hyps, summary, want)
    assert summary["n_duplicates"] == 0 and len(hyps) == len(want.accepted) > len(cases.rule_on_small_map().kept)


def test_whole_map(small):
    """spacing 2.0 m, the default headings: the best hypothesis is the rule's for that index, and the region run's best pose"""
    sm, m, d, loc = small
    hyps, summary = loc.relocalize(sm.query, seed_spacing=2.0)
    assert summary["n_headings"] == 10 == rr.default_n_headings(OFFLINE_PARAMS["coarse_search_angle_offset"])
    cells, _ = rule.seeds(m.view, 2.0)
    assert summary["n_seeds"] == len(cells) > 40 and summary["n_hypotheses"] == 10 * len(cells) and summary["n_returned"] >= 1
    want = cases.rule_on_small_map(spacing=2.0, n_headings=10, region=False, only=[hyps[0].index])
    assert want.hyps[0].accepted
    same_hypothesis(hyps[0], want.hyps[0], want.fits[0])
    near = cases.rule_on_small_map()
    best = near.hyps[near.kept[0]].fine_mean
    assert math.hypot(hyps[0].fine_mean[0] - best[0], hyps[0].fine_mean[1] - best[1]) < 0.05
    assert abs(rule.normalize_angle(hyps[0].fine_mean[2] - best[2])) < OFFLINE_PARAMS["coarse_angle_resolution"]
    print(f"whole map: {summary['n_seeds']} seeds, {summary['n_hypotheses']} hypotheses, {summary['n_passed']} passed, {summary['n_accepted']} accepted, "
          f"{summary['n_duplicates']} duplicates; coarse {summary['coarse_ms']:.1f} ms, fine {summary['fine_ms']:.1f} ms, total {summary['total_ms']:.1f} ms")


def test_the_same_map_as_nav_values(small):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    sm, m, d, loc = small
    g = OccupancyGrid.from_nav(m.nav, m.offset, cases.RESOLUTION)
    assert np.array_equal(g.cells()[:, :m.width], m.view["cells"][:, :m.width])
    other = MapLocalizer(PARAMS, LASER, max_batch=7).set_map(g)      # (another batch size: the answer does not depend on it)
    hyps, summary = other.relocalize(sm.query, **region())
    same_answer(hyps, summary, cases.rule_on_small_map())
    other.close(); g.close()


def test_handle_states(small):
    sm, m, d, loc = small
    fresh = MapLocalizer(PARAMS, LASER, max_batch=2)
    for call in (lambda: fresh.relocalize(sm.query), lambda: fresh.process(sm.query, np.zeros(3)), lambda: fresh.get_pose()):
        with pytest.raises(capi.KartoHipError) as e:
            call()
        assert e.value.code == capi.KH_ERR_NOT_FOUND
    for field, value in (("width", 0), ("device", 1), ("scale", math.nan), ("device_cells", None)):
        w = capi.KhMapView.from_buffer_copy(d.v)
        setattr(w, field, value)
        with pytest.raises(capi.KartoHipError) as e:
            fresh.set_map(w)
        assert e.value.code == capi.KH_ERR_INVALID_ARG
    fresh.set_map(d.v)
    with pytest.raises(capi.KartoHipError) as e:
        fresh.process(sm.query, np.zeros(3))
    assert e.value.code == capi.KH_ERR_NOT_FOUND, "a map but no pose"
    with pytest.raises(capi.KartoHipError) as e:
        fresh.relocalize(sm.query, seed_spacing=4097 * cases.RESOLUTION)
    assert e.value.code == capi.KH_ERR_INVALID_ARG
    # a map without a free cell: KH_OK with zero everything
    blank = DeviceView(cases.view_of(np.full((40, 50), cases.O, dtype=np.uint8), (0.0, 0.0), 20.0))
    hyps, summary = fresh.set_map(blank.v).relocalize(sm.query)
    assert hyps == [] and all(summary[k] == 0 for k in summary if k.startswith("n_") and k != "n_headings")
    fresh.close(); blank.close()


def test_relocalize_then_track(small):
    """the answer of a relocalization carries a tracking step: set_pose(best.robot_pose), then process of the same scan stays there"""
    sm, m, d, loc = small
    hyps, _ = loc.relocalize(sm.query, **region())
    loc.set_pose(hyps[0].robot_pose)
    robot, odom = loc.get_pose()
    assert np.array_equal(robot, hyps[0].robot_pose) and np.array_equal(odom, hyps[0].robot_pose)
    step = loc.process(sm.query, hyps[0].robot_pose)
    assert np.array_equal(bits(step.predicted_pose), bits(hyps[0].robot_pose)), "no odometric motion: the prediction is the pose itself"
    assert math.hypot(step.robot_pose[0] - sm.true_pose[0], step.robot_pose[1] - sm.true_pose[1]) <= 0.5 * math.sqrt(2.0) * cases.RESOLUTION + 0.01
    assert step.response > 0.5 and step.fit["score"] > 0.99
    assert np.array_equal(loc.get_pose()[0], step.robot_pose)


def test_tracking_equals_the_rule_and_a_chain(kartohip_lib, oracle_lib):
    """The setting of test_map_localises_like_a_chain: the map of 40 trajectory scans at 0.05 m, then scans 40 .. 45 with odometry =
    truth + a constant drift inside the sequential window, from scan 39's true pose.  Every step equals the rule bit for bit, and lies
    no further from the truth than the oracle's match of the same scan against its nearest 10 scans plus half a map-cell diagonal plus
    one fine step (the bound derived there)."""
    from oracle import karto
    create = (0.3, 0.01, 0.03)
    world, rng = synth.make_world(12345), np.random.default_rng(77)
    truth, _ = synth.trajectory(60)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(46)]
    m = cases.occupancy_map(ranges[:40], truth[:40], LASER)
    d = DeviceView(m.view)
    before = d.download()
    loc = MapLocalizer(dict(correlation_search_space_dimension=create[0], correlation_search_space_resolution=create[1],
                            correlation_search_space_smear_deviation=create[2]), LASER, max_batch=1).set_map(d.v)
    seq = karto.Matcher(*create, LASER.range_threshold, OFFLINE_PARAMS)
    chain = karto.Matcher(*create, LASER.range_threshold, OFFLINE_PARAMS)
    pts = mr.map_points(m.view)
    drift = np.array([0.06, -0.05, 0.02])
    loc.set_pose(truth[39])
    robot, odom = truth[39].copy(), truth[39].copy()
    half_diagonal, fine_step = 0.5 * math.sqrt(2.0) * cases.RESOLUTION, create[1]
    base = [karto.Scan(ranges[i], truth[i], LASER) for i in range(40)]
    for i in range(40, 46):
        odometric = truth[i] + drift
        got = loc.process(ranges[i], odometric)
        want = rule.track_step(m.view, pts, LASER, seq, OFFLINE_PARAMS, robot, odom, ranges[i], odometric)
        for a, b in ((got.predicted_pose, want.predicted), (got.sensor_pose, want.sensor_pose), (got.covariance, want.covariance),
                     (got.response, want.response), (got.robot_pose, want.robot_pose)):
            assert np.array_equal(bits(a), bits(b)), (i, a, b)
        same_fit(got.fit, want.fit)
        assert np.array_equal(loc.get_pose()[0], got.robot_pose) and np.array_equal(loc.get_pose()[1], odometric)
        nearest = np.argsort(np.hypot(truth[:40, 0] - truth[i, 0], truth[:40, 1] - truth[i, 1]))[:10]
        _, mean_chain, _ = chain.match_scan(karto.Scan(ranges[i], want.sensor_start, LASER), [base[k] for k in sorted(nearest)])
        dp_map = math.hypot(got.sensor_pose[0] - truth[i, 0], got.sensor_pose[1] - truth[i, 1])
        dp_chain = math.hypot(mean_chain[0] - truth[i, 0], mean_chain[1] - truth[i, 1])
        print(f"scan {i}: response {got.response:.4f}, fit score {got.fit['score']:.5f}, map {dp_map:.4f} m and chain {dp_chain:.4f} m from the truth")
        assert got.response > 0.1 and dp_map - dp_chain <= half_diagonal + fine_step
        robot, odom = want.robot_pose, odometric
    assert loc.stats()["steps"] == 6 and np.array_equal(d.download(), before)
    loc.close(); d.close()
