"""GPU: the distance field (kh_map_field_*, MapField; csrc/occupancy_field.hip) against tests/map_field_rule.py on the hand-made views
of tests/map_field_cases.py, uploaded through kh_device_upload, on the fit cases of tests/map_localize_cases.py and on the small map.
Every value a kernel produces is an integer and is compared exactly; the doubles derived from them on the host bit for bit."""
import numpy as np
import pytest

import map_field_cases as cases
import map_field_rule as rule
import map_localize_cases as lc
from common import LASER, bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_field import MapField
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

FIELD_CASES = cases.field_cases()
FIT_CASES = lc.fit_cases()


def same_field(got, want, view, radius):
    st = got.stats
    assert (st["ox"], st["oy"], st["width"], st["height"], st["radius_cells"]) == (view["ox"], view["oy"], view["width"], view["height"], radius)
    d2 = got.d2
    assert d2.dtype == np.uint32 and np.array_equal(d2, want), f"{int((d2 != want).sum())} values differ"
    assert {k: st[k] for k in ("n_obstacles", "n_far", "max_d2")} == rule.stats(want), st
    assert np.array_equal(bits(got.metres), bits(rule.metres(want, view["scale"])))


def field_on(view, radius, obstacles=rule.OCCUPIED):
    d = DeviceView(view)
    got = MapField(d.v, max_distance=radius / view["scale"], obstacles=obstacles)
    assert np.array_equal(d.download(), view["cells"].ravel()), "the view's cells were written"
    d.close()                                                  # the field is a snapshot: the view's memory may go
    return got


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c.name for c in FIELD_CASES])
def test_field_cases(kartohip_lib, case):
    got = field_on(case.view, case.radius, case.obstacles)
    want = rule.d2_brute(case.view, case.radius, case.obstacles)
    same_field(got, want, case.view, case.radius)
    case.check(got.d2)
    t = got.stats["times_ms"]
    assert t[0] > 0 and t[1] > 0 and t[2] >= t[0] + t[1] - 1e-3
    got.close()


@pytest.fixture(scope="module")
def small(kartohip_lib, oracle_lib):
    """the small map on the device, its capped rule field, a capped and an uncapped field of the library"""
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    sm, m = lc.small_map()
    g = OccupancyGrid.from_nav(m.nav, m.offset, lc.RESOLUTION)
    capped, uncapped = MapField(g, max_distance=2.0), MapField(g, max_distance=0.0)
    want = rule.d2_separable(m.view, 40)
    yield sm, m, g, capped, uncapped, want
    capped.close(); uncapped.close()
    g.close()


def test_the_small_map_capped_and_uncapped(small):
    sm, m, g, capped, uncapped, want = small
    assert rule.radius_cells(2.0, m.view["scale"]) == 40
    same_field(capped, want, m.view, 40)
    same_field(uncapped, rule.d2_separable(m.view, 0), m.view, 0)
    print(f"{m.width} x {m.height}: capped {capped.stats['times_ms']}, uncapped {uncapped.stats['times_ms']} ms, max_d2 {uncapped.stats['max_d2']}")


# ---------------------------------------------------------------- costs
@pytest.mark.parametrize("params", range(len(cases.INFLATIONS)))
def test_costs_on_the_table_cases(kartohip_lib, params):
    for case in cases.cost_fields():
        got = field_on(case.view, case.radius, case.obstacles)
        d2 = rule.d2_brute(case.view, case.radius, case.obstacles)
        for track, inflate in cases.UNKNOWN_POLICIES:
            kw = dict(cases.INFLATIONS[params], track_unknown=track, inflate_unknown=inflate)
            costs = got.costs(**kw)
            assert costs.dtype == np.uint8 and np.array_equal(costs, rule.costs(case.view, d2, case.radius, **kw)), (case.name, kw)
        got.close()


def test_costs_on_the_small_map_hold_every_kind_of_value(small):
    sm, m, g, capped, uncapped, want = small
    for field, r in ((capped, 40), (uncapped, 0)):
        costs = field.costs()
        assert np.array_equal(costs, rule.costs(m.view, want if r else rule.d2_separable(m.view, 0), r))
    present = np.bincount(costs.ravel(), minlength=256)
    assert present[0] > 0 and present[1:253].sum() > 0 and present[253] > 0 and present[254] > 0 and present[255] > 0, "a test that cannot pass vacuously"
    assert np.array_equal(capped.costs(track_unknown=1, inflate_unknown=1), rule.costs(m.view, want, 40, track_unknown=1, inflate_unknown=1))


def test_costs_refuse_a_field_that_does_not_reach(kartohip_lib):
    case = next(c for c in FIELD_CASES if c.name == "40 x 50 random, p_occ 0.3, seed 1, R 4")
    got = field_on(case.view, case.radius)
    with pytest.raises(capi.KartoHipError) as e:
        got.costs(inflation_radius=1.01)                       # 5 cells
    assert e.value.code == capi.KH_ERR_INVALID_ARG
    d2 = rule.d2_brute(case.view, case.radius)
    assert np.array_equal(got.costs(inflation_radius=1.0), rule.costs(case.view, d2, 4, inflation_radius=1.0)), "Rt == R is taken"
    with pytest.raises(capi.KartoHipError) as e:
        got.costs(inflation_radius=300.0)                      # above 1024 cells at this scale
    assert e.value.code == capi.KH_ERR_INVALID_ARG
    got.close()


# ---------------------------------------------------------------- clearance
def test_clearance(kartohip_lib):
    for name in ("40 x 50 random, p_occ 0.02, seed 1, R 4", "40 x 50 random, p_occ 0.3, seed 2, R 0"):
        case = next(c for c in FIELD_CASES if c.name == name)
        got = field_on(case.view, case.radius)
        d2 = rule.d2_brute(case.view, case.radius)
        pts = cases.clearance_points(case.view, d2)
        rng = np.random.default_rng(8)
        many = np.concatenate([pts, rng.uniform(-12.0, 12.0, size=(257 - len(pts), 2))])
        assert len(many) == 257
        for xy in (pts[:1], pts, many):
            metres, status, value = got.clearance(xy)
            want_m, want_s, want_v = rule.clearance(case.view, d2, xy)
            assert np.array_equal(status, want_s) and np.array_equal(value, want_v) and np.array_equal(bits(metres), bits(want_m)), name
        if case.radius:
            assert set(want_s.tolist()) == {rule.OK, rule.CLEAR_FAR, rule.OUTSIDE}
        L = capi.lib()
        status = np.zeros(len(pts), dtype=np.int32)
        assert L.kh_map_field_clearance(got._h, len(pts), pts.ctypes.data, None, status.ctypes.data, None) == capi.KH_OK, "any output may be NULL"
        assert np.array_equal(status, rule.clearance(case.view, d2, pts)[1])
        bad = pts.copy()
        bad[3, 1] = np.nan
        assert L.kh_map_field_clearance(got._h, len(bad), bad.ctypes.data, None, status.ctypes.data, None) == capi.KH_ERR_INVALID_ARG
        got.close()


# ---------------------------------------------------------------- score
def same_score(got, want):
    for k in ("n_kept", "n_hit", "n_inside", "n_near", "sum_d2", "cost"):
        assert got[k] == want[k], (k, got, want)
    assert np.array_equal(bits(got["score"]), bits(want["score"]))


@pytest.mark.parametrize("case", FIT_CASES, ids=[c.name for c in FIT_CASES])
def test_score_on_the_fit_cases(kartohip_lib, oracle_lib, case):
    r = 6
    got = field_on(case.view, r)
    d2 = rule.d2_separable(case.view, r)
    for t in (0, 3):
        scores = got.score(case.ranges, case.poses, case.laser, truncate_cells=t)
        assert len(scores) == len(case.poses)
        for s, pose in zip(scores, case.poses):
            same_score(s, rule.score(case.view, d2, r, case.laser, case.ranges, pose, t))
    got.close()


def test_score_shapes_and_refusals(small):
    sm, m, g, capped, uncapped, want = small
    truth = np.asarray(sm.true_pose, dtype=np.float64)
    rng = np.random.default_rng(12)
    poses = truth + rng.uniform(-1.0, 1.0, size=(70, 3)) * [1.5, 1.5, 0.5]
    poses[0] = truth
    scores = capped.score(sm.query, poses, LASER)              # 1081 beams, 70 poses
    for k in (0, 1, 33, 69):
        same_score(scores[k], rule.score(m.view, want, 40, LASER, sm.query, poses[k]))
    for k in range(70):
        same_score(scores[k], rule.score_arrays(m.view, want, 40, LASER, sm.query, poses[k]))
    same_score(capped.score(sm.query, [truth], LASER, truncate_cells=6)[0], rule.score(m.view, want, 40, LASER, sm.query, truth, 6))
    same_score(uncapped.score(sm.query, [truth], LASER, truncate_cells=6)[0], rule.score(m.view, rule.d2_separable(m.view, 0), 0, LASER, sm.query, truth, 6))
    for n in (1, 64, 65):
        laser = lc.circle(n)
        ranges = rng.uniform(0.5, 4.9, size=n)
        same_score(capped.score(ranges, [truth], laser)[0], rule.score(m.view, want, 40, laser, ranges, truth))
    # no hit beam: every reading at or beyond the range threshold
    nothing = capped.score(np.full(LASER.n_beams, LASER.range_threshold), [truth], LASER)[0]
    assert nothing["n_kept"] == LASER.n_beams and nothing["n_hit"] == 0 and nothing["cost"] == 0 and nothing["score"] == 0.0
    # every end outside the window: the sensor far off the map
    away = np.array([m.offset[0] - 100.0, m.offset[1] - 100.0, 0.3])
    off = capped.score(sm.query, [away], LASER)[0]
    assert off["n_hit"] > 0 and off["n_inside"] == 0 and off["cost"] == off["n_hit"] * 1600 and off["score"] == 0.0
    same_score(off, rule.score(m.view, want, 40, LASER, sm.query, away))

    def refused(field, poses, t=0, laser=LASER, ranges=sm.query):
        with pytest.raises(capi.KartoHipError) as e:
            field.score(ranges, poses, laser, truncate_cells=t)
        assert e.value.code == capi.KH_ERR_INVALID_ARG
    refused(uncapped, [truth])                                 # neither a radius nor a truncation
    refused(capped, [truth], 1025)
    far = lc.circle(16, range_threshold=(2 ** 20 - 1) / m.view["scale"], max_range=1e9)
    refused(capped, [truth], 0, far, np.full(16, 2.0))
    # the poses kh_map_fit refuses, on the lattice they were made for
    case = next(c for c in FIT_CASES if c.name.startswith("all eight octants"))
    field = field_on(case.view, 6)
    good = case.poses[0]
    for pose in lc.REFUSED_POSES:
        assert rule.ml.fit_refused(case.view, case.laser, pose)
        refused(field, [good, pose], 0, case.laser, case.ranges)
    edge = (2.0 ** 30 / case.view["scale"], 0.0, 0.0)          # the last sensor cell that is taken: nothing of it lands in the window
    same_score(field.score(case.ranges, [good, edge], case.laser)[1], rule.score(case.view, rule.d2_separable(case.view, 6), 6, case.laser, case.ranges, edge))
    field.close()


# ---------------------------------------------------------------- refinement
def same_refined(got, want):
    assert np.array_equal(bits(got.pose), bits(want.pose)), (got, want)
    assert (got.cost_start, got.cost, got.n_hit, got.rounds, got.halvings, got.status) == (want.cost_start, want.cost, want.n_hit, want.rounds, want.halvings,
                                                                                          want.status), (got, want)


def test_refinement_equals_the_rule(small):
    sm, m, g, capped, uncapped, want = small
    truth = np.asarray(sm.true_pose, dtype=np.float64)
    edge = np.array([2.0 ** 30 / m.view["scale"] + m.view["anchor"][0] - 0.01, truth[1], 0.0])      # a fifth of a cell short of the last cell the lattice takes
    starts = np.array([truth + [0.12, -0.08, 0.015], truth, truth + [-0.2, 0.15, -0.03], edge])
    for kw in (dict(), dict(truncate_cells=6), dict(max_rounds=2), dict(n_halvings=0, step_xy=0.05, step_heading=0.0)):
        got, times = capped.refine(sm.query, starts, LASER, **kw)
        rules = rule.refine(m.view, want, 40, LASER, sm.query, starts, **kw)
        for a, b in zip(got, rules):
            same_refined(a, b)
        assert times[1] >= times[0] > 0
        print(kw, [(r.status, r.rounds, r.cost_start, r.cost) for r in got], times)
        assert got[3].status == rule.LEFT_LATTICE and got[3].rounds == 0 and got[3].cost == got[3].n_hit * (36 if kw.get("truncate_cells") else 1600)
        if kw.get("max_rounds") == 2:
            assert got[0].status == rule.MAX_ROUNDS and got[0].rounds == 2
        else:
            assert got[0].status == rule.CONVERGED and got[0].cost < got[0].cost_start
    with pytest.raises(capi.KartoHipError) as e:
        uncapped.refine(sm.query, starts[:1], LASER)
    assert e.value.code == capi.KH_ERR_INVALID_ARG
    with pytest.raises(capi.KartoHipError) as e:
        capped.refine(sm.query, [truth, [np.nan, 0.0, 0.0]], LASER)
    assert e.value.code == capi.KH_ERR_INVALID_ARG


def test_the_localizer_wraps_the_same_calls(small):
    from slam_toolbox_amd.map_localizer import MapLocalizer
    from test_map_localize_gpu import PARAMS
    sm, m, g, capped, uncapped, want = small
    loc = MapLocalizer(PARAMS, LASER, max_batch=2)
    with pytest.raises(capi.KartoHipError) as e:
        loc.field()
    assert e.value.code == capi.KH_ERR_NOT_FOUND
    loc.set_map(g)
    field = loc.field(max_distance=2.0)
    same_field(field, want, m.view, 40)
    start = np.asarray(sm.true_pose, dtype=np.float64) + [0.12, -0.08, 0.015]
    wanted = rule.refine(m.view, want, 40, LASER, sm.query, [start], truncate_cells=6)[0]
    same_refined(loc.refine(sm.query, start, field=field, truncate_cells=6)[0][0], wanted)
    same_refined(loc.refine(sm.query, start, truncate_cells=6)[0][0], wanted)
    field.close()
    loc.close()


# ---------------------------------------------------------------- any view, and the snapshot
def test_views_from_a_merge_and_from_a_change_layer(kartohip_lib, oracle_lib):
    import map_match_rule as mr
    from slam_toolbox_amd.map_changes import MapChanges
    from slam_toolbox_amd.map_merge import MapMerge
    rng = np.random.default_rng(5)
    a = lc.view_of(lc.random_cells(rng, 20, 31), cases.A, cases.K, -4, 3)
    b = lc.view_of(lc.random_cells(rng, 25, 18), cases.A, cases.K, 2, -6)
    da, db = DeviceView(a), DeviceView(b)
    merged = MapMerge(da.v, db.v, (0.3, 0.2, 0.5))
    st = merged.stats
    mview = mr.view_dict(merged.cells(), cases.A, cases.K, st["ox"], st["oy"], st["width"])
    f = MapField(merged, max_distance=1.0)
    same_field(f, rule.d2_brute(mview, 4), mview, 4)
    f.close()
    layer = MapChanges(da.v)
    layer.observe(lc.circle(64), np.full(64, 1.3), [1.0, 2.5, 0.2])
    layer.diff(min_pass_through=0)
    pview = mr.view_dict(layer.read()["patched"], cases.A, cases.K, a["ox"], a["oy"], a["width"])
    f = MapField(layer, max_distance=0.0, obstacles="not_free")
    same_field(f, rule.d2_brute(pview, 0, rule.NOT_FREE), pview, 0)
    f.close()
    layer.close(); merged.close()
    da.close(); db.close()


def test_the_field_is_a_snapshot(kartohip_lib):
    """the source changes, then goes: the field and its readers answer as before"""
    case = next(c for c in FIELD_CASES if c.name == "40 x 50 random, p_occ 0.02, seed 3, R 11")
    d = DeviceView(case.view)
    got = MapField(d.v, max_distance=case.radius / case.view["scale"])
    want = rule.d2_brute(case.view, case.radius)
    other = np.full_like(case.view["cells"], 100)
    capi.check(capi.lib().kh_device_upload(d.buf, other.ctypes.data, other.size), "kh_device_upload")
    same_field(got, want, case.view, case.radius)
    d.close()
    same_field(got, want, case.view, case.radius)
    assert np.array_equal(got.costs(), rule.costs(case.view, want, case.radius))
    assert (got.costs() == 254).sum() == rule.stats(want)["n_obstacles"], "the states are the snapshot's too"
    got.close()
