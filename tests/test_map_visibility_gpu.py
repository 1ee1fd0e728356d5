"""GPU: kh_map_visibility_* (k_vis_gain, k_vis_best in csrc/occupancy_visibility.hip; the handle in csrc/map_visibility.cpp) against
tests/map_visibility_rule.py on the hand-made views of tests/map_visibility_cases.py, uploaded through kh_device_upload, and on the
small map.  Records, masks, picks and pick gains are integers no execution order shows in: every comparison is exact."""
import numpy as np
import pytest

import map_localize_cases as lc
import map_raycast_rule as rr
import map_visibility_cases as cases
import map_visibility_rule as rule
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_localizer import MapLocalizer, map_raycast
from slam_toolbox_amd.map_visibility import MapVisibility
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

VIS_CASES = cases.vis_cases()
SELECT_CASES = cases.select_cases()
BY_NAME = {c.name: c for c in VIS_CASES}


def same_records(got, want, where=""):
    assert got.shape == want.shape, where
    for f in rule.FIELDS:
        assert np.array_equal(got[f], want[f]), (where, f, got[f].tolist(), want[f].tolist())


@pytest.mark.parametrize("case", VIS_CASES, ids=[c.name for c in VIS_CASES])
def test_vis_cases(kartohip_lib, oracle_lib, case):
    """gain from a cleared mask, commit of every second pose in one call, gain after the commit, the mask, clear"""
    d = DeviceView(case.view)
    got, want = MapVisibility(d.v, case.laser, **case.params), rule.Visibility(case.view, case.laser, **case.params)
    st = got.stats
    assert st["reach"] == want.reach and st["bitmap_bytes"] == rule.bitmap_bytes(want.reach) and (st["width"], st["height"]) == (case.view["width"], case.view["height"])
    assert not got.mask.any()
    same_records(got.gain(case.poses), want.gain(case.poses), "from a cleared mask")
    assert got.stats["n_poses"] == len(case.poses) and got.stats["launches"] == 1 and got.kernel_ms > 0
    got.commit(case.poses[::2]); want.commit(case.poses[::2])
    assert np.array_equal(got.mask, want.mask)
    same_records(got.gain(case.poses), want.gain(case.poses), "after the commit")
    got.set_skip(False)
    same_records(got.gain(case.poses), want.gain(case.poses), "with every OR made")
    got.clear()
    assert not got.mask.any()
    got.commit(case.poses)
    want.clear(); want.commit(case.poses)
    assert np.array_equal(got.mask, want.mask), "committed with every OR made"
    assert np.array_equal(d.download(), case.view["cells"].ravel()), "the view's cells were written"
    got.close(); d.close()


def test_commit_of_one_and_of_seventy_poses_with_duplicates(kartohip_lib, oracle_lib):
    case = BY_NAME["64 beams, 2 poses, budget 20"]
    rng = np.random.default_rng(5)
    poses = np.stack([rng.uniform(-1.5, 14.5, 35), rng.uniform(0.0, 13.5, 35), rng.uniform(-3.0, 3.0, 35)], axis=1)
    poses = np.concatenate([poses, poses[::-1]])               # 70, every pose twice
    d = DeviceView(case.view)
    got, want = MapVisibility(d.v, case.laser, **case.params), rule.Visibility(case.view, case.laser, **case.params)
    got.commit(poses[:1]); want.commit(poses[:1])
    assert np.array_equal(got.mask, want.mask) and got.mask.any()
    got.commit(poses); want.commit(poses)
    assert np.array_equal(got.mask, want.mask) and got.stats["n_poses"] == 70
    same_records(got.gain(poses[:5]), want.gain(poses[:5]))
    assert (got.gain(poses)["gain"] == 0).all(), "nothing new where everything was committed"
    got.close(); d.close()


def test_set_map_keeps_the_mask_and_refuses_another_window(kartohip_lib, oracle_lib):
    closed, opened = cases.door_views()
    laser, left = lc.circle(128), [(2.5, 4.0, 0.0)]            # in the left room, the door to its right
    d = DeviceView(closed)
    got, want = MapVisibility(d.v, laser, max_unknown=5, w_free=1), rule.Visibility(closed, laser, max_unknown=5, w_free=1)
    got.commit(left); want.commit(left)
    behind = want.gain(left)[0]
    d.upload(opened)                                           # the map changed in place
    got.set_map(d.v); want.set_map(opened)
    assert np.array_equal(got.mask, want.mask) and got.mask.any(), "the mask is kept"
    now = got.gain(left)
    same_records(now, want.gain(left), "through the door")
    assert now[0]["seen_free"] > behind["seen_free"] and now[0]["new_free"] > 0 and behind["new_free"] == 0
    other = DeviceView(opened)                                 # another buffer, the same window: taken
    got.set_map(other.v)
    same_records(got.gain(left), now)
    for field, value in (("ox", closed["ox"] + 1), ("width", closed["width"] - 1), ("scale", 8.0)):
        w = capi.KhMapView.from_buffer_copy(other.v)
        setattr(w, field, value)
        with pytest.raises(capi.KartoHipError) as e:
            got.set_map(w)
        assert e.value.code == capi.KH_ERR_INVALID_ARG, field
    same_records(got.gain(left), now, "a refused view changes nothing")
    got.close(); other.close(); d.close()


@pytest.mark.parametrize("case", SELECT_CASES, ids=[c.name for c in SELECT_CASES])
def test_select_cases(kartohip_lib, oracle_lib, case):
    d = DeviceView(case.view)
    got, want = MapVisibility(d.v, case.laser, **case.params), rule.Visibility(case.view, case.laser, **case.params)
    if len(case.committed):
        got.commit(case.committed); want.commit(case.committed)
    picks, gains = got.select(case.poses, case.k, case.min_gain)
    want_picks, want_gains = want.select(case.poses, case.k, case.min_gain)
    assert picks.tolist() == want_picks.tolist() and gains.tolist() == want_gains.tolist(), case.name
    assert np.array_equal(got.mask, want.mask), "the mask is left holding the picks"
    st = got.stats
    assert st["rounds"] == len(picks) and st["launches"] == 3 * case.k and st["n_poses"] == len(case.poses)
    same_records(got.gain(case.poses[:3]), want.gain(case.poses[:3]), "after the select")
    assert np.array_equal(d.download(), case.view["cells"].ravel())
    got.close(); d.close()


def test_the_early_stop_and_the_tie(kartohip_lib, oracle_lib):
    by = {c.name: c for c in SELECT_CASES}
    stop, tie = by["an early stop: 5 candidates of 2 distinct poses, k 5"], by["a tie between two identical candidates"]
    d = DeviceView(stop.view)
    got = MapVisibility(d.v, stop.laser, **stop.params)
    picks, gains = got.select(stop.poses, stop.k, stop.min_gain)
    assert sorted(picks.tolist()) == [0, 2] and (gains > 0).all(), "two picks of five rounds: the copies add nothing"
    again, _ = got.select(stop.poses, 1, 1)
    assert len(again) == 0, "nothing is left to gain: no pick at all"
    big, _ = got.select(stop.poses, 1, 0xFFFFFFFF)
    assert len(big) == 0
    got.close()
    got = MapVisibility(d.v, tie.laser, **tie.params)
    alone = got.gain(tie.poses)["gain"]
    picks, _ = got.select(tie.poses, tie.k, tie.min_gain)
    assert alone[0] == alone[2] and alone[1] == alone[3] and picks[0] == (0 if alone[0] >= alone[1] else 1) and set(picks.tolist()) == {0, 1}
    got.close(); d.close()


def test_two_handles_on_one_view(kartohip_lib, oracle_lib):
    case = BY_NAME["65 beams, 5 poses, budget 20"]
    d = DeviceView(case.view)
    a, b = MapVisibility(d.v, case.laser, max_unknown=20), MapVisibility(d.v, case.laser, max_unknown=-1, w_unknown=0, w_occupied=7)
    wa, wb = rule.Visibility(case.view, case.laser, max_unknown=20), rule.Visibility(case.view, case.laser, max_unknown=-1, w_unknown=0, w_occupied=7)
    a.commit(case.poses[:2]); wa.commit(case.poses[:2])
    same_records(b.gain(case.poses), wb.gain(case.poses), "the other handle's mask is its own")
    same_records(a.gain(case.poses), wa.gain(case.poses))
    assert not b.mask.any() and np.array_equal(a.mask, wa.mask)
    a.close()
    same_records(b.gain(case.poses), wb.gain(case.poses), "after the first handle went")
    b.close(); d.close()


@pytest.fixture(scope="module")
def small(kartohip_lib, oracle_lib):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    sm, m = lc.small_map()
    g = OccupancyGrid.from_nav(m.nav, m.offset, lc.RESOLUTION)
    yield sm, m, g
    g.close()


def test_the_small_map_sees_the_walls_its_beams_hit(small):
    """1081 beams at 0.05 m through MapLocalizer.visibility: seen_occupied = the distinct HIT cells of the library's own cast"""
    from common import LASER
    from test_map_localize_gpu import PARAMS
    sm, m, g = small
    before = g.cells().copy()
    loc = MapLocalizer(PARAMS, LASER, max_batch=2).set_map(g)
    vis = loc.visibility(max_unknown=20)
    poses = np.asarray(sm.poses, dtype=np.float64)
    got = vis.gain(poses)
    cast = map_raycast(g.view(), LASER, poses, 20)
    for k in range(len(poses)):
        hits = {tuple(c) for c, code in zip(cast.cells[k].tolist(), cast.codes[k].tolist()) if code == capi.KH_RAY_HIT}
        assert got[k]["seen_occupied"] == len(hits) > 0
        assert (got[k]["beams_free"], got[k]["beams_hit"], got[k]["beams_unknown"]) == tuple(int((cast.codes[k] == c).sum()) for c in (rr.FREE, rr.HIT, rr.UNKNOWN))
    want = rule.Visibility(m.view, LASER, max_unknown=20)
    same_records(got[:2], want.gain(poses[:2]), "the rule at the first two poses")
    vis.commit(poses[:2]); want.commit(poses[:2])
    assert np.array_equal(vis.mask, want.mask)
    print(f"{m.width} x {m.height}, 8 poses of {LASER.n_beams} beams: {vis.stats}")
    assert np.array_equal(g.cells(), before), "kh_occupancy_read before and after: the cells were written"
    vis.close(); loc.close()


def test_candidates_from_the_regions_selected_against_the_rule(small):
    from slam_toolbox_amd.map_field import MapField
    sm, m, g = small
    field = MapField(g, max_distance=2.0)
    regions = field.regions(min_clearance=0.0)
    laser = lc.circle(64, range_threshold=4.0, max_range=7.5)
    poses = MapVisibility.candidates(regions, n_headings=2)
    frontiers = regions.frontiers
    assert len(poses) == 2 * len(frontiers) > 2 and np.array_equal(poses, rule.candidates(frontiers, 2)) and np.array_equal(poses, MapVisibility.candidates(frontiers, 2))
    assert poses[0, 2] == 0.0 and poses[1, 2] == np.pi and tuple(poses[2, :2]) == tuple(frontiers[1]["anchor_xy"])
    got, want = MapVisibility(g, laser), rule.Visibility(m.view, laser)
    picks, gains = got.select(poses, 3)
    want_picks, want_gains = want.select(poses, 3)
    assert picks.tolist() == want_picks.tolist() and gains.tolist() == want_gains.tolist() and len(picks) == 3
    assert np.array_equal(got.mask, want.mask)
    print(f"{len(poses)} candidates from {len(frontiers)} frontier clusters: picks {picks.tolist()}, gains {gains.tolist()}, {got.stats}")
    got.close(); regions.close(); field.close()
