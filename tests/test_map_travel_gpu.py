"""GPU: the travel costs (kh_map_travel_*, MapTravel; csrc/occupancy_travel.hip) against tests/map_travel_rule.py on the hand-made
views of tests/map_travel_cases.py, uploaded through kh_device_upload, and on the small map.  Every value a kernel produces is an
integer and is compared exactly: values, weights, goal statuses, the stats' counts, lookup triples, path heads and cells."""
import ctypes as C

import numpy as np
import pytest

import map_field_rule as fr
import map_localize_cases as lc
import map_regions_rule as regions_rule
import map_travel_cases as cases
import map_travel_rule as rule
from common import bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_field import MapField
from slam_toolbox_amd.map_travel import MapTravel
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

CASES = cases.travel_cases()
BY_NAME = {c.name: c for c in CASES}
COUNTS = ("ox", "oy", "width", "height", "clearance_cells", "inflation_cells", "connectivity", "n_traversable", "n_reached", "max_value")
_wanted = {}


def wanted(case):
    if case.name not in _wanted:
        _wanted[case.name] = rule.analyse(case.view, cases.field_values(case), case.radius, case.goals, **case.params)
    return _wanted[case.name]


def field_on(view, radius):
    d = DeviceView(view)
    field = MapField(d.v, max_distance=radius / view["scale"])
    d.close()                                                  # the field is a snapshot: the view's memory may go
    return field


def same_solution(got, status, want, where=""):
    """a solved MapTravel and its goal statuses against the rule's dict"""
    assert np.array_equal(status, want["goal_status"]), (where, "goal statuses")
    values, weights = got.values, got.weights
    assert values.dtype == np.uint32 and weights.dtype == np.uint16 and values.shape == want["values"].shape == weights.shape, where
    assert np.array_equal(weights, want["weights"]), (where, f"{int((weights != want['weights']).sum())} weights differ")
    assert np.array_equal(values, want["values"]), (where, f"{int((values != want['values']).sum())} values differ")
    for k in COUNTS:
        assert got.stats[k] == want["stats"][k], (where, k, got.stats[k], want["stats"][k])


def same_lookup(got, view, values, xy, snap, where=""):
    status, value, cell = got.lookup(xy, snap)
    want_s, want_v, want_c = rule.lookup(view, values, xy, snap)
    assert np.array_equal(status, want_s) and np.array_equal(value, want_v) and np.array_equal(cell, want_c), (where, snap)
    return want_s


def same_paths(got, view, want, xy, snap, max_cells, where=""):
    p = want["params"]
    paths = got.paths(xy, snap, max_cells)
    wanted_paths = rule.paths(view, want["values"], want["weights"], xy, snap, max_cells, p["connectivity"], p["cut_corners"])
    assert len(paths) == len(wanted_paths) == len(np.asarray(xy).reshape(-1, 2))
    for k, (g, w) in enumerate(zip(paths, wanted_paths)):
        assert (g.status, g.cost, g.start_cell, len(g.cells)) == (w["status"], w["cost"], w["start_cell"], w["n_cells"]), (where, k)
        assert np.array_equal(g.cells, w["cells"]), (where, k)
        assert np.array_equal(bits(g.xy), bits(rule.cell_world(view, w["cells"]))), (where, k, "world points")
    return wanted_paths


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_travel_cases(kartohip_lib, case):
    field = field_on(case.view, case.radius)
    got = MapTravel(field, **case.params)
    field.close()                                              # the handle never borrows the field
    with pytest.raises(capi.KartoHipError) as e:
        got.values                                             # no solve yet
    assert e.value.code == capi.KH_ERR_NOT_FOUND
    want = wanted(case)
    assert got.stats["n_traversable"] == want["stats"]["n_traversable"] and got.stats["n_reached"] == 0
    status = got.solve(case.goals)
    same_solution(got, status, want, case.name)
    t = got.stats["times_ms"]
    assert t[0] > 0 and t[1] > 0 and t[3] > 0 and (t[2] > 0) == (got.stats["launches"] > 0) == bool((status == rule.GOAL_OK).any())
    assert got.stats["rounds"] <= got.stats["launches"] and got.stats["tile_runs"] >= got.stats["rounds"]
    small = case.view["width"] * case.view["height"] <= 130 * 50
    pts = cases.lookup_points(case.view)
    for snap in (0, 1, 16) if small else (1,):
        same_lookup(got, case.view, want["values"], pts, snap, case.name)
    same_paths(got, case.view, want, case.starts, 1, 4096 if small else 65536, case.name)
    got.close()


def test_all_occupied_blocks_every_goal(kartohip_lib):
    case = BY_NAME["70 x 20 all occupied, N8"]
    field = field_on(case.view, 0)
    got = MapTravel(field, **case.params)
    status = got.solve(case.goals)
    assert status.tolist() == [rule.GOAL_BLOCKED] * 3 and np.all(got.values == capi.KH_TRAVEL_FAR) and np.all(got.weights == 0)
    assert got.stats["launches"] == 0 and got.stats["n_reached"] == 0 and got.stats["max_value"] == 0
    got.close(); field.close()


def test_lookups_of_one_and_of_257_points_and_null_outputs(kartohip_lib):
    for name in ("40 x 50 random, p_occ 0.4, seed 2, 3 goals, N8", "40 x 50 random, p_occ 0.1, seed 3, 4096 goals, N4"):
        case = BY_NAME[name]
        field = field_on(case.view, case.radius)
        got = MapTravel(field, **case.params)
        got.solve(case.goals)
        want = wanted(case)
        pts = cases.lookup_points(case.view)
        many = np.concatenate([pts, np.random.default_rng(9).uniform(-14.0, 14.0, size=(257 - len(pts), 2))])
        assert len(many) == 257
        codes = set()
        for xy in (pts[:1], many):
            for snap in (0, 1, 16):
                codes |= set(same_lookup(got, case.view, want["values"], xy, snap, name).tolist())
        assert codes == {rule.AT_OK, rule.AT_UNREACHED, rule.AT_OUTSIDE}
        L = capi.lib()
        value = np.zeros(len(pts), dtype=np.uint32)
        assert L.kh_map_travel_lookup(got._h, len(pts), pts.ctypes.data, 1, None, value.ctypes.data, None) == capi.KH_OK, "any output may be NULL"
        assert np.array_equal(value, rule.lookup(case.view, want["values"], pts, 1)[1])
        bad = pts.copy()
        bad[3, 1] = np.nan
        assert L.kh_map_travel_lookup(got._h, len(bad), bad.ctypes.data, 0, None, value.ctypes.data, None) == capi.KH_ERR_INVALID_ARG
        assert L.kh_map_travel_lookup(got._h, len(pts), pts.ctypes.data, 17, None, value.ctypes.data, None) == capi.KH_ERR_INVALID_ARG
        got.close(); field.close()


def test_paths_truncated_unreached_outside_and_of_65_starts(kartohip_lib):
    case = BY_NAME["130 x 50 serpentine, the goal at one end, N8"]
    field = field_on(case.view, case.radius)
    got = MapTravel(field, **case.params)
    got.solve(case.goals)
    want = wanted(case)
    v = case.view
    far_end = [cases.world(v, 129, 48)]                         # the other end of the corridor: 25 rows of 130 cells and 24 gaps
    whole = same_paths(got, v, want, far_end, 0, 65536, "whole")[0]
    assert whole["status"] == rule.PATH_OK and whole["n_cells"] == 25 * 130 + 24
    assert same_paths(got, v, want, far_end, 0, 1, "one cell")[0]["status"] == rule.PATH_TRUNCATED
    assert same_paths(got, v, want, far_end, 0, whole["n_cells"] - 1, "one short")[0]["status"] == rule.PATH_TRUNCATED
    assert same_paths(got, v, want, far_end, 0, whole["n_cells"], "its exact length")[0]["status"] == rule.PATH_OK
    assert same_paths(got, v, want, [cases.world(v, 0, 0)], 0, 1, "from the goal")[0]["status"] == rule.PATH_OK
    mixed = [cases.world(v, 5, 1), cases.world(v, -1, 0), cases.world(v, 7, 4)]      # a wall, outside, the corridor
    got_codes = [p["status"] for p in same_paths(got, v, want, mixed, 0, 4096, "codes")]
    assert got_codes == [rule.PATH_UNREACHED, rule.PATH_OUTSIDE, rule.PATH_OK]
    assert same_paths(got, v, want, mixed[:1], 1, 4096, "snapped off the wall")[0]["status"] == rule.PATH_OK
    rng = np.random.default_rng(3)
    many = np.array([cases.world(v, int(i), int(j)) for i, j in zip(rng.integers(-2, 132, 65), rng.integers(-2, 52, 65))])
    codes = {p["status"] for p in same_paths(got, v, want, many, 0, 700, "65 starts")}
    assert codes == {rule.PATH_OK, rule.PATH_TRUNCATED, rule.PATH_UNREACHED, rule.PATH_OUTSIDE}
    L = capi.lib()
    heads = (capi.KhTravelPath * 65)()
    assert L.kh_map_travel_paths(got._h, 65, many.ctypes.data, 0, 700, heads, None) == capi.KH_OK, "the cells may be NULL"
    assert [h.n_cells for h in heads] == [p["n_cells"] for p in rule.paths(v, want["values"], want["weights"], many, 0, 700, 8, 0)]
    got.close(); field.close()


def test_rounds_per_check_does_not_show_and_solves_repeat(kartohip_lib):
    for name in ("130 x 50 serpentine, the goal at one end, N8", "129 x 33 mixed, N4", "40 x 50 random, p_occ 0.4, seed 1, 3 goals, N8, cut 1"):
        case = BY_NAME[name]
        field = field_on(case.view, case.radius)
        d2, costs = field.d2, field.costs()
        got = MapTravel(field, **case.params)
        blobs = {}
        for k in (1, 8, 0, 64):
            got.set_rounds_per_check(k)
            status = got.solve(case.goals)
            blobs[k] = (status.tobytes(), got.values.tobytes(), got.weights.tobytes())
            assert got.stats["launches"] % max(k, 1) == 0 and got.stats["launches"] >= got.stats["rounds"]
        assert blobs[1] == blobs[8] == blobs[0] == blobs[64], name
        same_solution(got, status, wanted(case), name)
        # other goals on the same handle, then the first again
        other = np.array([cases.world(case.view, case.view["width"] - 1, case.view["height"] - 1), cases.world(case.view, 2, 0)])
        status2 = got.solve(other)
        same_solution(got, status2, rule.analyse(case.view, cases.field_values(case), case.radius, other, **case.params), name + ", other goals")
        status = got.solve(case.goals)
        assert (status.tobytes(), got.values.tobytes(), got.weights.tobytes()) == blobs[1], "the first solve again"
        assert np.array_equal(field.d2, d2) and np.array_equal(field.costs(), costs), "the analysis wrote the field"
        got.close(); field.close()


def test_the_field_s_reach_is_checked(kartohip_lib):
    view = lc.view_of(cases.two_rooms(), cases.A, cases.K)
    field = field_on(view, 2)                                   # R = 2; the default inflation reaches Rt = 3 cells at this scale
    for kw in (dict(min_clearance=3 / cases.K, cost_weight=0), dict(), dict(cost_weight=1), dict(connectivity=6), dict(neutral_cost=0), dict(goal_snap_cells=17),
               dict(min_clearance=float("nan")), dict(inflation_radius=-1.0), dict(cut_corners=2), dict(cost_weight=256)):
        with pytest.raises(capi.KartoHipError) as e:
            MapTravel(field, **kw)
        assert e.value.code == capi.KH_ERR_INVALID_ARG, kw
    case = BY_NAME["two rooms, a field of R 2 below Rt 3 with cost_weight 0, N8"]
    got = MapTravel(field, **case.params)                       # with cost_weight 0 Rt is not checked against the field
    same_solution(got, got.solve(case.goals), wanted(case), case.name)
    assert got.stats["inflation_cells"] == 3
    near = MapTravel(field, min_clearance=2 / cases.K, inflation_radius=0.5)      # Rc == R and Rt == R are taken
    goal = [cases.world(view, 5, 5)]
    same_solution(near, near.solve(goal), rule.analyse(view, fr.d2_brute(view, 2), 2, goal, min_clearance=2 / cases.K, inflation_radius=0.5), "Rc == Rt == R")
    for h in (near, got, field):
        h.close()


def test_recompute_after_a_door_opens_and_another_lattice(kartohip_lib):
    shut, door = lc.view_of(cases.two_rooms(door=0), cases.A, cases.K), lc.view_of(cases.two_rooms(door=3), cases.A, cases.K)
    goal = [cases.world(shut, 5, 5)]
    d = DeviceView(shut)
    field = MapField(d.v, max_distance=8 / cases.K)
    got = MapTravel(field, min_clearance=1 / cases.K)
    status = got.solve(goal)
    want = rule.analyse(shut, fr.d2_brute(shut, 8), 8, goal, min_clearance=1 / cases.K)
    same_solution(got, status, want, "shut")
    assert np.all(got.values[1:21, 32:64] == capi.KH_TRAVEL_FAR)
    d.upload(door)
    field.update(d.v)
    got.recompute(field)
    L = capi.lib()
    xy = np.array(goal, dtype=np.float64)
    heads = (capi.KhTravelPath * 1)()
    assert L.kh_map_travel_read(got._h, None, None) == capi.KH_ERR_NOT_FOUND, "a recompute drops the solution"
    assert L.kh_map_travel_lookup(got._h, 1, xy.ctypes.data, 0, None, None, None) == capi.KH_ERR_NOT_FOUND
    assert L.kh_map_travel_paths(got._h, 1, xy.ctypes.data, 0, 8, heads, None) == capi.KH_ERR_NOT_FOUND
    assert got.stats["n_reached"] == 0
    status = got.solve(goal)
    want = rule.analyse(door, fr.d2_brute(door, 8), 8, goal, min_clearance=1 / cases.K)
    same_solution(got, status, want, "the door is open")
    assert np.all(got.values[3:19, 34:62] != capi.KH_TRAVEL_FAR), "the other room is reached"
    d.close()
    # another window of the same lattice: the arrays are made anew
    case = BY_NAME["129 x 33 comb, the teeth join in the last row of the last tile, N8"]
    e = DeviceView(case.view)
    field.update(e.v)
    got.recompute(field)
    status = got.solve(case.goals)
    same_solution(got, status, rule.analyse(case.view, fr.d2_brute(case.view, 8), 8, case.goals, min_clearance=1 / cases.K), "after a window change")
    before = got.values
    # a field on another lattice is refused, and the solution stands
    other = lc.view_of(cases.two_rooms(), cases.A, 2 * cases.K)
    o = DeviceView(other)
    elsewhere = MapField(o.v, max_distance=1.0)
    assert L.kh_map_travel_recompute(got._h, elsewhere._h) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_travel_recompute(got._h, None) == capi.KH_ERR_INVALID_ARG
    assert np.array_equal(got.values, before)
    for h in (elsewhere, got, field):
        h.close()
    o.close(); e.close()


def test_the_localizer_s_wrapper(kartohip_lib):
    """MapLocalizer.travel makes a field that reaches max(Rc, Rt) for the call; the analysis outlives it"""
    from common import LASER
    from slam_toolbox_amd.map_localizer import MapLocalizer
    from test_map_localize_gpu import PARAMS
    case = BY_NAME["two rooms and a door of 2 cells, Rc 2, N8"]
    d = DeviceView(case.view)
    loc = MapLocalizer(PARAMS, LASER, max_batch=2).set_map(d.v)
    got = loc.travel(max_distance=8 / cases.K, **case.params)
    same_solution(got, got.solve(case.goals), wanted(case), "through the localizer")
    far = loc.travel(max_distance=0.25, min_clearance=3.0, inflation_radius=4.0, connectivity=8)      # the field is made to reach 16 cells
    assert far.stats["clearance_cells"] == 12 and far.stats["inflation_cells"] == 16 and far.stats["n_traversable"] == 0
    for h in (far, got, loc):
        h.close()
    d.close()


@pytest.fixture(scope="module")
def small(kartohip_lib, oracle_lib):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    sm, m = lc.small_map()
    g = OccupancyGrid.from_nav(m.nav, m.offset, lc.RESOLUTION)
    field = MapField(g, max_distance=2.0)
    yield sm, m, field, fr.d2_separable(m.view, 40)
    field.close(); g.close()


@pytest.mark.parametrize("rc", (0, 3))
def test_the_small_map(small, rc):
    sm, m, field, d2 = small
    poses = np.asarray(sm.poses)[:, :2]
    clearance = cases.rcases.clearance_of(rc, m.view["scale"])
    for conn in (4, 8):
        kw = dict(min_clearance=clearance, connectivity=conn, goal_snap_cells=2)
        got = field.travel(**kw)
        status = got.solve(poses[:1])
        want = rule.analyse(m.view, d2, 40, poses[:1], **kw)
        same_solution(got, status, want, f"Rc {rc}, N{conn}")
        assert status.tolist() == [rule.GOAL_OK] and got.stats["clearance_cells"] == rc
        paths = same_paths(got, m.view, want, poses, 2, 4096, f"Rc {rc}, N{conn}")
        assert all(p["status"] == rule.PATH_OK for p in paths), "all eight poses are reached"
        regions = field.regions(min_clearance=clearance, connectivity=conn)
        clusters = regions.frontiers
        order = got.rank(clusters, 1)
        assert [(k, v) for k, v, _ in order] == rule.rank(m.view, want["values"], clusters, 1) and len(order) == len(clusters) > 1
        assert any(v is not None for _, v, _ in order)
        if conn == 4:
            ids = regions.region_ids
            _, _, cell = got.lookup(poses[:1], 2)
            mine = ids[cell[0, 1] - m.view["oy"], cell[0, 0] - m.view["ox"]]
            assert mine < regions_rule.DROPPED and np.array_equal(got.values != capi.KH_TRAVEL_FAR, ids == mine), "the reached mask is the goal's region"
        print(f"{m.width} x {m.height}, Rc {rc}, N{conn}: {got.stats}")
        regions.close(); got.close()
