"""GPU: the footprint analysis (kh_map_footprint_*, MapFootprint; csrc/occupancy_footprint.hip) against tests/map_footprint_rule.py on
the hand-made views of tests/map_footprint_cases.py, uploaded through kh_device_upload, and on the small map.  Every value a kernel
produces is an integer and is compared exactly: records, masks, summaries."""
import math

import numpy as np
import pytest

import map_field_rule as fr
import map_footprint_cases as cases
import map_footprint_rule as rule
import map_localize_cases as lc
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_field import MapField
from slam_toolbox_amd.map_footprint import FOOTPRINT_DTYPE, MapFootprint
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

POSE_CASES = cases.pose_cases()
LAYER_CASES = cases.layer_cases()


def field_on(view, radius, obstacles=fr.OCCUPIED):
    d = DeviceView(view)
    field = MapField(d.v, max_distance=radius / view["scale"], obstacles=obstacles)
    d.close()                                                  # the field is a snapshot: the view's memory may go
    return field


def same_records(got, want, where=""):
    assert got.dtype == FOOTPRINT_DTYPE == rule.DTYPE and got.shape == want.shape, where
    for k in rule.FIELDS:
        assert np.array_equal(got[k], want[k]), (where, k, got[k].tolist(), want[k].tolist())


@pytest.mark.parametrize("case", POSE_CASES, ids=[c.name for c in POSE_CASES])
def test_pose_cases(kartohip_lib, case):
    field = field_on(case.view, case.radius, case.obstacles)
    d2 = field.d2
    assert np.array_equal(d2, cases.field_values(case))
    fp = MapFootprint(field, case.verts)
    field.close()                                              # the handle never borrows the field
    want = rule.check(case.view, d2, case.verts, case.poses)
    same_records(fp.check(case.poses), want, case.name)
    assert np.all(want["n_cells"] == want["n_free"] + want["n_occupied"] + want["n_unknown"] + want["n_outside"])
    st = fp.stats
    assert st["reach"] == rule.create_check(case.verts, case.view["scale"]) and st["n_vertices"] == len(case.verts)
    assert (st["ox"], st["oy"], st["width"], st["height"]) == tuple(case.view[k] for k in ("ox", "oy", "width", "height"))
    assert st["times_ms"][0] > 0 and st["times_ms"][2] > 0
    fp.close()


def test_the_rectangle_s_hand_values_and_a_wall_inside_a_corner(kartohip_lib):
    cells = np.full((40, 60), lc.F, dtype=np.uint8)
    view = lc.view_of(cells, (0.0, 0.0), 20.0, -30, -20)
    # a wall on the first corner's vertex cell of the 30-degree rectangle; the 0-degree one (columns -10 .. 10, rows -6 .. 6) misses it
    corner = rule.pose_cells(cases.RECTANGLE, (0.0, 0.0, math.radians(30)), (0.0, 0.0), 20.0)[0]
    view["cells"][corner[1] + 20, corner[0] + 30] = lc.O
    field = field_on(view, 40)
    fp = field.footprint(cases.RECTANGLE)
    poses = [(0.0, 0.0, math.radians(a)) for a in (0, 30, 45, 90)]
    got = fp.check(poses)
    same_records(got, rule.check(view, field.d2, cases.RECTANGLE, poses))
    assert got["n_cells"].tolist() == [273, 269, 247, 273]
    assert got["status"].tolist()[:2] == [rule.FREE, rule.COLLISION] and got["n_occupied"][1] == 1 and got["min_d2"][1] == 0 and got["min_d2"][0] > 0
    fp.close(); field.close()


@pytest.mark.parametrize("n", (1, 3, 4, 5, 257))
def test_pose_counts_around_the_workgroup_s_four_waves(kartohip_lib, n):
    case = POSE_CASES[6]
    assert case.name.startswith("65 x 17, the rectangle")
    field = field_on(case.view, case.radius)
    fp = MapFootprint(field, case.verts)
    rng = np.random.default_rng(n)
    v = case.view
    poses = np.stack([rng.uniform(-0.6, 3.2, n), rng.uniform(-0.6, 0.8, n), rng.uniform(-4.0, 4.0, n)], axis=1)
    if n >= 3:
        poses[2] = poses[0]                                    # the same pose twice in one call
    want = rule.check(v, field.d2, case.verts, poses)
    same_records(fp.check(poses), want, n)
    fp.close(); field.close()


def test_poses_on_the_lattice_s_edge_and_refusals(kartohip_lib):
    view = cases.random_view(7, 5, 9, 4.0)
    field = field_on(view, 2)
    fp = MapFootprint(field, cases.ONE_CELL)
    poses = cases.lattice_poses(view) + [cases.world(view, 2, 2) + (0.0,)]
    want = rule.check(view, field.d2, cases.ONE_CELL, poses)
    assert want["status"].tolist()[:8] == [rule.OUTSIDE, rule.LATTICE] * 4 and want["status"].tolist()[8:10] == [rule.LATTICE] * 2
    same_records(fp.check(poses), want)
    L = capi.lib()
    out = np.zeros(4, dtype=FOOTPRINT_DTYPE)
    xy = np.zeros((4, 3))
    assert L.kh_map_footprint_check(fp._h, 0, xy.ctypes.data, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_footprint_check(fp._h, 65537, xy.ctypes.data, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_footprint_check(fp._h, 4, None, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_footprint_check(fp._h, 4, xy.ctypes.data, None) == capi.KH_ERR_INVALID_ARG
    xy[3, 2] = np.inf
    assert L.kh_map_footprint_check(fp._h, 4, xy.ctypes.data, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_footprint_check(None, 3, xy.ctypes.data, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    for verts in (cases.DIAMOND_255, [(63.75, 0.0), (0.0, 63.5), (-63.5, 0.0), (0.0, -63.5)]):      # reach 255 is taken, 256 refused
        try:
            MapFootprint(field, verts).close()
            assert verts is cases.DIAMOND_255
        except capi.KartoHipError as e:
            assert e.code == capi.KH_ERR_INVALID_ARG and verts is not cases.DIAMOND_255
    fp.close(); field.close()


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c.name for c in LAYER_CASES])
def test_layer_cases(kartohip_lib, case):
    field = field_on(case.view, 2)
    fp = MapFootprint(field, case.verts)
    field.close()
    want_masks, want = rule.layer(case.view, case.verts, case.n_headings, case.max_status)
    masks, got = fp.layer(case.n_headings, case.max_status)
    assert masks.dtype == np.uint32 and masks.shape == want_masks.shape
    assert np.array_equal(masks, want_masks), (case.name, f"{int((masks != want_masks).sum())} masks differ")
    assert np.array_equal(got["n_fit"], want["n_fit"]) and got["n_any"] == want["n_any"] and got["n_all"] == want["n_all"], case.name
    none, again = fp.layer(case.n_headings, case.max_status, masks=False)
    assert none is None and np.array_equal(again["n_fit"], want["n_fit"]) and again["n_all"] == want["n_all"], "the masks may be NULL"
    L = capi.lib()
    assert L.kh_map_footprint_layer(fp._h, case.n_headings, case.max_status, masks.ctypes.data, None) == capi.KH_OK, "the summary may be NULL"
    assert np.array_equal(masks, want_masks)
    assert fp.stats["layer_rows"] > 0 and fp.stats["times_ms"][1] > 0
    fp.close()


def test_the_layer_s_refusals(kartohip_lib):
    view = cases.random_view(8, 6, 9, 4.0)
    field = field_on(view, 2)
    fp = MapFootprint(field, cases.LONG_64)
    L = capi.lib()
    for h, ms in ((0, 0), (33, 0), (1, -1), (1, 3)):
        assert L.kh_map_footprint_layer(fp._h, h, ms, None, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_footprint_layer(fp._h, 2, 0, None, None) == capi.KH_OK
    far = MapFootprint(field, [(16.0, 1.0), (-15.7, 1.0), (-15.7, -1.0), (16.0, -1.0)])          # reach 66
    assert far.stats["reach"] > capi.KH_FOOTPRINT_LAYER_REACH
    assert L.kh_map_footprint_layer(far._h, 2, 0, None, None) == capi.KH_ERR_INVALID_ARG
    same_records(far.check([(0.0, 0.0, 0.3)]), rule.check(view, field.d2, far.vertices.tolist(), [(0.0, 0.0, 0.3)]), "a pose check has no such limit")
    for h in (far, fp, field):
        h.close()


def test_recompute_after_an_update_equals_a_fresh_handle_and_two_handles_side_by_side(kartohip_lib):
    first, second = cases.random_view(9, 17, 65, 20.0, -7, -3), cases.random_view(10, 17, 65, 20.0, -7, -3, p_free=0.5, p_occ=0.2)
    d = DeviceView(first)
    field = MapField(d.v, max_distance=0.4)
    fp, other = MapFootprint(field, cases.RECTANGLE), MapFootprint(field, cases.TRIANGLE)
    poses = cases.edge_poses(first)
    before = fp.check(poses)
    same_records(before, rule.check(first, field.d2, cases.RECTANGLE, poses), "before")
    d.upload(second)
    field.update(d.v)
    same_records(fp.check(poses), before, "the handle keeps its snapshot")
    fp.recompute(field)
    fresh = MapFootprint(field, cases.RECTANGLE)
    want = rule.check(second, field.d2, cases.RECTANGLE, poses)
    same_records(fp.check(poses), want, "recomputed")
    same_records(fresh.check(poses), want, "fresh")
    same_records(other.check(poses), rule.check(first, fr.d2_brute(first, 8), cases.TRIANGLE, poses), "the other handle still holds the first map")
    m1, s1 = fp.layer(7, 1)
    m2, s2 = fresh.layer(7, 1)
    assert np.array_equal(m1, m2) and np.array_equal(m1, rule.layer(second, cases.RECTANGLE, 7, 1)[0]) and s1["n_any"] == s2["n_any"]
    # a field on another lattice is refused, and the snapshot stands
    o = DeviceView(lc.view_of(np.full((4, 4), lc.F, dtype=np.uint8), cases.A, 40.0))
    elsewhere = MapField(o.v, max_distance=1.0)
    L = capi.lib()
    assert L.kh_map_footprint_recompute(fp._h, elsewhere._h) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_footprint_recompute(fp._h, None) == capi.KH_ERR_INVALID_ARG
    same_records(fp.check(poses), want, "after the refusals")
    for h in (elsewhere, fresh, other, fp, field):
        h.close()
    o.close(); d.close()


def test_check_path_on_a_travel_path_of_the_small_map(kartohip_lib, oracle_lib):
    from common import LASER
    from slam_toolbox_amd.map_localizer import MapLocalizer
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    from test_map_localize_gpu import PARAMS
    sm, m = lc.small_map()
    g = OccupancyGrid.from_nav(m.nav, m.offset, lc.RESOLUTION)
    field = MapField(g, max_distance=2.0)
    travel = field.travel(goal_snap_cells=2)
    poses = np.asarray(sm.poses)[:, :2]
    travel.solve(poses[:1])
    path = travel.paths(poses[-1:], 2, 4096)[0]
    assert path.status == capi.KH_TRAVEL_PATH_OK and len(path.xy) > 10
    d2 = field.d2
    verts = rule.rectangle(1.0, 0.6)
    fp = field.footprint(verts)
    for level in (capi.KH_FOOTPRINT_COLLISION, capi.KH_FOOTPRINT_UNKNOWN):
        records, first = fp.check_path(path.xy, level)
        want, want_first = rule.check_path(m.view, d2, verts, path.xy, level)
        same_records(records, want, level)
        assert first == want_first
    loc = MapLocalizer(PARAMS, LASER, max_batch=2).set_map(g)
    through = loc.footprint(verts, max_distance=2.0)
    same_records(through.check_path(path.xy)[0], want, "through the localizer")
    print(f"{m.width} x {m.height}: a path of {len(path.xy)} cells, first blocked {want_first}; {fp.stats}")
    for h in (through, loc, fp, travel, field, g):
        h.close()
