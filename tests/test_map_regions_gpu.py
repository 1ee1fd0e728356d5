"""GPU: the region analysis (kh_map_regions_*, MapRegions; csrc/occupancy_regions.hip) against tests/map_regions_rule.py on the
hand-made views of tests/map_regions_cases.py, uploaded through kh_device_upload, and on the small map.  Every value a kernel
produces is an integer and is compared exactly -- id grids, every record field, the summary, lookup statuses and ids -- and the
doubles derived from them on the host bit for bit."""
import ctypes as C

import numpy as np
import pytest

import map_field_rule as fr
import map_localize_cases as lc
import map_regions_cases as cases
import map_regions_rule as rule
from common import bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_field import MapField
from slam_toolbox_amd.map_regions import MapRegions
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

CASES = cases.region_cases()
BY_NAME = {c.name: c for c in CASES}
INTEGERS = ("root", "n_cells", "box", "sum_i", "sum_j", "max_d2", "n_other", "link", "anchor_cell")


def same(got, want, where=""):
    """a MapRegions against the rule's dict, everything"""
    st = got.stats
    for k, v in want["stats"].items():
        assert st[k] == v, (where, k, st[k], v)
    for key in ("region_ids", "frontier_ids"):
        ids = getattr(got, key)
        assert ids.dtype == np.uint32 and ids.shape == want[key].shape, (where, key)
        assert np.array_equal(ids, want[key]), (where, key, f"{int((ids != want[key]).sum())} ids differ")
    for key in ("regions", "frontiers"):
        records = getattr(got, key)
        assert len(records) == len(want[key]), (where, key)
        for k, (g, w) in enumerate(zip(records, want[key])):
            for name in INTEGERS:
                assert g[name] == w[name], (where, key, k, name, g[name], w[name])
            for name in ("centroid", "anchor_xy"):
                assert np.array_equal(bits(np.array(g[name])), bits(np.array(w[name]))), (where, key, k, name)


def field_on(view, radius):
    d = DeviceView(view)
    field = MapField(d.v, max_distance=radius / view["scale"])
    d.close()                                                  # the field is a snapshot: the view's memory may go
    return field


def wanted(case, **params):
    return rule.analyse(case.view, cases.field_values(case), case.radius, **dict(case.params, **params))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_region_cases(kartohip_lib, case):
    field = field_on(case.view, case.radius)
    got = MapRegions(field, **case.params)
    field.close()                                              # the handle never borrows the field
    same(got, wanted(case), case.name)
    t = got.stats["times_ms"]
    assert all(v > 0 for v in t[:1] + t[2:]) and t[6] >= sum(t[:6]) - 1e-3
    got.close()


def test_cap_at_exactly_n_kept_and_one_below(kartohip_lib):
    case = BY_NAME["66 x 18 checkerboard, capped at 100, N4"]
    field = field_on(case.view, 0)
    n = 66 * 18 // 2
    for cap in (n, n - 1, 1):
        got = MapRegions(field, connectivity=4, max_regions=cap)
        same(got, wanted(case, max_regions=cap), f"cap {cap}")
        assert got.stats["truncated"][0] == int(cap < n) and got.stats["n_kept"][0] == cap
        got.close()
    for minimum in (108, 109):
        ring = BY_NAME["30 x 20, a ring of wall: inside and outside, N4"]
        f2 = field_on(ring.view, 0)
        got = MapRegions(f2, connectivity=4, min_region_cells=minimum)
        same(got, wanted(ring, min_region_cells=minimum), f"minimum {minimum}")
        assert got.stats["n_kept"][0] == (2 if minimum == 108 else 1)
        got.close(); f2.close()
    field.close()


def test_a_field_that_does_not_reach_is_refused(kartohip_lib):
    case = BY_NAME["two rooms, a field of R 3: FAR members, N8"]
    field = field_on(case.view, 3)
    with pytest.raises(capi.KartoHipError) as e:
        MapRegions(field, min_clearance=5 / cases.K)
    assert e.value.code == capi.KH_ERR_INVALID_ARG
    got = MapRegions(field, min_clearance=3 / cases.K)         # Rc == R is taken
    same(got, wanted(case, min_clearance=3 / cases.K), "Rc == R")
    assert got.regions[0]["max_d2"] == capi.KH_FIELD_FAR
    for kw in (dict(connectivity=6), dict(min_clearance=float("nan")), dict(min_region_cells=0), dict(max_frontiers=0), dict(min_clearance=300.0)):
        with pytest.raises(capi.KartoHipError) as e:
            MapRegions(field, **kw)
        assert e.value.code == capi.KH_ERR_INVALID_ARG, kw
    got.close(); field.close()


def test_lookup(kartohip_lib):
    for name in ("40 x 50 random, p_occ 0.4, seed 1, minimum 3, N8", "40 x 50 random, p_occ 0.1, seed 2, N4"):
        case = BY_NAME[name]
        field = field_on(case.view, case.radius)
        got = MapRegions(field, **case.params)
        want = wanted(case)
        pts = cases.lookup_points(case.view)
        rng = np.random.default_rng(9)
        many = np.concatenate([pts, rng.uniform(-14.0, 14.0, size=(257 - len(pts), 2))])
        assert len(many) == 257
        for xy in (pts[:1], pts, many):
            status, ids = got.lookup(xy)
            want_s, want_i = rule.lookup(case.view, want["region_ids"], xy)
            assert np.array_equal(status, want_s) and np.array_equal(ids, want_i), name
        if "minimum" in name:
            assert set(want_s.tolist()) == {rule.AT_OK, rule.AT_NONE, rule.AT_DROPPED, rule.OUTSIDE}
        a, b = pts[0], pts[1]
        assert got.reachable(a, b) == rule.reachable(case.view, want["region_ids"], a, b)
        L = capi.lib()
        status = np.zeros(len(pts), dtype=np.int32)
        assert L.kh_map_regions_lookup(got._h, len(pts), pts.ctypes.data, status.ctypes.data, None) == capi.KH_OK, "either output may be NULL"
        assert np.array_equal(status, rule.lookup(case.view, want["region_ids"], pts)[0])
        bad = pts.copy()
        bad[3, 1] = np.nan
        assert L.kh_map_regions_lookup(got._h, len(bad), bad.ctypes.data, status.ctypes.data, None) == capi.KH_ERR_INVALID_ARG
        got.close(); field.close()


def test_recompute_after_a_door_opens_a_window_change_and_another_lattice(kartohip_lib):
    shut, door = lc.view_of(cases.two_rooms(door=0), cases.A, cases.K), lc.view_of(cases.two_rooms(door=3), cases.A, cases.K)
    d = DeviceView(shut)
    field = MapField(d.v, max_distance=8 / cases.K)
    got = MapRegions(field, min_clearance=1 / cases.K)
    want = rule.analyse(shut, fr.d2_brute(shut, 8), 8, min_clearance=1 / cases.K)
    same(got, want, "shut")
    assert got.stats["n_kept"][0] == 2
    d.upload(door)
    field.update(d.v)
    got.recompute(field)
    want = rule.analyse(door, fr.d2_brute(door, 8), 8, min_clearance=1 / cases.K)
    same(got, want, "the door is open")
    assert got.stats["n_kept"][0] == 1, "two regions became one"
    d.close()
    # another window of the same lattice: the arrays are made anew
    case = BY_NAME["129 x 33 comb, N8"]
    e = DeviceView(case.view)
    field.update(e.v)
    got.recompute(field)
    same(got, rule.analyse(case.view, fr.d2_brute(case.view, 8), 8, min_clearance=1 / cases.K), "after a window change")
    before = (got.stats, got.region_ids)
    # a field on another lattice is refused, and the analysis stands
    other = lc.view_of(cases.two_rooms(), cases.A, 2 * cases.K)
    o = DeviceView(other)
    elsewhere = MapField(o.v, max_distance=1.0)
    assert capi.lib().kh_map_regions_recompute(got._h, elsewhere._h) == capi.KH_ERR_INVALID_ARG
    assert capi.lib().kh_map_regions_recompute(got._h, None) == capi.KH_ERR_INVALID_ARG
    short = MapField(e.v, max_distance=0.5 / cases.K)          # another field of the same lattice, R = 1: Rc == R is taken
    got.recompute(short)
    same(got, rule.analyse(case.view, fr.d2_brute(case.view, 1), 1, min_clearance=1 / cases.K), "a field of R 1")
    assert before[0]["width"] == 129 and before[1].shape == (33, 129)
    for h in (short, elsewhere, got, field):
        h.close()
    o.close(); e.close()


def test_the_same_create_twice_gives_identical_bytes_and_leaves_the_field_alone(kartohip_lib):
    case = BY_NAME["130 x 50 serpentine, N8"]
    mixed = BY_NAME["129 x 33 mixed, N4"]
    for c in (case, mixed):
        field = field_on(c.view, c.radius)
        d2, costs = field.d2, field.costs()
        runs = []
        for _ in range(2):
            got = MapRegions(field, **c.params)
            L, n = capi.lib(), C.c_int32()
            blobs = [got.region_ids.tobytes(), got.frontier_ids.tobytes()]
            for which in (0, 1):
                L.kh_map_regions_get(got._h, which, None, 0, C.byref(n))
                records = (capi.KhRegion * max(1, n.value))()
                assert L.kh_map_regions_get(got._h, which, records, n.value, C.byref(n)) == capi.KH_OK
                blobs.append(bytes(records)[:n.value * C.sizeof(capi.KhRegion)])
            runs.append(blobs)
            got.close()
        assert runs[0] == runs[1]
        assert np.array_equal(field.d2, d2) and np.array_equal(field.costs(), costs), "the analysis wrote the field"
        field.close()


def test_the_localizer_s_wrapper(kartohip_lib):
    """MapLocalizer.regions makes a field that reaches min_clearance for the call; the analysis outlives it"""
    from common import LASER
    from slam_toolbox_amd.map_localizer import MapLocalizer
    from test_map_localize_gpu import PARAMS
    case = BY_NAME["two rooms and a door of 2 cells, Rc 2, N8"]
    d = DeviceView(case.view)
    loc = MapLocalizer(PARAMS, LASER, max_batch=2).set_map(d.v)
    got = loc.regions(max_distance=8 / cases.K, **case.params)
    same(got, wanted(case), "through the localizer")
    far = loc.regions(max_distance=0.25, min_clearance=3.0, connectivity=8)      # the field is made to reach 12 cells
    assert far.stats["clearance_cells"] == 12 and far.stats["n_traversable"] == 0
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
    for conn in (4, 8):
        kw = dict(min_clearance=cases.clearance_of(rc, m.view["scale"]), connectivity=conn)
        got = field.regions(**kw)
        want = rule.analyse(m.view, d2, 40, **kw)
        same(got, want, f"Rc {rc}, N{conn}")
        assert got.stats["clearance_cells"] == rc and got.stats["n_kept"][0] > 1 and got.stats["n_kept"][1] > 1
        poses = np.asarray(sm.poses)[:, :2]
        assert all(got.reachable(a, b) for a in poses for b in poses), "the eight mapped poses are mutually reachable"
        print(f"{m.width} x {m.height}, Rc {rc}, N{conn}: {got.stats['n_kept']} kept of {got.stats['n_total']}, times {got.stats['times_ms']} ms")
        got.close()
