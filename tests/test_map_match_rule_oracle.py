"""CPU: tests/map_match_rule.py -- the numpy statement of the map-sourced rasterisation rule and of MatchScan's control flow --
is pinned to the oracle.  Fed the points FindValidPoints keeps of real base scans, in container order, the rule's point loop
must give ScanMatcher::AddScans' grid byte for byte (a 3 x 3 smear kernel, and one that holds 100 off-centre, where the "cell
already occupied" skip depends on the order); MatchScan restated on CorrelateScan over that grid must give MatchScan's result
exactly."""
import numpy as np
import pytest

import map_match_rule as mr
from common import OFFLINE_PARAMS, PRESETS, Scenario, bits
from oracle import karto

GEOMETRIES = {
    "kernel3": (0.3, 0.01, 0.005, 4.0),           # sigma / res = 0.5: half width round(2 * 0.5) = 1
    "foot4": (0.3, 0.01, 0.0999, 4.0),            # sigma / res = 9.99 >= 9.9875: the four neighbours hold 100 too
    "loop": (2.0, 0.05, 0.03, 4.0),
}


def _valid_points(om, query, base):
    pts = [om.find_valid_points(b, query.sensor_pose[:2]) for b in base]
    return np.concatenate(pts, axis=0)


@pytest.mark.parametrize("name", ["kernel3", "foot4", "loop"])
def test_rule_loop_is_add_scans(oracle_lib, name):
    sc = Scenario(seed=5, n_base=6, start=30)
    query, base = sc.oracle_scans()
    om = karto.Matcher(*GEOMETRIES[name], OFFLINE_PARAMS)
    kernel = om.kernel()
    n100 = int((kernel == 100).sum())
    assert kernel.shape == ((3, 3) if name == "kernel3" else kernel.shape) and n100 == (5 if name == "foot4" else 1)
    om.add_scans(query, base)
    want = om.grid()
    assert want.any()
    stats = {}
    got = mr.rule_grid(om, query.sensor_pose, _valid_points(om, query, base), stats)
    assert stats["stamped"] > 0 and stats["skipped"] > 0
    assert np.array_equal(got, want)
    # the order matters where the kernel holds 100 off-centre: the same points backwards stamp another set
    if name == "foot4":
        back = mr.rule_grid(om, query.sensor_pose, _valid_points(om, query, base)[::-1])
        assert not np.array_equal(back, want)


@pytest.mark.parametrize("preset,penalize,refine", [("K", True, True), ("K", False, False), ("L", True, True)])
def test_match_is_match_scan(oracle_lib, preset, penalize, refine):
    create, params = PRESETS[preset]["create"], PRESETS[preset]["params"]
    create = create[:3] + (6.0,)                       # a short range threshold keeps the grids small
    sc = Scenario(seed=9, n_base=5, start=60)
    query, base = sc.oracle_scans()
    ref = karto.Matcher(*create, params)
    want = ref.match_scan(query, base, penalize, refine)
    om = karto.Matcher(*create, params)
    grid = mr.rule_grid(om, query.sensor_pose, _valid_points(om, query, base))
    assert np.array_equal(grid, ref.grid())
    mr.install(om, grid)
    assert np.array_equal(om.grid(), grid)
    got = mr.match(om, query, params, penalize, refine)
    assert want[0] > 0.0
    for a, b in zip(want, got):
        assert np.array_equal(bits(a), bits(b))


def test_match_expands_on_an_empty_grid(oracle_lib):
    """nothing in reach: response 0 after three expansions, the same as MatchScan without base scans; an empty query gives
    Mapper.cpp:547-557's result"""
    create, params = (0.3, 0.01, 0.03, 4.0), OFFLINE_PARAMS
    sc = Scenario(seed=9, n_base=1, start=60)
    query, _ = sc.oracle_scans()
    ref = karto.Matcher(*create, params)
    want = ref.match_scan(query, [], True, True)
    om = karto.Matcher(*create, params)
    mr.install(om, mr.rule_grid(om, query.sensor_pose, np.zeros((0, 2))))
    got = mr.match(om, query, params, True, True)
    assert want[0] == 0.0
    for a, b in zip(want, got):
        assert np.array_equal(bits(a), bits(b))
    empty = karto.Scan(np.zeros(0), query.sensor_pose, points=np.zeros((0, 2)))
    for a, b in zip(ref.match_scan(empty, [], True, True), mr.match(om, empty, params, True, True)):
        assert np.array_equal(bits(a), bits(b))


def test_map_points_order_and_arithmetic():
    cells = np.zeros((3, 8), dtype=np.uint8)
    cells[0, 4] = cells[2, 1] = cells[1, 0] = 100
    cells[1, 3] = 255
    cells[0, 7] = 100                                  # beyond `width`: padding, not a cell
    v = mr.view_dict(cells, (0.3, -0.7), 1.0 / 0.03, ox=-5, oy=2, width=7)
    pts = mr.map_points(v)
    want = [(0.3 + (-5 + 4) / v["scale"], -0.7 + (2 + 0) / v["scale"]), (0.3 + (-5 + 0) / v["scale"], -0.7 + (2 + 1) / v["scale"]),
            (0.3 + (-5 + 1) / v["scale"], -0.7 + (2 + 2) / v["scale"])]
    assert np.array_equal(bits(pts), bits(np.array(want)))


# ---------------------------------------------------------------- maps beyond one trip of k_map_collect (tests/map_match_cases.py)
import map_match_cases as mc      # noqa: E402

TRIP_CASES = mc.trip_cases()
_grids = {}


def _view(case):
    return mr.view_dict(mc.cells_of(case.nav), case.offset, 1.0 / case.res)


def _rule(case):
    """(grid info, view, points, grid, stats) of a case, computed once"""
    if case.name not in _grids:
        om = karto.Matcher(*case.create, OFFLINE_PARAMS)
        view, stats = _view(case), {}
        pts = mr.map_points(view)
        grid = mr.rule_grid(om, case.pose, pts, stats)
        _grids[case.name] = (om.grid_info(), view, pts, grid, stats, om)
    return _grids[case.name]


@pytest.mark.parametrize("case", TRIP_CASES, ids=[c.name for c in TRIP_CASES])
def test_trip_case_holds_the_units_of_its_name(oracle_lib, case):
    gi, view, pts, grid, stats, om = _rule(case)
    h, w = case.nav.shape
    per_row = -(-w // 64)
    lower, upper = mr.units_lower_bound(view, gi), mr.units_upper_bound(view, gi)
    assert lower > case.above and f"above {case.above} units" in case.name
    assert lower == upper == per_row * h, "the map lies inside the region of interest: the clip is the map, unit u is row u // per_row"
    assert stats["inside"] == len(pts) == (case.nav == 100).sum() and stats["stamped"] > 0
    occ = case.nav == 100
    assert 0.05 <= occ.mean() <= 0.25 and occ[0].all() and occ[-1].all() and occ[:, 0].all() and occ[:, -1].all()
    units = np.zeros((h, per_row * 64), dtype=bool)
    units[:, :w] = occ
    per_unit = units.reshape(h, per_row, 64).sum(axis=2).ravel()
    if lower > mc.TRIP_UNITS:
        assert per_unit[mc.TRIP_UNITS - 1] > 0 and per_unit[mc.TRIP_UNITS] > 0, "occupied cells on either side of unit 4096"
        if case.res < 0.01:
            # several map cells per grid cell: points of trip two find their cell occupied
            first = int(per_unit[:mc.TRIP_UNITS].sum())
            before = {}
            mr.rule_grid(om, case.pose, pts[:first], before)
            assert stats["skipped"] - before["skipped"] > 0 and before["skipped"] > 0
    assert -(-lower // mc.SCAN_THREADS) > 1, "more than one unit per thread of the scan"


def test_the_stamping_order_shows_in_the_bytes_of_a_trip_case(oracle_lib):
    """a smear kernel that holds 100 on its centre alone gives the same bytes in any order (a stamp is a maximum), so the cases on FOOT's
    kernel are the ones that test the order: the same points backwards give another grid"""
    changed = []
    for case in TRIP_CASES:
        gi, view, pts, grid, stats, om = _rule(case)
        n100 = int((om.kernel() == 100).sum())
        if n100 == 1 and case.res == 0.005:
            continue                                                     # (no information, and the slowest of the table)
        back = mr.rule_grid(om, case.pose, pts[::-1])
        assert n100 > 1 or np.array_equal(back, grid)
        if not np.array_equal(back, grid):
            changed.append(case.name)
    assert len(changed) == 2 and all("100 off-centre" in n for n in changed)


def test_batch_case_holds_its_three_clips(oracle_lib):
    b = mc.batch_case()
    view = mr.view_dict(mc.cells_of(b.nav), b.offset, 1.0 / b.res)
    pts = mr.map_points(view)
    om = karto.Matcher(*b.create, OFFLINE_PARAMS)
    bounds, inside = [], []
    for pose in b.poses:
        stats = {}
        mr.rule_grid(om, pose, pts, stats)
        gi = om.grid_info()
        bounds.append((mr.units_lower_bound(view, gi), mr.units_upper_bound(view, gi)))
        inside.append(stats["inside"])
    assert bounds[0] == (8320, 8320) and bounds[0][0] > mc.TRIP_UNITS and inside[0] == len(pts)
    assert bounds[1] == (1, 3) and inside[1] == 1, "the map's first cell alone; the clip adds at most two rows and two columns"
    assert bounds[2] == (0, 0) and inside[2] == 0
    gi = om.grid_info()                                                  # (centred on the last pose)
    reach = (gi["roi_w"] + 4) / gi["scale"]
    assert b.poses[2][0] - reach > b.offset[0] + b.nav.shape[1] * b.res, "300 m away: no clip rule reaches the map"
    assert [hi for _, hi in bounds] == b.units and len(b.poses) == 3


def test_capped_launches_left_alone_are_crossed_by_the_golden_shapes():
    """k_raster_tile and k_repitch* run on at most 2048 tiles of 64 x 64 cells, k_repitch_full on at most 4096 rows: the S preset's grid
    holds 4096 tiles and the C2 preset's more than 8000 rows, both rasterised by
    tests/test_baseline_shapes_gpu.py::test_golden_vectors_on_the_hip_path (match_S, corr_C2)"""
    from common import Golden
    width, height = (int(v) for v in Golden("match_S").d["grid_geom"][:2])
    assert -(-width // 64) * -(-height // 64) == 4096 > 2048
    assert int(Golden("corr_C2").d["grid_geom"][1]) > 8000 > 4096
