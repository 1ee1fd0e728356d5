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
