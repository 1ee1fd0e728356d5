"""GPU: the map-sourced correlation grid and the matches on it (kh_matcher_add_map / _match_map*, k_map_collect in
csrc/matcher_kernels.hip; kh_occupancy_write_nav, k_nav_to_occ in csrc/occupancy.hip) against tests/map_match_rule.py: the grid
bytes with np.array_equal, the matches bit for bit.  Small matchers, maps of at most about 200 x 200 cells filled through
OccupancyGrid.from_nav, then the maps of tests/map_match_cases.py, whose clips take k_map_collect through more than one trip of its
capped launch; one test -- does a map localise as well as a chain of scans -- uses a built map of the synthetic world."""
import ctypes as C
import math

import numpy as np
import pytest

import map_match_cases as mc
import map_match_rule as mr
from common import LASER, OFFLINE_PARAMS, Scenario, bits
from slam_toolbox_amd import capi, synth

pytestmark = pytest.mark.gpu

SMALL = mc.SMALL                            # 13 x 13 smear kernel, region of interest 831 cells
LOOP = (2.0, 0.05, 0.03, 4.0)               # loop-like: 3 x 3 kernel, region of interest 201 cells
FOOT = mc.FOOT                              # sigma / res = 9.99: the kernel holds 100 on the centre's four neighbours
DYADIC = (2.0, 0.25, 0.25, 8.0)             # every product below is exact: 5 x 5 kernel, region of interest 73 cells
cells_of = mc.cells_of


def pair(create, params=OFFLINE_PARAMS, max_batch=1):
    from oracle import karto
    from slam_toolbox_amd.scan_matcher import MapperParams, ScanMatcher
    return ScanMatcher.Create(MapperParams(**params), *create, max_batch=max_batch), karto.Matcher(*create, params)


def scans_at(pose, ranges=None):
    """the same scan for the library and for the oracle; the grid only reads its sensor pose"""
    from oracle import karto
    from slam_toolbox_amd.scan_matcher import LocalizedRangeScan
    ranges = np.full(8, 1.0) if ranges is None else ranges
    return LocalizedRangeScan(ranges, pose, LASER.min_angle, LASER.ang_res), karto.Scan(ranges, pose, LASER)


def random_nav(rng, h, w, p_occ=0.3):
    return rng.choice(np.array([-1, 100, 0], dtype=np.int8), size=(h, w), p=[(1 - p_occ) / 2, p_occ, (1 - p_occ) / 2])


def check_grid(hm, om, pose, nav, offset, res, slot=0, stats=None):
    """AddMap of from_nav(nav) == the rule's grid; returns the rule's grid"""
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    g = OccupancyGrid.from_nav(nav, offset, res)
    hq, _ = scans_at(pose)
    hm.AddMap(hq, g, slot)
    got = hm.GetCorrelationGrid(slot)
    want = mr.rule_grid(om, pose, mr.map_points(mr.view_dict(cells_of(nav), offset, 1.0 / res)), stats)
    gi, oi = hm.grid_info(slot), om.grid_info()
    assert (gi["offset_x"], gi["offset_y"]) == (oi["offset_x"], oi["offset_y"]) and gi["data_size"] == oi["data_size"]
    assert np.array_equal(got, want), f"{int((got != want).sum())} grid bytes differ"
    g.close()
    return want


# ---------------------------------------------------------------- write_nav

@pytest.mark.parametrize("height", [1, 2])
@pytest.mark.parametrize("width", [1, 3, 4, 7, 8, 9, 63, 64, 65])
def test_write_nav(kartohip_lib, width, height):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    rng = np.random.default_rng(100 * width + height)
    for phase in range(3):
        nav = np.array([(-1, 100, 0)[(k + phase) % 3] for k in range(width * height)], dtype=np.int8).reshape(height, width)
        g = OccupancyGrid.from_nav(nav, (1.0, -0.5), 0.5)
        assert np.array_equal(g.nav(), nav)
        cells = g.cells()
        assert cells.shape == (height, (width + 7) & ~7) and not cells[:, width:].any(), "padding bytes must be zero"
        assert np.array_equal(cells[:, :width], cells_of(nav))
        p, h = g.counters()
        assert not p.any() and not h.any()
        other = random_nav(rng, height, width)
        g.write_nav(other)                                     # over a grid that held something else
        assert np.array_equal(g.nav(), other)
        bad = other.copy()
        bad[height - 1, width - 1] = 50
        with pytest.raises(capi.KartoHipError) as e:
            g.write_nav(bad)
        assert e.value.code == capi.KH_ERR_INVALID_ARG
        assert np.array_equal(g.nav(), other) and np.array_equal(g.cells()[:, :width], cells_of(other)), "a refused write changed the grid"
        g.close()


# ---------------------------------------------------------------- grid bytes

def test_one_cell_and_no_cell(kartohip_lib, oracle_lib):
    hm, om = pair(SMALL)
    pose = np.array([2.0, -1.0, 0.3])
    want = check_grid(hm, om, pose, np.array([[100]], dtype=np.int8), (2.5, -1.25), 0.01)
    assert (want == 100).sum() == 1
    for nav in (np.array([[0]], dtype=np.int8), np.full((5, 9), -1, dtype=np.int8), np.zeros((9, 5), dtype=np.int8)):
        assert not check_grid(hm, om, pose, nav, (2.5, -1.25), 0.01).any()
    hm.close()


@pytest.mark.parametrize("width", [7, 8, 9, 63, 64, 65])
def test_widths_around_the_row_padding_and_the_unit(kartohip_lib, oracle_lib, width):
    hm, om = pair(SMALL)
    rng = np.random.default_rng(width)
    pose = np.array([0.4, 0.2, 0.0])
    for height, p_occ in ((1, 1.0), (3, 0.6), (130, 0.2)):       # (130 rows x 2 units: more units than one workgroup's four waves)
        nav = random_nav(rng, height, width, p_occ)
        nav[:, 0] = 100
        nav[:, width - 1] = 100
        assert check_grid(hm, om, pose, nav, (0.11, 0.03), 0.01).any()
    hm.close()


@pytest.mark.parametrize("create,map_res,name", [(SMALL, 0.01, "equal"), (SMALL, 0.05, "coarser x5"), (SMALL, 0.005, "finer x2"),
                                                 (LOOP, 0.03, "incommensurate")], ids=lambda v: v if isinstance(v, str) else None)
def test_map_resolutions(kartohip_lib, oracle_lib, create, map_res, name):
    hm, om = pair(create)
    rng = np.random.default_rng(17)
    nav = random_nav(rng, 150, 170, 0.25)
    pose = np.array([1.0, 2.0, 0.1])
    offset = (pose[0] - 0.5 * 170 * map_res + 0.0037, pose[1] - 0.5 * 150 * map_res - 0.0041)
    stats = {}
    check_grid(hm, om, pose, nav, offset, map_res, stats=stats)
    assert stats["stamped"] > 100
    if name == "finer x2":
        assert stats["skipped"] > 100, "several map cells per grid cell: the later ones find the cell occupied"
    hm.close()


def test_rounding_ties_half_away_from_zero(kartohip_lib, oracle_lib):
    """map 0.125 on a grid of 0.25, anchors and pose multiples of 0.125: (x - offset) * scale is exact and ends on .5 for every
    other column, left of the grid's cell 0 too -- -0.5 rounds to -1 (outside), not to 0"""
    hm, om = pair(DYADIC)
    pose = np.array([0.125, -0.375, 0.0])
    nav = np.full((192, 192), 100, dtype=np.int8)
    offset = (-12.0, -12.125)
    pts = mr.map_points(mr.view_dict(cells_of(nav), offset, 8.0))
    mr.rule_grid(om, pose, pts[:1])
    gi = om.grid_info()
    gxd = (pts[:, 0] - gi["offset_x"]) * gi["scale"]
    gyd = (pts[:, 1] - gi["offset_y"]) * gi["scale"]
    for v in (gxd, gyd):
        assert (v == -0.5).any() and (v == 0.5).any() and (v == gi["roi_w"] - 0.5).any() and (v == -1.5).any()
    want = check_grid(hm, om, pose, nav, offset, 0.125)
    # the region of interest is full; the ring of cells around it got what the smear kernel spreads, nothing was stamped there
    grid = want.reshape(-1, gi["width_step"])
    roi = grid[gi["roi_y"]:gi["roi_y"] + gi["roi_h"], gi["roi_x"]:gi["roi_x"] + gi["roi_w"]]
    assert (roi == 100).all() and (grid == 100).sum() == gi["roi_w"] * gi["roi_h"]
    hm.close()


def test_region_of_interest_edges(kartohip_lib, oracle_lib):
    """occupied columns and rows that land on grid cells -1, 0, roi - 1 and roi"""
    hm, om = pair(LOOP)
    pose = np.array([3.0, -2.0, 0.0])
    res, n = 0.05, 211
    offset = (pose[0] - 0.5 * (n - 1) * res + 0.004, pose[1] - 0.5 * (n - 1) * res - 0.003)
    mr.rule_grid(om, pose, np.zeros((0, 2)))
    gi = om.grid_info()
    axis = np.arange(n, dtype=np.float64) / (1.0 / res)
    gx = mr._round((offset[0] + axis - gi["offset_x"]) * gi["scale"]).astype(int)
    gy = mr._round((offset[1] + axis - gi["offset_y"]) * gi["scale"]).astype(int)
    nav = np.zeros((n, n), dtype=np.int8)
    for wanted in (-1, 0, gi["roi_w"] - 1, gi["roi_w"]):
        assert (gx == wanted).any() and (gy == wanted).any()
        nav[:, gx == wanted] = 100
        nav[gy == wanted, :] = 100
    stats = {}
    want = check_grid(hm, om, pose, nav, offset, res, stats=stats).reshape(-1, gi["width_step"])
    assert stats["inside"] == 4 * gi["roi_w"] - 4, "columns and rows 0 and roi - 1, nothing of -1 and roi"
    hm.close()


def test_map_outside_and_half_inside(kartohip_lib, oracle_lib):
    hm, om = pair(LOOP)
    rng = np.random.default_rng(4)
    nav = random_nav(rng, 100, 120, 0.3)
    offset = (10.0, 20.0)                                         # the map covers [10, 16] x [20, 25]
    assert not check_grid(hm, om, np.array([100.0, -50.0, 0.0]), nav, offset, 0.05).any()
    assert not check_grid(hm, om, np.array([13.0, 31.0, 0.0]), nav, offset, 0.05).any()      # in reach in x, 6 m off in y
    stats = {}
    check_grid(hm, om, np.array([8.0, 22.5, 0.0]), nav, offset, 0.05, stats=stats)          # the grid ends at x = 13.025
    n_occ = int((nav == 100).sum())
    assert 0.3 * n_occ < stats["inside"] < 0.7 * n_occ
    assert not check_grid(hm, om, np.array([1e300, 0.0, 0.0]), nav, offset, 0.05).any()
    hm.close()


def test_order_dependent_skip(kartohip_lib, oracle_lib):
    """a smear kernel with 100 off-centre: of two neighbouring occupied cells the later one finds its cell occupied and does not
    stamp -- in row-major order"""
    hm, om = pair(FOOT)
    assert (om.kernel() == 100).sum() == 5
    rng = np.random.default_rng(8)
    nav = random_nav(rng, 90, 110, 0.15)
    nav[40, 10:100] = 100                                         # walls
    nav[10:80, 55] = 100
    nav[60:64, 20:24] = 100
    pose = np.array([-1.0, 0.5, 0.0])
    offset = (pose[0] - 0.55 + 0.0012, pose[1] - 0.45 + 0.0031)
    stats = {}
    want = check_grid(hm, om, pose, nav, offset, 0.01, stats=stats)
    assert stats["skipped"] > 100 and stats["stamped"] > 100, "the skip did not fire in the rule for this input"
    # the visiting order decides: the same cells from the last to the first give another grid (column-major would not: of two
    # 4-neighbours it visits the same one first as row-major does)
    pts = mr.map_points(mr.view_dict(cells_of(nav), offset, 1.0 / 0.01))
    assert not np.array_equal(mr.rule_grid(om, pose, pts[::-1]), want)
    hm.close()


def test_hand_made_view_with_negative_origin(kartohip_lib, oracle_lib):
    hm, om = pair(LOOP)
    rng = np.random.default_rng(21)
    width, height, ws = 77, 60, 96                               # a row stride of the caller's own
    cells = np.zeros((height, ws), dtype=np.uint8)
    cells[:, :width] = cells_of(random_nav(rng, height, width, 0.3))
    cells[:, width:] = 100                                        # beyond `width`: not cells
    L = capi.lib()
    buf = C.c_void_p()
    capi.check(L.kh_device_malloc(0, cells.size, C.byref(buf)), "kh_device_malloc")
    capi.check(L.kh_device_upload(buf, cells.ctypes.data, cells.size), "kh_device_upload")
    v = capi.KhMapView()
    v.device_cells, v.device, v.width, v.height, v.width_step, v.ox, v.oy = buf.value, 0, width, height, ws, -40, -25
    v.anchor[0], v.anchor[1], v.scale = 0.51, -0.27, 1.0 / 0.04
    pose = np.array([0.3, 0.1, 0.0])
    hq, _ = scans_at(pose)
    hm.AddMap(hq, v)
    want = mr.rule_grid(om, pose, mr.map_points(mr.view_dict(cells, (0.51, -0.27), 1.0 / 0.04, -40, -25, width)))
    assert want.any() and np.array_equal(hm.GetCorrelationGrid(), want)
    # malformed views, a bad slot
    scan = hq.c()
    for field, value in (("width", 0), ("height", -1), ("width_step", width - 1), ("scale", 0.0), ("scale", math.inf), ("scale", math.nan),
                         ("device", 1), ("device_cells", None)):
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        assert L.kh_matcher_add_map(hm._h, 0, C.byref(scan), C.byref(w)) == capi.KH_ERR_INVALID_ARG, field
    assert L.kh_matcher_add_map(hm._h, 1, C.byref(scan), C.byref(v)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_matcher_add_map(hm._h, -1, C.byref(scan), C.byref(v)) == capi.KH_ERR_INVALID_ARG
    out = np.zeros(2), np.zeros(6), np.zeros(18), np.zeros(2, dtype=np.int32)
    arr = (capi.KhScan * 2)(scan, scan)
    assert L.kh_matcher_match_map_batch(hm._h, 2, arr, C.byref(v), 1, 1, out[1], out[2], out[0], out[3]) == capi.KH_ERR_INVALID_ARG, "n > max_batch"
    assert np.array_equal(hm.GetCorrelationGrid(), want), "a refused call changed the grid"
    hm.close()
    L.kh_device_free(buf)


def test_live_map_view_after_growth(kartohip_lib, oracle_lib):
    from test_live_map_edges_gpu import _place, _synthetic, placing_mapper
    laser = synth.Laser()
    poses, ranges = _synthetic(6, 3)
    poses[:3, :2] = [(10.0, 10.0), (10.5, 10.2), (11.0, 10.1)]
    poses[3:, :2] = [(26.0, 24.0), (26.5, 24.5), (27.0, 24.2)]
    m = placing_mapper(laser)
    live = m.live_map(0.05, np.array([16.0, 16.0]), math.inf)     # an anchor inside the map: negative lattice cells
    with pytest.raises(capi.KartoHipError) as e:
        live.view()
    assert e.value.code == capi.KH_ERR_NOT_FOUND
    for k in range(3):
        _place(m, ranges[k], poses[k], k)
    live.update()
    first = live.info()
    for k in range(3, 6):
        _place(m, ranges[k], poses[k], k)
    assert live.update()["relayouts"] == 1, "the window did not grow"
    info, v = live.info(), live.view()
    assert (info["width"], info["height"]) != (first["width"], first["height"]) and info["ox"] < 0 and info["oy"] < 0
    assert (v.ox, v.oy, v.width, v.height, v.width_step) == tuple(info[k] for k in ("ox", "oy", "width", "height", "width_step"))
    assert (v.anchor[0], v.anchor[1], v.scale) == (16.0, 16.0, 1.0 / 0.05)
    cells = live.cells()
    view = mr.view_dict(cells, (16.0, 16.0), v.scale, v.ox, v.oy, v.width)
    hm, om = pair(LOOP)
    for k, pose in enumerate((poses[1], poses[4], np.array([18.0, 17.0, 0.0]))):
        hq, _ = scans_at(pose)
        hm.AddMap(hq, live)
        want = mr.rule_grid(om, pose, mr.map_points(view))
        assert np.array_equal(hm.GetCorrelationGrid(), want)
        assert k == 2 or want.any()
    hm.close(); live.close(); m.close()


# ---------------------------------------------------------------- slot coherence

def _scenario_map(sc, res, half=5.0):
    """a nav grid of `half` metres around the scenario's query: the base scans' in-range end points occupied, the rest unknown"""
    n = int(round(2 * half / res))
    offset = (sc.query_pose[0] - half + 0.0013, sc.query_pose[1] - half - 0.0021)
    nav = np.full((n, n), -1, dtype=np.int8)
    for r, p in zip(sc.ranges[:sc.n_base], sc.base_poses):
        pts = synth.scan_points(r, p, LASER)
        ok = np.isfinite(r) & (r < LASER.range_threshold) & (r > LASER.min_range)
        i = np.floor((pts[ok, 0] - offset[0]) / res + 0.5).astype(int)
        j = np.floor((pts[ok, 1] - offset[1]) / res + 0.5).astype(int)
        keep = (i >= 0) & (i < n) & (j >= 0) & (j < n)
        nav[j[keep], i[keep]] = 100
    return nav, offset


def test_slot_takes_maps_and_scans_in_turn(kartohip_lib, oracle_lib):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    sc = Scenario(seed=3, n_base=6, start=40)
    hq, hb = sc.hip_scans()
    nav_a, off_a = _scenario_map(sc, 0.05)
    rng = np.random.default_rng(2)
    nav_b, off_b = random_nav(rng, 120, 90, 0.3), (sc.query_pose[0] - 1.0, sc.query_pose[1] - 2.0)
    ga, gb = OccupancyGrid.from_nav(nav_a, off_a, 0.05), OccupancyGrid.from_nav(nav_b, off_b, 0.02)
    other, _ = scans_at(sc.query_pose + np.array([0.7, -0.4, 0.2]))
    for create in (SMALL, FOOT):
        hm, om = pair(create)
        steps = [("map", hq, ga), ("scans", hq, hb), ("map", other, gb), ("scans", other, hb[:2]), ("map", hq, ga)]
        for step, (kind, q, src) in enumerate(steps):
            fresh, _ = pair(create)
            for h in (hm, fresh):
                h.AddMap(q, src) if kind == "map" else h.AddScans(q, src)
            got, want = hm.GetCorrelationGrid(), fresh.GetCorrelationGrid()
            assert want.any(), f"{create} step {step} ({kind}): a fresh handle's grid is empty"
            assert np.array_equal(got, want), f"{create} step {step} ({kind}): {int((got != want).sum())} bytes differ from a fresh handle's"
            fresh.close()
        # ... and a single MatchScan (the fused path keeps its own tables of the slot) between two maps
        fresh, _ = pair(create)
        for a, b in zip(hm.MatchScan(hq, hb), fresh.MatchScan(hq, hb)):
            assert np.array_equal(bits(a), bits(b)), f"{create}: MatchScan after a map differs from a fresh handle's"
        assert np.array_equal(hm.GetCorrelationGrid(), fresh.GetCorrelationGrid())
        fresh.close()
        hm.AddMap(other, gb)
        fresh, _ = pair(create)
        fresh.AddMap(other, gb)
        assert np.array_equal(hm.GetCorrelationGrid(), fresh.GetCorrelationGrid())
        fresh.close(); hm.close()
    ga.close(); gb.close()


def test_match_is_the_same_on_every_scoring_path(kartohip_lib, oracle_lib):
    """the block map (dense scoring ignores it), the re-pitched copies (off: scored from the grid itself) and the LDS-staged
    kernels all read what the map rasterisation left"""
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    sc = Scenario(seed=3, n_base=6, start=40)
    hq, hb = sc.hip_scans()
    nav, off = _scenario_map(sc, 0.04, half=4.0)
    g = OccupancyGrid.from_nav(nav, off, 0.04)
    for create in (SMALL, LOOP):
        results = []
        for debug in (dict(), dict(dense_score=True), dict(no_dual_copy=True), dict(lds_score=True), dict(windowed_score=True)):
            hm, _ = pair(create)
            hm.set_debug(False, **debug)
            first = hm.MatchScanMap(hq, g)
            hm.AddScans(hq, hb)                                   # the slot's copies and block map follow the scans ...
            hm.MatchScanMap(hq, g)
            again = hm.MatchScanMap(hq, g)                        # ... and the map again
            for a, b in zip(first, again):
                assert np.array_equal(bits(a), bits(b))
            results.append(first)
            hm.close()
        assert results[0][0] > 0.1
        for r in results[1:]:
            for a, b in zip(results[0], r):
                assert np.array_equal(bits(a), bits(b))
    g.close()


# ---------------------------------------------------------------- matches

MAX_BATCH = 4


@pytest.fixture(scope="module")
def match_case():
    """one map, MAX_BATCH queries around it (the last far off the map), and the rule's match of each for the four flag pairs"""
    sc = Scenario(seed=12, n_base=8, start=90)
    nav, off = _scenario_map(sc, 0.05)
    rng = np.random.default_rng(5)
    poses = [sc.query_pose + np.array([rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), rng.uniform(-0.1, 0.1)]) for _ in range(MAX_BATCH - 1)]
    poses.append(sc.query_pose + np.array([300.0, 100.0, 0.5]))
    queries = [scans_at(p, sc.query_ranges) for p in poses]
    from oracle import karto
    om = karto.Matcher(*SMALL, OFFLINE_PARAMS)
    pts = mr.map_points(mr.view_dict(cells_of(nav), off, 1.0 / 0.05))
    want = {}
    for k, (_, oq) in enumerate(queries):
        grid = mr.rule_grid(om, oq.sensor_pose, pts)
        for flags in ((True, True), (False, True), (True, False), (False, False)):
            mr.install(om, grid)
            want[k, flags] = mr.match(om, oq, OFFLINE_PARAMS, *flags)
    return nav, off, queries, want


@pytest.mark.parametrize("n", [1, 3, MAX_BATCH])
@pytest.mark.parametrize("flags", [(True, True), (False, True), (True, False), (False, False)], ids=["pen+fine", "fine", "pen", "plain"])
def test_match_map_batch(kartohip_lib, oracle_lib, match_case, n, flags):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    nav, off, queries, want = match_case
    g = OccupancyGrid.from_nav(nav, off, 0.05)
    hm, _ = pair(SMALL, max_batch=MAX_BATCH)
    which = list(range(MAX_BATCH - n, MAX_BATCH))                 # the far-off query is in every batch
    resp, means, covs, status = hm.MatchScanMapBatch([queries[k][0] for k in which], g, *flags)
    assert (status == capi.KH_OK).all()
    for row, k in enumerate(which):
        w = want[k, flags]
        assert np.array_equal(bits(resp[row]), bits(w[0])), (k, resp[row], w[0])
        assert np.array_equal(bits(means[row]), bits(w[1])), (k, means[row], w[1])
        assert np.array_equal(bits(covs[row]), bits(w[2])), k
    assert resp[-1] == 0.0 and (resp[:-1] > 0.1).all() if n > 1 else resp[-1] == 0.0
    if n == 1:
        one = hm.MatchScanMap(queries[which[0]][0], g, *flags)
        for a, b in zip(one, want[which[0], flags]):
            assert np.array_equal(bits(a), bits(b))
    hm.close(); g.close()


def test_empty_query(kartohip_lib, oracle_lib, match_case):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    nav, off, queries, want = match_case
    g = OccupancyGrid.from_nav(nav, off, 0.05)
    hm, om = pair(SMALL, max_batch=MAX_BATCH)
    pose = np.array([1.0, 2.0, 0.3])
    he, oe = scans_at(pose, np.zeros(0))
    w = mr.match(om, oe, OFFLINE_PARAMS)
    car = OFFLINE_PARAMS["coarse_angle_resolution"]
    assert w[0] == 0.0 and np.array_equal(w[1], pose) and np.array_equal(np.diag(w[2]), [500.0, 500.0, 4 * (car * car)])
    resp, means, covs, status = hm.MatchScanMapBatch([queries[0][0], he, queries[1][0]], g)
    assert (status == capi.KH_OK).all()
    for a, b in zip((resp[1], means[1], covs[1]), w):
        assert np.array_equal(bits(a), bits(b))
    for row, k in ((0, 0), (2, 1)):
        for a, b in zip((resp[row], means[row], covs[row]), want[k, (True, True)]):
            assert np.array_equal(bits(a), bits(b))
    for a, b in zip(hm.MatchScanMap(he, g), w):
        assert np.array_equal(bits(a), bits(b))
    hm.close(); g.close()


# ---------------------------------------------------------------- clips beyond one trip of k_map_collect

TRIP_CASES = mc.trip_cases()


@pytest.mark.parametrize("case", TRIP_CASES, ids=[c.name for c in TRIP_CASES])
def test_clips_of_more_units_than_one_trip(kartohip_lib, oracle_lib, case):
    """maps of 1040 .. 8320 units inside the region of interest (tests/map_match_cases.py): k_map_collect's second and third trip,
    k_map_collect_scan with up to nine units per thread; the point order decides the bytes where the kernel holds 100 off-centre and
    the skips where several map cells share a grid cell"""
    hm, om = pair(case.create)
    stats = {}
    check_grid(hm, om, case.pose, case.nav, case.offset, case.res, stats=stats)
    assert stats["inside"] == (case.nav == 100).sum() and stats["stamped"] > 1000
    assert stats["skipped"] > 1000 or (case.res == 0.01 and case.create == mc.SMALL)
    hm.close()


def test_match_map_batch_with_clips_of_every_size(kartohip_lib, oracle_lib):
    """one batch whose jobs hold 8320 units, 3 units at the most and none: the launch is sized by the first, the waves of the second
    leave the loop at once and the scan of the third writes a total of 0"""
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    b = mc.batch_case()
    sc = Scenario(seed=12, n_base=8, start=90)
    g = OccupancyGrid.from_nav(b.nav, b.offset, b.res)
    hm, om = pair(b.create, max_batch=len(b.poses))
    queries = [scans_at(p, sc.query_ranges) for p in b.poses]
    pts = mr.map_points(mr.view_dict(mc.cells_of(b.nav), b.offset, 1.0 / b.res))
    resp, means, covs, status = hm.MatchScanMapBatch([q for q, _ in queries], g)
    assert (status == capi.KH_OK).all()
    occupied = []
    for k, (_, oq) in enumerate(queries):
        grid = mr.rule_grid(om, oq.sensor_pose, pts)
        got = hm.GetCorrelationGrid(k)
        assert np.array_equal(got, grid), f"job {k}: {int((got != grid).sum())} grid bytes differ"
        occupied.append(int((grid == 100).sum()))
        mr.install(om, grid)
        w = mr.match(om, oq, OFFLINE_PARAMS)
        assert np.array_equal(bits(resp[k]), bits(w[0])), (k, resp[k], w[0])
        assert np.array_equal(bits(means[k]), bits(w[1])), (k, means[k], w[1])
        assert np.array_equal(bits(covs[k]), bits(w[2])), k
    assert occupied[0] > 10000 and occupied[1:] == [1, 0] and resp[2] == 0.0
    hm.close(); g.close()


# ---------------------------------------------------------------- does it localise

def test_map_localises_like_a_chain(kartohip_lib, oracle_lib):
    """A scan at a known pose, handed over with an offset inside the search window, matched against (a) the occupancy map of 40
    trajectory scans at 0.05 m, on the GPU, and (b) its nearest 10 scans, by the oracle on the CPU -- the reference's own answer.

    Bound: the map match may lie further from the truth than the chain match by at most half a map-cell diagonal plus one fine
    lattice step.  A base point and the centre of the map cell it fell into are at most half a diagonal apart -- that is the largest
    displacement the map can give any point of the scene, so the best alignment moves by no more -- and both answers are lattice
    points of the fine search, one step apart at the least.  In heading the same displacement, seen from the sensor at the median
    valid range r of the query, is a turn of half_diagonal / r; one fine angle step is added likewise."""
    from oracle import karto
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    from slam_toolbox_amd.scan_matcher import LocalizedRangeScan, MapperParams, ScanMatcher
    create, params = (0.3, 0.01, 0.03, 12.0), OFFLINE_PARAMS
    world, rng = synth.make_world(12345), np.random.default_rng(77)
    truth, _ = synth.trajectory(60)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(41)]
    base_h = [LocalizedRangeScan(ranges[i], truth[i], LASER.min_angle, LASER.ang_res) for i in range(40)]
    g = OccupancyGrid.CreateFromScans(base_h, 0.05, LASER)
    gt = truth[40]
    offset = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05)])
    hq = LocalizedRangeScan(ranges[40], gt + offset, LASER.min_angle, LASER.ang_res)
    hm = ScanMatcher.Create(MapperParams(**params), *create)
    r_map, mean_map, _ = hm.MatchScanMap(hq, g)
    nearest = np.argsort(np.hypot(truth[:40, 0] - gt[0], truth[:40, 1] - gt[1]))[:10]
    om = karto.Matcher(*create, params)
    r_chain, mean_chain, _ = om.match_scan(karto.Scan(ranges[40], gt + offset, LASER),
                                           [karto.Scan(ranges[i], truth[i], LASER) for i in sorted(nearest)])

    def dist(mean):
        dh = (mean[2] - gt[2] + math.pi) % (2 * math.pi) - math.pi
        return math.hypot(mean[0] - gt[0], mean[1] - gt[1]), abs(dh)
    (dp_map, dh_map), (dp_chain, dh_chain) = dist(mean_map), dist(mean_chain)
    half_diagonal, fine_step, fine_angle = 0.5 * math.sqrt(2.0) * 0.05, 0.01, params["fine_search_angle_offset"]
    valid = ranges[40][np.isfinite(ranges[40]) & (ranges[40] < 12.0)]
    r_med = float(np.median(valid))
    print(f"map match: response {r_map:.4f}, {dp_map:.4f} m and {dh_map:.5f} rad from the truth; chain match: response {r_chain:.4f}, "
          f"{dp_chain:.4f} m and {dh_chain:.5f} rad; handed over {math.hypot(offset[0], offset[1]):.4f} m and {abs(offset[2]):.5f} rad off; "
          f"bounds on the excess {half_diagonal + fine_step:.4f} m, {half_diagonal / r_med + fine_angle:.5f} rad (median range {r_med:.2f} m)")
    assert r_map > 0.1 and r_chain > 0.1
    assert dp_map - dp_chain <= half_diagonal + fine_step
    assert dh_map - dh_chain <= half_diagonal / r_med + fine_angle
    hm.close(); g.close()
