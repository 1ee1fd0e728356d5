"""GPU: the occupancy kernels (k_occ_trace, k_occ_trace_resident, k_occ_update; csrc/occupancy.hip) against the CPU oracle
(oracle/occupancy_oracle.c) on the edge inputs of tests/occupancy_cases.py: beams that leave the grid or never enter it, negative
cell indices and rounding ties, every direction of the walk, readings on each range gate, grid widths around the 8-cell width
step, cells exactly on `pass == min_pass_through` and `hits / pass == occupancy_threshold`, 50 000 increments of one cell, and
a grid object reused over calls of very different sizes.  Every comparison is np.array_equal over the whole (height, width_step)
extent of all three arrays, padding columns included.  tests/test_edge_cases_oracle.py checks on the CPU that each case reaches
its edge.

Not tested, on purpose: a KEPT beam whose point reading is not finite.  o_to_int turns it into INT32_MIN and the Bresenham walk
(the reference's too) runs for 2^31 steps -- the library inherits that input from the reference unguarded."""
import ctypes as C
import os

import numpy as np
import pytest

import occupancy_cases as oc
from common import LASER
from slam_toolbox_amd import synth
from test_edge_cases_oracle import oracle_scans

pytestmark = pytest.mark.gpu
OCC = list(oc.all_cases())
EDGES = np.load(os.path.join(os.path.dirname(__file__), "golden", "occupancy_edges.npz"))


def hip_scans(scans):
    """[(sensor_xy, ranges, points)] -> library scans with the point readings replaced (AddScans reads ranges, points and the
    sensor position only)"""
    from slam_toolbox_amd.scan_matcher import LocalizedRangeScan
    out = []
    for s, r, p in scans:
        h = LocalizedRangeScan(np.ones(r.shape[0]), np.array([s[0], s[1], 0.0]), LASER.min_angle, LASER.ang_res)
        h.ranges = np.ascontiguousarray(r, dtype=np.float64).copy()
        h.points = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 2).copy()
        out.append(h)
    return out


def assert_grid_equals(g, want, what=""):
    cells, p, hits = want
    gp, gh = g.counters()
    assert gp.shape == p.shape == (g.height, g.width_step)
    assert np.array_equal(gp, p), f"{what}: {int((gp != p).sum())} pass counters differ"
    assert np.array_equal(gh, hits), f"{what}: {int((gh != hits).sum())} hit counters differ"
    gc = g.cells()
    assert np.array_equal(gc, cells), f"{what}: {int((gc != cells).sum())} cell states differ"


def _edges_dense():
    w, h, ws = (int(v) for v in EDGES["dims"])
    cells = np.zeros(ws * h, dtype=np.uint8)
    cells[EDGES["cells_idx"]] = EDGES["cells_val"]
    p, hits = np.zeros(ws * h, dtype=np.uint32), np.zeros(ws * h, dtype=np.uint32)
    p[EDGES["count_idx"]] = EDGES["pass_val"]
    hits[EDGES["count_idx"]] = EDGES["hit_val"]
    return w, h, ws, cells.reshape(h, ws), p.reshape(h, ws), hits.reshape(h, ws)


def test_range_gates_match_the_reference(kartohip_lib):
    """the reference's own OccupancyGrid::CreateFromScans on scans whose ranges sit on every gate
    (tests/golden/occupancy_edges.npz, made by tests/golden/make_golden_occupancy_edges.py).  Its points are all finite, so a
    regression of a range gate fails here by assertion (the case table guards its NaN points with finite twins)"""
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    from slam_toolbox_amd.scan_matcher import LocalizedRangeScan
    w, h, ws, cells, p, hits = _edges_dense()
    scans = [LocalizedRangeScan(EDGES["ranges"][k], EDGES["poses"][k], LASER.min_angle, LASER.ang_res) for k in range(EDGES["ranges"].shape[0])]
    g = OccupancyGrid.CreateFromScans(scans, float(EDGES["resolution"]), LASER)
    assert (g.GetWidth(), g.GetHeight(), g.width_step) == (w, h, ws)
    assert np.array_equal(g.offset.view(np.uint64), np.asarray(EDGES["offset"], dtype=np.float64).view(np.uint64))
    assert_grid_equals(g, (cells, p, hits), "reference gates")
    g.close()


@pytest.mark.parametrize("case", OCC, ids=[c.name for c in OCC])
def test_case_equals_the_oracle(kartohip_lib, oracle_lib, case):
    from oracle import karto
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    twin = oc.finite_twin(case)
    if twin is not None:
        # dropped beams of this case carry NaN points; its finite twin goes first, so that a kernel which keeps one of them is
        # stopped here by an assertion and never walks the NaN
        g = OccupancyGrid(twin.width, twin.height, twin.offset, twin.resolution)
        g.AddScans(hip_scans(twin.scans), twin.gates)
        g.Update(twin.min_pass, twin.threshold)
        assert_grid_equals(g, karto.occupancy_from_scans(twin.width, twin.height, twin.offset, twin.resolution, oracle_scans(twin.scans),
                                                         twin.gates, twin.min_pass, twin.threshold), twin.name)
        g.close()
    want = karto.occupancy_from_scans(case.width, case.height, case.offset, case.resolution, oracle_scans(case.scans), case.gates,
                                      case.min_pass, case.threshold)
    g = OccupancyGrid(case.width, case.height, case.offset, case.resolution)
    g.AddScans(hip_scans(case.scans), case.gates)
    g.Update(case.min_pass, case.threshold)
    assert_grid_equals(g, want, case.name)
    assert g.stats()["beams"] == sum(r.size for _, r, _ in case.scans)
    g.close()


def test_contention_closed_form(kartohip_lib):
    """50 000 increments of the same counters: the closed form, next to the oracle comparison of the case table"""
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    case = oc.contention_case()
    g = OccupancyGrid(case.width, case.height, case.offset, case.resolution)
    g.AddScans(hip_scans(case.scans), case.gates)
    p, hits = g.counters()
    n = oc.CONTENTION_BEAMS
    assert p[1, 1] == n and hits[1, 1] == 0 and p[1, 6] == 2 * n and hits[1, 6] == n
    assert p.sum() == 7 * n and hits.sum() == n
    g.close()


def test_update_twice_without_clear(kartohip_lib, oracle_lib):
    """Update rewrites every cell: one that was known under the first parameters and falls back to Unknown under the second
    must not keep its old state"""
    from oracle import karto
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    cases = {(c.min_pass, c.threshold): c for c in oc.update_cases()}
    first = cases[(0, 0.0)]
    g = OccupancyGrid(first.width, first.height, first.offset, first.resolution)
    g.AddScans(hip_scans(first.scans), first.gates)
    order = [(0, 0.0), (3, 0.5), (2, 0.1), (3, 1.0), (0, 0.1), (2, 0.0)]
    states = []
    for mp, th in order:
        c = cases[(mp, th)]
        g.Update(mp, th)
        assert_grid_equals(g, karto.occupancy_from_scans(c.width, c.height, c.offset, c.resolution, oracle_scans(c.scans), c.gates, mp, th), c.name)
        states.append(g.cells().copy())
    assert ((states[0] != 0) & (states[1] == 0)).any() and ((states[0] == 100) & (states[1] == 255)).any()
    g.close()


def test_one_grid_over_calls_of_different_sizes(kartohip_lib, oracle_lib):
    """small call, a call 20 x larger (the staging buffers regrow), a smaller one, Clear, the first again: each state equals the
    oracle fed the same sequence"""
    from oracle import karto
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    w, h, off, res, steps = oc.reuse_steps()
    g = OccupancyGrid(w, h, off, res)
    fed, states = [], []
    for k, (op, scans) in enumerate(steps):
        if op == "clear":
            g.Clear()
            fed = []
        else:
            g.AddScans(hip_scans(scans), oc.GATES)
            fed = fed + list(scans)
        g.Update(2, 0.1)
        want = karto.occupancy_from_scans(w, h, off, res, oracle_scans(fed), oc.GATES, 2, 0.1)
        assert_grid_equals(g, want, f"step {k} ({op})")
        states.append(g.counters()[0].copy())
    assert not states[3].any() and np.array_equal(states[4], states[0]) and not np.array_equal(states[1], states[0])
    g.close()


def _write_bad_readings(ranges, laser):
    """NaN, +inf, readings under min_range, over the threshold and over max_range written into a copy of the queue"""
    r = ranges.copy()
    n = r.shape[1]
    for i in range(r.shape[0]):
        r[i, (7 * i) % n] = np.nan
        r[i, (7 * i + 300) % n:(7 * i + 300) % n + 5] = np.inf
        r[i, (11 * i + 500) % n] = laser.min_range
        r[i, (11 * i + 501) % n] = 0.03
        r[i, (13 * i + 640) % n] = laser.range_threshold
        r[i, (13 * i + 641) % n] = laser.range_threshold - 1e-06
        r[i, (13 * i + 642) % n] = np.nextafter(laser.range_threshold - 1e-06, 0.0)
        r[i, (13 * i + 643) % n] = 26.5
        r[i, (17 * i + 900) % n] = laser.max_range
        r[i, (17 * i + 901) % n] = np.nextafter(laser.max_range, 0.0)
        r[i, n - 1 - (i % 3)] = 24.0                                   # the last, partial run of 64 beams (1081 = 16 * 64 + 57)
    return r


def test_resident_trace_equals_the_oracle(kartohip_lib, oracle_lib):
    """kh_mapper_build_map (k_occ_trace_resident, fed from the mapper's resident scans) against the CPU oracle over the same scans
    pulled with kh_mapper_get_scan -- the oracle itself, not only the packed GPU path.  The same mapper as the single submap of a
    MapMerger under the identity (k_occ_trace_merged) gives the same grid: c = 1, s = 0, t = 0 is exact on every finite point, and
    the kept beams have finite points"""
    import test_localization_gpu as loc
    from oracle import karto
    from slam_toolbox_amd.mapper import Mapper
    from slam_toolbox_amd.merge import MapMerger
    from slam_toolbox_amd.occupancy_grid import compute_dimensions
    laser = synth.Laser()
    ranges, odom = loc._queue()
    ranges = _write_bad_readings(ranges[:120], laser)
    m = Mapper(laser, loop_search_maximum_distance=loc.LOOP_DIST)
    accepted = sum(int(m.Process(ranges[i], odom[i], 0.1 * i)[0]) for i in range(ranges.shape[0]))
    assert accepted >= 20
    pulled, oscans, n_bad = [], [], 0
    for i in m.alive():
        s, _ = m.scan(int(i))
        r = np.ctypeslib.as_array(s.ranges, (s.n,)).copy()
        pts = np.ctypeslib.as_array(s.points_xy, (2 * s.n,)).copy().reshape(-1, 2)
        kept = (r > laser.min_range) & (r < laser.max_range)
        assert np.isfinite(pts[kept]).all()
        n_bad += int((~np.isfinite(r)).sum())
        oscans.append(karto.Scan(r, np.array(s.sensor_pose[:]), points=pts))
        pulled.append((np.array(s.sensor_pose[:2]), r, pts))
    assert n_bad >= 6 * len(oscans), "the bad readings did not reach the stored scans"
    for res in (0.05, 0.013):
        g = m.build_map(res)
        w, h, off = compute_dimensions(hip_scans(pulled), laser.min_range, laser.range_threshold, res)
        assert (g.width, g.height) == (w, h) and np.array_equal(g.offset.view(np.uint64), off.view(np.uint64))
        want = karto.occupancy_from_scans(g.width, g.height, g.offset, res, oscans, laser, 2, 0.1)
        assert_grid_equals(g, want, f"resolution {res}")
        assert (want[0] == 100).sum() > 100 and (want[0] == 255).sum() > 10000
        mg = MapMerger(res)
        mg.add_submap(m)
        merged = mg.merge()
        assert (merged.width, merged.height, merged.width_step) == (g.width, g.height, g.width_step)
        assert np.array_equal(merged.offset.view(np.uint64), g.offset.view(np.uint64))
        for got, built in zip(merged.counters(), g.counters()):
            assert np.array_equal(got, built), f"resolution {res}: the merged counters differ from build_map's"
        assert np.array_equal(merged.cells(), g.cells())
        merged.close(); mg.close()
        g.close()
    m.close()
