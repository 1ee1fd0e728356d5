"""The matcher at smear-kernel sizes and grid pitches off the presets: every geometry of tests/geometry_cases.py
(tests/test_geometry_cases_oracle.py proves on the CPU that each sits where its name says, and that every read stays inside the
slot's allocation) on the device, compared with the CPU oracle for equality -- grid_info and kernel, the correlation grid on both
rasteriser routes and on slots 0 and 5 of a batch handle, a slot rasterised again with another scene, MatchScan on every scoring route,
MatchScanBatch of 8 on a max_batch = 8 handle (where bshift 3 against 5 is decided), CorrelateScan at two cells, and the smear limits of
kh_matcher_create.  Every test prints kernel_size, n_foot, ws, bshift and the route it took.

FOUND with the table (no defect of the library; geometry_cases / DESIGN.md section 3b): at an even side (search 0.63, resolution
0.01: 64 cells) MatchScan's coarse lattice has round(31.5) + 1 = 33 poses two cells apart, one more than the probability grid holds, and
the reference throws "Unable to find best position".  The library answers KH_ERR_SEARCH on every route, as the oracle and the
reference do; that geometry and its neighbour (side 65) are also matched by a one-cell CorrelateScan over the whole search space.

That the table bites was shown with four one-line mutants that change values only off the presets, built into one library and run
once against this file (26 of 137 cases fail) and against tests/test_matcher_gpu.py, test_raster_corner_cases_gpu.py and
test_seq_edges_gpu.py (91 pass: blind to all four):
* k_raster_tile: the second point of a wave pass dropped at k = 5 -- every test of `k5`;
* k_raster_tile_reg: j_hi one row short at k = 9, and kseq_tile: a footprint that reaches a band with its last row only left out at
  k = 9 -- every test of `k9` and `k9 coarse` (both rasterisers);
* k_raster_bin and kseq_bin: the last block column of a footprint not marked when bshift = 3 and the half kernel is >= 10 cells --
  test_batch_of_eight of `k21 narrow` and `k25`, and only since the query has readings that land behind the walls by the half kernel
  and 8 to 15 cells (windows that touch a footprint's rim alone): with readings on the walls and far away only, no case noticed."""
import numpy as np
import pytest

import geometry_cases as gc
import lds_cases as lc
import test_geometry_cases_oracle as tg
from common import bits

pytestmark = pytest.mark.gpu

GEOS = [g for g in gc.GEOMETRIES if not g.last]
LAST = [g for g in gc.GEOMETRIES if g.last]
FAILED = tg.FAILED


def _same(a, b, what):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert np.array_equal(bits(a), bits(b)), f"{what}: {a} vs {b}"


def _same_result(want, got, tag):
    for what, o, h in zip(("response", "mean", "covariance"), want, got):
        _same(o, h, f"{what}, {tag}")


def _say(geo, max_batch, route):
    p = geo.probe
    print(f"[{geo.name}] kernel_size {p['kernel_size']} n_foot {p['n_foot']} ws {p['ws']} height {p['height']} side {p['side']} "
          f"max_batch {max_batch} bshift {p['bshift8'] if max_batch >= 8 else p['bshift1']}: {route}")


def _throws(geo):
    return geo.name == "side 64"


# ---------------------------------------------------------------- create
def check_create(geo):
    om = geo.oracle_matcher()
    for mb in (1, 8):
        hm = geo.hip_matcher(max_batch=mb)
        try:
            g, want = hm.grid_info(), om.grid_info()
            ints = [k for k in want if not k.startswith("offset")]
            assert {k: g[k] for k in ints} == {k: want[k] for k in ints} and g["search_side"] == geo.probe["side"]
            assert np.array_equal(hm.kernel(), om.kernel())
            assert all(hm.grid_info(slot=s) == g for s in range(mb))
            _say(geo, mb, "create")
        finally:
            hm.close()


# ---------------------------------------------------------------- rasterisation
RASTER_SEQUENCE = (("table", 0), ("table", gc.SHIFT_CELLS), ("hash", 0), ("hash", gc.SHIFT_CELLS), ("table", 0), ("hash", gc.SHIFT_CELLS), ("table", gc.SHIFT_CELLS))


def check_raster(geo):
    """AddScans on both rasteriser routes, every call after another scene on the same slot (Grid::Clear from the tile list: each
    route's clear after each route's stamps); slot 0 of a plain handle, slots 0 and 5 of a batch handle"""
    om = geo.oracle_matcher()
    want = {}
    for raster, shift in set(RASTER_SEQUENCE):
        sc = tg.scene_of(geo, shift)
        om.add_scans(sc.query.oracle(), [b.oracle() for b in sc.bases(raster)])
        want[(raster, shift)] = om.grid()
    assert len({w.tobytes() for w in want.values()}) == 4
    for mb, slots in ((1, (0,)), (8, (0, 5))):
        hm = geo.hip_matcher(max_batch=mb)
        try:
            for raster, shift in RASTER_SEQUENCE:
                sc = tg.scene_of(geo, shift)
                hq, hb = sc.query.hip(), [b.hip() for b in sc.bases(raster)]
                for slot in slots:
                    hm.AddScans(hq, hb, slot=slot)
                om.add_scans(sc.query.oracle(), [])
                for slot in slots:
                    g = hm.grid_info(slot=slot)
                    assert {k: g[k] for k in om.grid_info()} == om.grid_info()
                    got = hm.GetCorrelationGrid(slot=slot)
                    bad = np.nonzero(got != want[(raster, shift)])[0]
                    assert bad.size == 0, f"{geo.name}: grid of slot {slot} (max_batch {mb}) after {raster} / shift {shift}: {bad.size} bytes differ, first at {bad[:4]}"
            assert all(not hm.GetCorrelationGrid(slot=s).any() for s in range(mb) if s not in slots)
            _say(geo, mb, f"rasterised {len(RASTER_SEQUENCE)} times per slot {slots}: table and hash, clear with{'' if gc.clear_tail(gc.derive(geo.create)) else 'out'} tail")
        finally:
            hm.close()


# ---------------------------------------------------------------- MatchScan on every scoring route
def _expected(geo, params, raster):
    """the oracle's MatchScan per (penalize, refine) with grid and lookup table, and the coarse pass's volume and probabilities"""
    sc = tg.scene_of(geo)
    om = geo.oracle_matcher(params)
    q, base = sc.query.oracle(), [b.oracle() for b in sc.bases(raster)]
    out = {}
    for pen, refine in gc.FLAGS:
        res = om.match_scan(q, base, pen, refine)
        out[(pen, refine)] = dict(result=res, grid=om.grid(), lookup=om.lookup_table())
    # (False, False) ran last: the coarse pass alone
    out["volume"] = om.volume()[..., 0].copy()
    out["probs"] = om.probs()
    return out


def check_match(geo, scoring):
    from slam_toolbox_amd.scan_matcher import MapperParams
    sc = tg.scene_of(geo)
    n_calls = 0
    hm = geo.hip_matcher()
    try:
        for pname, params in geo.params_sets():
            hm.SetParams(MapperParams(**params))
            for raster in gc.RASTER:
                want = _expected(geo, params, raster)
                hq, hb = sc.query.hip(), [b.hip() for b in sc.bases(raster)]
                hm.set_debug(False, **gc.debug_bits(scoring))
                before = hm.seq_stats()
                for pen, refine in gc.FLAGS:
                    tag = f"{geo.name} / {pname} / {raster} / {scoring} (pen={pen} refine={refine})"
                    w = want[(pen, refine)]
                    if _throws(geo):
                        assert w["result"][0] == FAILED
                        with pytest.raises(RuntimeError, match="Unable to find best position"):
                            hm.MatchScan(hq, hb, pen, refine)
                    else:
                        _same_result(w["result"], hm.MatchScan(hq, hb, pen, refine), tag)
                        assert np.array_equal(w["lookup"], hm.lookup_table()), f"lookup table, {tag}"
                    assert np.array_equal(w["grid"], hm.GetCorrelationGrid()), f"grid, {tag}"
                    n_calls += 1
                after = hm.seq_stats()
                route = gc.route(scoring, raster, len(gc.FLAGS))
                got = {k: after[k] - before[k] for k in ("calls", "fused_score", "ineligible")}
                assert got == {k: route[k] for k in got} and after["fine_mismatches"] == 0, f"route of {geo.name} / {raster} / {scoring}: {after}"
                if route["ineligible"]:
                    assert after["ineligible_reason"] == route["ineligible_reason"]
                _say(geo, 1, f"MatchScan {pname} {raster} {scoring}: seq_stats +{got}, reason {after['ineligible_reason']}")
                if scoring == "fused" or _throws(geo):
                    continue
                # the coarse pass's volume and search-space probabilities (keeping them takes the call off the fused path: reason 1)
                hm.set_debug(True, **gc.debug_bits(scoring))
                _same_result(want[(False, False)]["result"], hm.MatchScan(hq, hb, False, False), f"{geo.name} / {raster} / {scoring}, volume kept")
                _, resp = hm.volume()
                assert np.array_equal(bits(want["volume"]), bits(resp)), f"response volume, {geo.name} / {raster} / {scoring}"
                lattice = hm.search_probabilities()
                _same(want["volume"].max(axis=2), lattice, "search-space probabilities vs the oracle's volume")
                side = geo.probe["side"]
                if side % 2 == 1:
                    probs = np.zeros((side, side))
                    probs[::2, ::2] = lattice
                    _same(want["probs"], probs, "search-space probabilities vs the oracle's probs()")
    finally:
        hm.close()
    assert n_calls == len(geo.params_sets()) * len(gc.RASTER) * len(gc.FLAGS)


# ---------------------------------------------------------------- public CorrelateScan calls, and the LDS route confirmed
def check_correlate(geo):
    """the coarse search and the geometry's CorrelateScan calls (two cells on k = 9 / 21: no copies are built at these sizes, the
    result alone is asserted; one cell over the whole search space on the 64 | 65 pair) on the windowed and the LDS-staged kernels.
    With dense scoring and profiling on, kh_matcher_score_loads reads what lds_cases.predict() derives where prepare_job's rule
    sends the search down the LDS path: the route is the predicted one."""
    sc = tg.scene_of(geo)
    om = geo.oracle_matcher()
    oq, ob = sc.query.oracle(), [b.oracle() for b in sc.base]
    hq, hb = sc.query.hip(), [b.hip() for b in sc.base]
    searches = [("coarse", gc.coarse_args(geo, gc.PARAMS))] + tg.correlate_calls(geo)
    handles = {}
    try:
        for route in ("windowed", "lds"):
            for mb in (1, 8):
                hm = handles[(route, mb)] = geo.hip_matcher(max_batch=mb)
                hm.set_debug(True, dense_score=True, **{route + "_score": True})
                hm.profile(True)
                hm.AddScans(hq, hb)
        om.add_scans(oq, ob)
        for tag, (off, step, ang_off, ang_res) in searches:
            for pen in (True, False):
                want = om.correlate_scan(oq, oq.sensor_pose, off, step, ang_off, ang_res, pen, False)
                if want[0] == FAILED:
                    assert _throws(geo) and tag == "coarse"
                    continue
                vol, table = om.volume()[..., 0], om.lookup_table()
                cl = lc.classify(om, gc.Search(sc.query, sc.query.pose, ang_off, ang_res))
                lds, loads = lc.predict(None, cl, lc.chunks(None, cl))
                assert gc.copies(dict(cl["lat"], na=cl["na"]), cl["P"]) == 0
                for (route, mb), hm in handles.items():
                    hm.score_loads()
                    got = hm.CorrelateScan(hq, sc.query.pose, off, step, ang_off, ang_res, pen, None, False)
                    n = hm.score_loads()
                    what = f"{geo.name} / {tag} / {route} / max_batch {mb} (pen={pen})"
                    _same_result(want, got, what)
                    assert np.array_equal(table, hm.lookup_table()), f"lookup table, {what}"
                    assert np.array_equal(bits(vol), bits(hm.volume()[1])), f"response volume, {what}"
                    if route == "lds" and lds:
                        assert n == loads, f"{what}: not the LDS-staged route ({n} loads, {loads} predicted)"
                    took = "LDS-staged" if (route == "lds" and lds) else "windowed"
                    _say(geo, mb, f"CorrelateScan {tag} {cl['lat']['nx']} x {cl['lat']['ny']} x {cl['na']} step {cl['lat']['sx']}: {took}, {n} loads, no copies")
    finally:
        for hm in handles.values():
            hm.close()


# ---------------------------------------------------------------- batches of 8 on a max_batch = 8 handle
def check_batch(geo):
    sc = tg.scene_of(geo)
    om = geo.oracle_matcher()
    ob = [b.oracle() for b in sc.base]
    hb = [b.hip() for b in sc.base]
    queries = [sc.query_at(i) for i in range(8)]
    hqs = [q.hip() for q in queries]
    hm = geo.hip_matcher(max_batch=8)
    try:
        for pen, refine in gc.FLAGS:
            want = [om.match_scan(q.oracle(), ob, pen, refine) for q in queries]
            resp, means, covs, status = hm.MatchScanBatch(hqs, [hb] * 8, pen, refine)
            if _throws(geo):
                assert all(w[0] == FAILED for w in want) and (status != 0).all()
                continue
            assert (status == 0).all()
            for i in range(8):
                tag = f"{geo.name}, job {i} of the batch (pen={pen} refine={refine})"
                _same_result(want[i], (resp[i], means[i], covs[i]), tag + " vs oracle")
                single = hm.MatchScan(hqs[i], hb, pen, refine)
                _same_result(single, (resp[i], means[i], covs[i]), tag + " vs a single match on the same handle")
        _say(geo, 8, "MatchScanBatch of 8 == 8 single matches == oracle")
        # the same as eight coarse searches in ONE CorrelateScanBatch (and, on the 64 | 65 pair, eight one-cell searches)
        for tag, (off, step, ang_off, ang_res) in [("coarse", gc.coarse_args(geo, gc.PARAMS))] + [c for c in tg.correlate_calls(geo) if c[0] == "one_cell"]:
            if tag == "coarse" and _throws(geo):
                continue
            for i in range(8):
                hm.AddScans(hqs[i], hb, slot=i)
            centres = np.array([q.pose for q in queries])
            resp, means, covs, status = hm.CorrelateScanBatch(hqs, centres, off, step, ang_off, ang_res, True, False)
            assert (status == 0).all()
            for i, q in enumerate(queries):
                oq = q.oracle()
                om.add_scans(oq, ob)
                want = om.correlate_scan(oq, oq.sensor_pose, off, step, ang_off, ang_res, True, False)
                _same_result(want, (resp[i], means[i], covs[i]), f"{geo.name}, {tag} search {i} of the batch vs oracle")
                assert np.array_equal(om.grid(), hm.GetCorrelationGrid(slot=i))
                single = hm.CorrelateScan(hqs[i], q.pose, off, step, ang_off, ang_res, True, None, False, slot=i)
                _same_result(single, (resp[i], means[i], covs[i]), f"{geo.name}, {tag} search {i} of the batch vs a single search")
            _say(geo, 8, f"CorrelateScanBatch of 8 {tag} searches == 8 single searches == oracle")
    finally:
        hm.close()


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_create(kartohip_lib, geo):
    check_create(geo)


@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_rasterise_both_routes_and_again(kartohip_lib, geo):
    check_raster(geo)


@pytest.mark.parametrize("scoring", gc.SCORING)
@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_match_scan(kartohip_lib, geo, scoring):
    check_match(geo, scoring)


@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_correlate_scan_and_lds_route(kartohip_lib, geo):
    check_correlate(geo)


@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_batch_of_eight(kartohip_lib, geo):
    check_batch(geo)


def test_create_limits_on_the_library(kartohip_lib):
    """the four smear values at the limits give a handle or None exactly as the oracle does, and a valid create straight after a
    refusal works"""
    from oracle import karto
    from slam_toolbox_amd.scan_matcher import MapperParams, ScanMatcher
    res = tg.LIMIT_RES
    for smear, ok in tg.smear_limits():
        try:
            karto.Matcher(10 * res, res, smear, 1.0, gc.PARAMS)
            oracle_ok = True
        except ValueError:
            oracle_ok = False
        hm = ScanMatcher.Create(MapperParams(**gc.PARAMS), 10 * res, res, smear, 1.0)
        assert (hm is not None) == oracle_ok == ok, smear
        if hm is not None:
            assert hm.grid_info()["kernel_size"] == (3 if smear < res else 41)
            hm.close()
        else:
            again = ScanMatcher.Create(MapperParams(**gc.PARAMS), 10 * res, res, 0.5 * res, 1.0)
            assert again is not None and again.grid_info()["kernel_size"] == 3
            again.close()


def test_one_raster_tile_narrower_than_a_window_row(kartohip_lib):
    """ws 56, 51 rows: the extreme geometry, last in the file (tests/test_geometry_cases_oracle.py::
    test_every_read_stays_inside_the_allocation has the in-bounds argument for it)"""
    geo, = LAST
    check_create(geo)
    check_raster(geo)
    for scoring in gc.SCORING:
        check_match(geo, scoring)
    check_correlate(geo)
    check_batch(geo)
