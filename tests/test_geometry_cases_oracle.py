"""tests/geometry_cases.py on the CPU: every geometry of the table sits where its name says (probe == the restated formulas of
kh_matcher_create == what the CPU oracle's matcher reports), its scene is no trivial one, every read of the scoring kernels stays
inside the slot's allocation (the address arithmetic restated over the oracle's lookup table and lattice), and the CPU oracle itself
equals the reference there -- live where oracle/_ref is built, and everywhere against the recordings of
tests/golden/make_golden_ref_checks.py in tests/golden/ref_checks.npz.  tests/test_geometry_gpu.py then walks the table on the device."""
import math

import numpy as np
import pytest

import geometry_cases as gc
import lds_cases as lc
from common import LASER, bits, ref_digest, ref_recorded, ref_row
from oracle import ref

LIVE = ref.available()
GEOS = gc.GEOMETRIES
FAILED = -1e9               # the oracle's and the reference driver's answer where the reference throws


def slug(s):
    return s.replace(" ", "_")


# ---------------------------------------------------------------- the calls of a geometry, shared with the generator of the recordings
def one_cell_args(geo):
    """CorrelateScan over the whole search space at one cell: side x side poses (the 64 | 65 pair)"""
    d = gc.derive(geo.create)
    res = 1.0 / (1.0 / geo.create[1])
    off = 0.5 * (float(d["side"]) - 1) * res
    return (off, off), (res, res), 0.06, 0.03


def two_cell_args(geo):
    """CorrelateScan at two cells on a lattice of 11 x 15 poses, 9 angles"""
    res = 1.0 / (1.0 / geo.create[1])
    return (10 * res, 14 * res), (2 * res, 2 * res), 0.08, 0.02


def correlate_calls(geo):
    """[(tag, args)] of the public CorrelateScan calls the geometry is given besides MatchScan"""
    out = []
    if geo.name in ("side 64", "side 65"):
        out.append(("one_cell", one_cell_args(geo)))
    if geo.two_cells:
        out.append(("two_cells", two_cell_args(geo)))
    return out


def calls(geo):
    """every recorded call of a geometry: (key, name of the params set, kind, argument)"""
    out = []
    for pname, params in geo.params_sets():
        for pen, refine in gc.FLAGS:
            out.append((f"geo_{slug(geo.name)}_{pname}_match_{int(pen)}{int(refine)}", pname, "match", (pen, refine)))
    for tag, args in correlate_calls(geo):
        for pen in (True, False):
            out.append((f"geo_{slug(geo.name)}_K_{tag}_{int(pen)}", "K", "correlate", args + (pen,)))
    return out


def run_call(m, kind, arg, q, base):
    """one call on an oracle or reference matcher (they share the method names)"""
    if kind == "match":
        return m.match_scan(q, base, *arg)
    off, res, ang_off, ang_res, pen = arg
    m.add_scans(q, base)
    centre = np.array(q.sensor_pose() if hasattr(q.sensor_pose, "__call__") else q.sensor_pose, dtype=np.float64)
    return m.correlate_scan(q, centre, off, res, ang_off, ang_res, pen, False)


def ref_scans(scene):
    return ref.RefScan(scene.query.ranges, scene.query.pose), [ref.RefScan(b.ranges, b.pose) for b in scene.base]


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def recorded(oracle_lib):
    if LIVE:
        ref.init_laser(gc.laser())
    yield ref_recorded()
    if LIVE:
        ref.init_laser(LASER)


_scenes = {}


def scene_of(geo, shift=0):
    if (geo.name, shift) not in _scenes:
        _scenes[(geo.name, shift)] = gc.Scene(geo, shift)
    return _scenes[(geo.name, shift)]


# ---------------------------------------------------------------- the table
def test_table_is_complete():
    names = [g.name for g in GEOS]
    assert len(set(names)) == len(names) and GEOS[-1].last and sum(g.last for g in GEOS) == 1
    ks = {g.probe["kernel_size"] for g in GEOS}
    assert {3, 5, 7, 9, 13, 21, 25, 27, 41} <= ks
    assert {(g.probe["kernel_size"], g.probe["n_foot"]) for g in GEOS if g.probe["kernel_size"] == 41} == {(41, 0), (41, 4)}
    # the >= 8 dispatch from both sides; the bshift rule from both sides of both of its limits
    assert max(k for k in ks if k < 8) == 7 and min(k for k in ks if k >= 8) == 9
    for a, b in gc.PAIRS[:2]:
        pa, pb = gc.BY_NAME[a].probe, gc.BY_NAME[b].probe
        assert (pa["bshift8"], pb["bshift8"]) == (3, 5) and pa["bshift1"] == pb["bshift1"] == 5
    assert (gc.BY_NAME["k25"].probe["kernel_size"], gc.BY_NAME["k27"].probe["kernel_size"]) == (25, 27)
    assert (gc.BY_NAME["side 64"].probe["side"], gc.BY_NAME["side 65"].probe["side"]) == (64, 65)
    a, b = (gc.derive(gc.BY_NAME[n].create) for n in gc.PAIRS[2])
    assert (a["ws"], a["height"]) == (b["ws"], b["height"]), "n_foot 0 | 4 on the same grid"
    # pitches: one raster tile; under two; under the 64-byte window row; under kLdsPitch; every residue of ws mod 64 that has a tail
    wss = {g.probe["ws"] for g in GEOS}
    assert {56, 96, 120, 144, 184, 240, 248, 264, 280} == wss
    assert min(g.probe["tiles"] for g in GEOS) == 1 and any(g.probe["ws"] < 2 * gc.TILE and g.probe["ws"] > gc.TILE for g in GEOS)
    assert any(g.probe["ws"] < lc.TILE_BYTES for g in GEOS) and any(lc.TILE_BYTES < g.probe["ws"] < lc.LDS_PITCH for g in GEOS)
    assert {g.probe["ws"] for g in GEOS if gc.clear_tail(gc.derive(g.create))} >= {56, 120, 184, 248, 280}
    assert sum(g.offline for g in GEOS) == 2 and {g.name for g in GEOS if g.two_cells} == {"k9", "k21 narrow"}
    d = gc.derive(gc.BY_NAME["pad 7"].create)
    assert d["ws"] - d["width"] == 7
    d = gc.derive(gc.BY_NAME["k21 narrow"].create)
    assert (d["side"], d["roi"]) == (31, 91)
    d = gc.derive(gc.BY_NAME["k41 small"].create)
    assert 3 * d["kernel_size"] > d["ws"] and d["tiles"] == 4


def test_half_away_case_is_exact():
    _, res, smear, _ = gc.BY_NAME["k7 half away"].create
    assert 2.0 * smear / res == 2.5 and math.floor(2.5 + 0.5) == 3 and round(2.5) == 2, "banker's rounding would give k = 5"
    assert gc.BY_NAME["k7 half away"].probe["kernel_size"] == 7


@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_probe_is_what_create_derives(oracle_lib, geo):
    d = gc.derive(geo.create)
    assert {k: d[k] for k in gc.PROBE_KEYS} == geo.probe
    om = geo.oracle_matcher()
    g = om.grid_info()
    kern = om.kernel()
    assert (g["kernel_size"], g["width_step"], g["height"], g["width"], g["data_size"]) == (d["kernel_size"], d["ws"], d["height"], d["width"], d["data_size"])
    assert (g["roi_x"], g["roi_y"], g["roi_w"], g["roi_h"]) == (d["border"], d["border"], d["roi"], d["roi"])
    assert om.probs().shape[0] == d["side"]
    assert int((kern == 100).sum()) - 1 == d["n_foot"] and np.array_equal(kern, gc.kernel_values(geo.create[2], 1.0 / g["scale"]))
    assert d["tiles"] == ((d["ws"] + 63) // 64) * ((d["height"] + 63) // 64) <= 16384
    assert d["grid_pad"] >= d["pad"] + gc.GRID_PAD and d["grid_pad"] % 256 == 0


# ---------------------------------------------------------------- the scenes
_coarse = {}


def coarse_of(geo):
    """oracle matcher after AddScans + coarse search of the table scene: (matcher, result, classes)"""
    if geo.name not in _coarse:
        om = geo.oracle_matcher()
        sc = scene_of(geo)
        out, search = gc.run_coarse(om, geo, sc)
        _coarse[geo.name] = (om, out, lc.classify(om, search), search)
    return _coarse[geo.name]


@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_scene_is_not_trivial(oracle_lib, geo):
    sc = scene_of(geo)
    d = gc.derive(geo.create)
    om = geo.oracle_matcher()
    q, base = sc.query.oracle(), [b.oracle() for b in sc.base]
    r, mean, _ = om.match_scan(q, base, True, True)
    grid = om.grid()
    assert int((grid == 100).sum()) >= 50
    if geo.name == "side 64":
        # an even side: the coarse lattice of MatchScan (offset 0.5 * (side - 1) cells, steps of two) has round(31.5) + 1 = 33 poses,
        # the last one cell behind the probability grid -- the reference throws (Mapper.cpp:786-796).  The geometry is matched by a
        # one-cell CorrelateScan over the whole search space instead (64 x 64 poses).
        assert r == FAILED and om.volume().shape[:2] == (33, 33)
        r, mean, _ = run_call(om, "correlate", one_cell_args(geo) + (True,), q, base)
        assert om.volume().shape[:2] == (64, 64)
    assert 0.5 < r < 1.0
    # the far readings: finite, scored, off the array -- with the row wrap of the one-dimensional index
    far = np.arange(gc.N_BEAMS)[4::gc.FAR_EVERY]
    assert np.isfinite(sc.query.ranges).all() and (sc.query.ranges[far] >= 3.0 * sc.rt).all() and far.size == 20
    om, _, cl, _ = coarse_of(geo)
    lat = cl["lat"]
    grid = om.grid()
    table = om.lookup_table().astype(np.int64)
    pose = lat["base0"] + (np.arange(lat["nx"]) * lat["sx"])[None, :] + (np.arange(lat["ny"]) * lat["sy_ws"])[:, None]
    at = pose[None, :, :, None] + table[:, None, None, far]                     # (angle, y, x, far reading)
    outside = (at < 0) | (at >= d["data_size"])
    assert outside.any()
    col = (lat["base0"] % d["ws"]) + (np.arange(lat["nx"]) * lat["sx"])[None, None, :, None] + cl["gx"][:, None, None, far]
    wrapped = ~outside & ((col < 0) | (col >= d["ws"]))
    if d["ws"] <= gc.NARROW:
        rows_with_stamps = grid.reshape(d["height"], d["ws"]).any(axis=1)
        assert wrapped.any() and rows_with_stamps[at[wrapped] // d["ws"]].any(), "a far reading wraps into a row that holds stamps"
    # the fringe readings: windows that hold nothing but the outermost cells of some footprints
    if d["kernel_size"] >= 21:
        fringe = np.arange(gc.N_BEAMS)[1::gc.FAR_EVERY]
        at = pose[None, :, :, None] + table[:, None, None, fringe]
        inside = (at >= 0).all(axis=(1, 2)) & (at < d["data_size"]).all(axis=(1, 2))            # (angle, fringe reading)
        top = np.where(inside[:, None, None, :], grid[np.clip(at, 0, d["data_size"] - 1)], 0).max(axis=(1, 2))
        assert ((top > 0) & (top <= 20)).sum() >= 3, "windows that touch a footprint's rim only"
    # the second scene of a slot, and the hash route's input
    om2 = geo.oracle_matcher()
    s2 = scene_of(geo, gc.SHIFT_CELLS)
    om2.add_scans(s2.query.oracle(), [b.oracle() for b in s2.base])
    g2 = om2.grid()
    assert g2.any() and (grid[g2 == 0] != 0).sum() >= 50, "bytes of the first scene the second one must clear"
    assert max(b.n for b in sc.bases("hash")) == gc.MAX_READINGS + 1 and max(b.n for b in sc.bases("table")) == gc.N_BEAMS
    assert np.isnan(sc.long.ranges[400:]).all() and np.isfinite(sc.long.ranges[:400]).all()
    for scene, table_grid in ((sc, grid), (s2, g2)):
        om2.add_scans(scene.query.oracle(), [b.oracle() for b in scene.bases("hash")])
        assert ((om2.grid() != 0) & (table_grid == 0)).any(), "the long scan adds stamps of its own: four different grids per geometry"


# ---------------------------------------------------------------- every read inside the allocation
def _searches(geo):
    """(name, classes, Search-like, beams) of the searches the GPU file runs on the geometry: the coarse and the fine pass of MatchScan
    and the public CorrelateScan calls"""
    om, out, cl, search = coarse_of(geo)
    sc = scene_of(geo)
    yield "coarse", cl
    q = sc.query.oracle()
    res = 1.0 / (1.0 / geo.create[1])
    if out[0] != FAILED:
        om.correlate_scan(q, out[1].copy(), (res, res), (res, res), 0.5 * gc.PARAMS["coarse_angle_resolution"], gc.PARAMS["fine_search_angle_offset"],
                          True, True, cov_in=out[2])
        yield "fine", lc.classify(om, gc.Search(sc.query, out[1], 0.5 * gc.PARAMS["coarse_angle_resolution"], gc.PARAMS["fine_search_angle_offset"]))
    for tag, (off, step, ang_off, ang_res) in correlate_calls(geo):
        om.correlate_scan(q, q.sensor_pose, off, step, ang_off, ang_res, True, False)
        yield tag, lc.classify(om, gc.Search(sc.query, sc.query.pose, ang_off, ang_res))
    gc.run_coarse(om, geo, sc)         # (the cached matcher is left on its coarse search)


@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_every_read_stays_inside_the_allocation(oracle_lib, geo):
    """the in-bounds argument of geometry_cases' docstring, per search: fast windows of k_score and kseq_score, the LDS regions of
    K3', and the rule that keeps the copies off"""
    d = gc.derive(geo.create)
    lo_ok, hi_ok = -d["grid_pad"], d["data_size"] + d["grid_pad"]
    seen = []
    for name, cl in _searches(geo):
        lat = cl["lat"]
        assert lat["linear"], name
        assert gc.copies(dict(lat, na=cl["na"]), cl["P"]) == 0, "no search of the table allocates copies of the grid"
        assert (cl["cls"] == lc.FAST).any()
        one_tile = (lat["nx"] - 1) * lat["sx"] + 1 <= gc.TILE_SPAN
        if one_tile:
            for masked in (True, False):
                lo, hi = gc.score_reads(cl, d, masked)
                assert lo_ok <= lo and hi < hi_ok, (name, masked, lo, hi)
                # the fast rule alone gives the bound: 3 bytes in front of -pad, 63 behind data_size + pad
                assert lo >= -d["pad"] - 3 and hi < d["data_size"] + d["pad"] + 64
        else:
            # several tile columns (the one-cell search of 64 | 65 poses): k_score's lanes stop at the window's last pose
            start = lat["base0"] + cl["gx"] + cl["gy"] * lat["ws"]
            start = start[cl["cls"] == lc.FAST]
            assert start.min() - 3 >= lo_ok and start.max() + (lat["nx"] - 1) * lat["sx"] + (lat["ny"] - 1) * lat["sy_ws"] + 3 < hi_ok
        lds = all(lc.lds_rule(lat, cl["P"]).values())
        assert lds == (one_tile and lat["ny"] <= lc.MAX_ROWS)
        if lds:
            ch = lc.chunks(None, cl)
            lo, hi = lc.region_bounds(cl, ch)
            assert lo >= lo_ok and hi < hi_ok, (name, lo, hi)
            assert all(c["rows"] <= lc.LDS_ROWS and c["x_extent"] <= lc.LDS_PITCH for waves in ch["groups"] for lst in waves for c in lst)
        seen.append(name)
    assert seen[0] == "coarse" and ("fine" in seen or geo.name == "side 64")
    if d["ws"] < lc.TILE_BYTES:
        # the extreme case: a 64-byte window row is longer than a grid row, a staged row of 192 bytes spans more than three
        assert d["ws"] * 3 < lc.LDS_PITCH and d["pad_rows"] * d["ws"] > 512


# ---------------------------------------------------------------- the oracle against the reference
def _same_row(a, b):
    assert np.array_equal(bits(a), bits(b)), (a, b)


def test_old_recordings_are_unchanged(recorded):
    """the entries the reference check had before the geometry table: same keys, same bytes (sha256 over keys, dtypes, shapes, bytes)"""
    import hashlib
    old = sorted(k for k in recorded.files if not k.startswith("geo_"))
    h = hashlib.sha256()
    for k in old:
        a = recorded[k]
        h.update(k.encode() + str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes())
    assert len(old) == OLD_ENTRIES[0] and h.hexdigest() == OLD_ENTRIES[1]


OLD_ENTRIES = (39, "bbda6d319948b803935f6753c4c8e9fa84295f7834e4e40210817bbc14047efb")          # (count, digest) of the entries recorded before this table


@pytest.mark.parametrize("geo", GEOS, ids=repr)
def test_oracle_equals_reference(recorded, geo):
    sc = scene_of(geo)
    oq, ob = sc.query.oracle(), [b.oracle() for b in sc.base]
    if LIVE:
        rq, rb = ref_scans(sc)
    for pname, params in geo.params_sets():
        mo = geo.oracle_matcher(params)
        if LIVE:
            mr = ref.RefMatcher(*geo.create, params)
            assert np.array_equal(mr.kernel(), mo.kernel()) and mr.grid_info() == mo.grid_info()
        for key, p, kind, arg in calls(geo):
            if p != pname:
                continue
            b = run_call(mo, kind, arg, oq, ob)
            lt = mo.lookup_table()
            throws = geo.name == "side 64" and kind == "match"
            assert (b[0] == FAILED) == throws
            if LIVE:
                a = run_call(mr, kind, arg, rq, rb)
                assert np.array_equal(bits(a[0]), bits(b[0]))
                assert np.array_equal(mr.grid(), mo.grid())
                assert np.array_equal(mr.lookup_table(*lt.shape), lt)
                if not throws:
                    assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2]))
                    _same_row(ref_row(a), recorded[key])
            if not throws:
                _same_row(ref_row(b), recorded[key])
            else:
                assert recorded[key][0] == FAILED
            assert ref_digest(mo.grid()) == str(recorded[key + "_grid"])
            assert ref_digest(lt) == str(recorded[key + "_lut"])


# ---------------------------------------------------------------- create limits
LIMIT_RES = 2.0 ** -5


def smear_limits():
    """(smear, accepted) at a resolution that is a power of two: 0.5 * res and 10 * res are exact doubles"""
    lo, hi = 0.5 * LIMIT_RES, 10 * LIMIT_RES
    return ((lo, True), (hi, True), (math.nextafter(lo, 0.0), False), (math.nextafter(hi, math.inf), False))


def test_create_limits_on_the_oracle(oracle_lib):
    from oracle import karto
    assert 1.0 / (1.0 / LIMIT_RES) == LIMIT_RES
    for smear, ok in smear_limits():
        assert gc.accepted(LIMIT_RES, smear) == ok
        if ok:
            m = karto.Matcher(10 * LIMIT_RES, LIMIT_RES, smear, 1.0, gc.PARAMS)
            assert m.grid_info()["kernel_size"] == (3 if smear < LIMIT_RES else 41)
        else:
            with pytest.raises(ValueError):
                karto.Matcher(10 * LIMIT_RES, LIMIT_RES, smear, 1.0, gc.PARAMS)
        if LIVE:
            if ok:
                ref.RefMatcher(10 * LIMIT_RES, LIMIT_RES, smear, 1.0, gc.PARAMS)
            else:
                with pytest.raises(ValueError):
                    ref.RefMatcher(10 * LIMIT_RES, LIMIT_RES, smear, 1.0, gc.PARAMS)
