"""tests/seq_cases.py on the CPU: every case of the fused-match edge table reaches the edge its probe names, by the oracle alone --
counts of readings, scans and points, the restated eligibility rules either side of each limit, usable query readings, distinct
first-point cells, tiles written, tie counts of the coarse and the fine volume, angle counts, the fine average on the lattice.  A case
moved off its edge (the 129-scan case made 128) fails here, without a GPU; tests/test_seq_edges_gpu.py then walks the same table."""
import numpy as np
import pytest

import seq_cases as sc
from common import PRESETS, bits

CASES = sc.cases()
BY_NAME = {c.name: c for c in CASES}
INVALID = np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def matchers(oracle_lib):
    cache = {}

    def get(case):
        key = case.geometry()
        if key not in cache:
            cache[key] = case.oracle_matcher()
        return cache[key]
    return get


_stage_cache = {}


def staged(matchers, case, pen, refine):
    key = (case.name, pen, refine)
    if key not in _stage_cache:
        _stage_cache[key] = sc.stages(matchers(case), case, pen, refine)
    return _stage_cache[key]


def test_table_is_complete():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.kind for c in CASES} == set(sc.KINDS)
    for _, seq in sc.SEQUENCES:
        assert all(n in BY_NAME for n in seq)
        assert len({BY_NAME[n].geometry() for n in seq}) == 1, "a sequence runs on one handle"
    for c in CASES:
        assert c.pairs and "reason" in c.probe


def test_preset_footprints(oracle_lib):
    """which presets have cells of 100 besides the centre (the order-dependent rule, a state byte per point): only S"""
    from common import make_oracle_matcher
    got = {p: sc.geometry(make_oracle_matcher(p))["n_foot"] for p in PRESETS}
    assert got == {"S": 4, "L": 0, "C2": 0, "K": 0}
    assert sc.geometry(make_oracle_matcher("L"))["kernel_size"] == 3          # below 8 x 8: the batch path's stamping kernel
    assert sc.geometry(make_oracle_matcher("C2"))["tiles"] == 127 * 127 < sc.MAX_TILES


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_eligibility_is_what_the_probe_says(matchers, case):
    geo = sc.geometry(matchers(case))
    assert sc.refusal(case, geo) == case.probe["reason"]
    limit = case.probe.get("limit")
    if limit == "query readings":
        assert case.query.n == case.probe["n"] and case.probe["n"] - sc.MAX_READINGS == (1 if case.probe["reason"] else 0)
    if limit == "base readings":
        assert max(b.n for b in case.base) == case.probe["n"] and case.probe["n"] - sc.MAX_READINGS == (1 if case.probe["reason"] else 0)
        assert case.query.n <= sc.MAX_READINGS
    if limit == "scans":
        assert case.n_scans() == case.probe["scans"] and len(case.base) == case.probe["listed"]
        assert case.probe["scans"] - sc.MAX_SCANS == (1 if case.probe["reason"] else 0)
        assert max(b.n for b in case.base) == 16
        if "empty_at" in case.probe:
            assert tuple(i for i, b in enumerate(case.base) if b.n == 0) == case.probe["empty_at"]
            assert case.base[0].n == 0 and case.base[-1].n == 0
        if "counts" in case.probe:
            nan_scans = [b for b in case.base if b.n > 0 and np.isnan(b.ranges).all()]
            assert len(nan_scans) == 1 and sum(1 for b in case.base if b.n == 0) == 1
            om = matchers(case)
            assert om.find_valid_points(nan_scans[0].oracle(), case.query.pose[:2]).shape[0] == 0
    if limit in ("points", "lds"):
        assert case.n_points() == case.probe["points"] and max(b.n for b in case.base) <= sc.MAX_READINGS and case.n_scans() <= sc.MAX_SCANS
        bytes_, bm_global, fits = sc.lds_plan(case.n_points(), geo)
        if limit == "points":
            assert case.probe["points"] - sc.MAX_POINTS == (1 if case.probe["reason"] else 0)
            assert sc.lds_plan(sc.MAX_POINTS, geo)[2], "the LDS rule must not bind before the point limit"
        else:
            assert geo["n_foot"] > 0 and case.n_points() <= sc.MAX_POINTS and bm_global == case.probe["bm_global"]
            assert fits == (case.probe["reason"] == 0)
            assert sc.lds_plan(case.n_points() - 1, geo)[2] and not sc.lds_plan(case.n_points() + (1 if fits else 0), geo)[2]
    if limit == "tiles":
        assert geo["tiles"] == case.probe["tiles"] and (geo["tiles"] > sc.MAX_TILES) == (case.probe["reason"] == 5)
        assert abs(geo["tiles"] - sc.MAX_TILES) <= 2 * 128 + 1            # the next grid size either way


def test_limit_pairs_are_neighbours():
    """N and N + 1 of every limit are both in the table"""
    by_limit = {}
    for c in CASES:
        if "limit" in c.probe:
            by_limit.setdefault(c.probe["limit"] + c.name[-4:] if c.probe["limit"] == "points" else c.probe["limit"], []).append(c.probe["reason"])
    for limit, reasons in by_limit.items():
        assert 0 in reasons and any(r != 0 for r in reasons), limit


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("slice readings", "slice valid")], ids=lambda c: c.name)
def test_query_slices(matchers, case):
    om = matchers(case)
    assert case.query.n == case.probe["readings"]
    st = staged(matchers, case, True, False)
    table = st["lookup"]
    assert table.shape[1] == case.query.n
    usable = int((table[0] != INVALID).sum())
    if case.kind == "slice readings":
        assert usable == case.query.n and case.query.n in (1, 63, 64, 65, 129)
    else:
        assert usable == case.probe["usable"] and usable in (1, 63, 64, 65, 129)
        bad = ~np.isfinite(case.query.ranges)
        assert bad[-25:].all() and np.isnan(case.query.ranges).any() and np.isinf(case.query.ranges).any()
        first_ok = np.nonzero(~bad)[0]
        assert bad[first_ok[0]:first_ok[-1] + 1].any() or usable == 1, "invalid readings between the usable ones"
        assert int((case.query.ranges[~bad] > case.create[3]).sum()) == case.probe["beyond_threshold"]
    assert (usable + sc.SLICE - 1) // sc.SLICE <= (case.query.n + sc.SLICE - 1) // sc.SLICE


def _first_cells(om, case):
    """distinct cells of the region of interest that FindValidPoints' readings of the base scans fall on"""
    q = case.query.oracle()
    om.add_scans(q, [])
    g = om.grid_info()
    cells = set()
    for b in case.base:
        if b.n == 0:
            continue
        pts = om.find_valid_points(b.oracle(), q.sensor_pose[:2])
        pts = pts[np.isfinite(pts).all(axis=1)]
        gx = np.array([sc.round_half_away(v) for v in (pts[:, 0] - g["offset_x"]) * g["scale"]], dtype=np.int64)
        gy = np.array([sc.round_half_away(v) for v in (pts[:, 1] - g["offset_y"]) * g["scale"]], dtype=np.int64)
        ok = (gx >= 0) & (gx < g["roi_w"]) & (gy >= 0) & (gy < g["roi_h"])
        cells.update(zip(gx[ok].tolist(), gy[ok].tolist()))
    return cells


def _tiles_written(om, grid):
    g = om.grid_info()
    ws = g["width_step"]
    a = grid.reshape(-1, ws)
    ty, tx = np.nonzero(a)
    return len(set(zip((ty // sc.TILE).tolist(), (tx // sc.TILE).tolist())))


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "candidates"], ids=lambda c: c.name)
def test_candidates(matchers, case):
    om = matchers(case)
    n = len(_first_cells(om, case))
    if "candidates" in case.probe:
        assert n == case.probe["candidates"] == 1 and case.n_scans() == 1
        st = staged(matchers, case, False, True)
        assert st["coarse_ties"] == 1 and st["fine_tie_cells"] > case.probe["fine_tie_cells_over"] and st["fine_on_lattice"]
        assert all(staged(matchers, case, pen, refine)["coarse_ties"] == 1 for pen, refine in case.pairs)
    else:
        assert n > case.probe["candidates_over"]
        assert sc.geometry(om)["n_foot"] == case.probe["n_foot"]


def test_clear_sequence(matchers):
    a, b = BY_NAME["clear a: over 2048 tiles written"], BY_NAME["clear b: one short scan elsewhere"]
    om = matchers(a)
    st_a = staged(matchers, a, True, True)
    assert _tiles_written(om, st_a["grid"]) > a.probe["tiles_over"] == sc.CLEAR_WAVES
    st_b = staged(matchers, b, True, True)
    assert 0 < _tiles_written(om, st_b["grid"]) <= b.probe["tiles_at_most"]
    assert dict(sc.SEQUENCES)["clear"] == (a.name, b.name, a.name)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("coarse ties", "tie cap", "expansion")], ids=lambda c: c.name)
def test_coarse_ties(matchers, case):
    for pen, refine in case.pairs:
        st = staged(matchers, case, pen, refine)
        want = case.probe["ties"]
        if want == "recorded":
            # with penalties the distance penalty separates the poses along the wall: what is left is recorded, not assumed
            assert 1 <= st["coarse_ties"] <= sc.TIE_CAP
            print(f"{case.name}: the oracle's coarse volume has {st['coarse_ties']} best poses")
        elif isinstance(want, tuple):
            assert want[0] <= st["coarse_ties"] <= want[1] and st["coarse_response"] > 0.5
            assert st["coarse_ties"] % sc.geometry(matchers(case))["nx"] == 0, "every x of the lattice ties"
        else:
            assert st["coarse_ties"] == want and st["coarse_response"] == 0.0
            assert st["coarse_shape"][0] * st["coarse_shape"][1] * st["coarse_shape"][2] == want
        if case.kind == "tie cap":
            assert st["coarse_shape"] == (case.probe["nx"], case.probe["nx"], case.probe["na"])
        if case.kind == "expansion":
            assert st["coarse_ties"] <= sc.TIE_CAP and st["expansions"] == (3 if case.probe["expansion"] else 0)
            assert case.n_scans() > 0 and st["grid"].any()
    if case.kind == "tie cap":
        assert not case.params["use_response_expansion"]


def test_tie_cap_neighbours():
    got = sorted(c.probe["ties"] for c in CASES if c.kind == "tie cap")
    assert got[0] == sc.TIE_CAP and got[1] > sc.TIE_CAP
    # no lattice nx * nx * na of more than one position lies between the cap and the nearest case above it
    assert not [(n, a) for n in range(2, 64) for a in range(1, 2049) if sc.TIE_CAP < n * n * a < got[1]]


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "fine lattice"], ids=lambda c: c.name)
def test_fine_lattice(matchers, case):
    st = staged(matchers, case, True, True)
    n = case.probe["fine_angles"]
    assert sc.fine_angles(case.params) == n
    assert st["lookup"].shape == (n, case.query.n) and st["fine_shape"] == (3, 3, n)
    assert (n * 9 <= sc.MAX_FINE) == case.probe["on_device"]
    assert st["coarse_ties"] == 1 and st["fine_on_lattice"], "the device's fine pass is taken iff the lattice fits"
    stats = sc.predict(sc.zero_stats(), case, sc.geometry(matchers(case)), st, True)
    assert (stats["fine_on_device"], stats["fine_fallbacks"]) == ((1, 0) if case.probe["on_device"] else (0, 1))


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "fine ties"], ids=lambda c: c.name)
def test_fine_ties(matchers, case):
    (pen, refine), = case.pairs
    st = staged(matchers, case, pen, refine)
    assert st["fine_ties"] > 1
    assert st["fine_on_lattice"] == case.probe["on_lattice"]
    if "fine_tie_cells_over" in case.probe:
        assert st["fine_tie_cells"] > case.probe["fine_tie_cells_over"] and st["coarse_ties"] > 1
    if case.probe.get("on_device"):
        assert st["coarse_ties"] == 1
        assert sc.predict(sc.zero_stats(), case, sc.geometry(matchers(case)), st, True)["fine_on_device"] == 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_stages_are_the_oracles_match_scan(matchers, case):
    """the pass-by-pass restatement the probes are read from gives ko_match_scan's own result, grid and table"""
    om = matchers(case)
    for pen, refine in case.pairs:
        st = staged(matchers, case, pen, refine)
        r, mean, cov = om.match_scan(case.query.oracle(), [b.oracle() for b in case.base], pen, refine)
        for o, s in zip((r, mean, cov), st["result"]):
            assert np.array_equal(bits(np.asarray(o)), bits(np.asarray(s)))
        assert np.array_equal(om.grid(), st["grid"]) and np.array_equal(om.lookup_table(), st["lookup"])


def test_every_fine_average_is_on_the_lattice(matchers):
    """no case of the table reaches finalize_job's off-lattice rescoring (seq_cases.fine_average_on_lattice says why)"""
    for case in CASES:
        for pen, refine in case.pairs:
            if refine:
                assert staged(matchers, case, pen, refine)["fine_on_lattice"], case.name
