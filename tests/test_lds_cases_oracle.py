"""tests/lds_cases.py on the CPU: every case of the table sits on the edge its probe names, shown by the restated rules of the path
(lds_cases.classify / chunks / predict) over the CPU oracle's lookup table and lattice -- the lattice the search arguments give, which
condition of prepare_job's lds_ok fails just past a limit, descriptor lists exactly full, one chunk of 64 windows in one class, the
tail remainders of every class for every way K3' deals the steps, unions exactly at the region's limits and split one cell further,
the fallback's slow entries, the classes at the array's edges.  A case moved off its edge fails here, without a GPU;
tests/test_lds_edges_gpu.py then walks the same table on the device."""
import numpy as np
import pytest

import lds_cases as lc

CASES = lc.cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def matchers(oracle_lib):
    cache = {}

    def get(case):
        if case.geometry() not in cache:
            cache[case.geometry()] = case.oracle_matcher()
        return cache[case.geometry()]
    return get


_built = {}


def built(matchers, case):
    """(classes, chunks) of the case, from the oracle's search"""
    if case.name not in _built:
        om = matchers(case)
        lc.run_oracle(om, case, True)
        cl = lc.classify(om, case)
        _built[case.name] = (cl, lc.chunks(case, cl))
    return _built[case.name]


def all_chunks(ch, angle_pair=None):
    groups = ch["groups"] if angle_pair is None else [ch["groups"][angle_pair]]
    return [d for waves in groups for lst in waves for d in lst]


def test_table_is_complete():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.kind for c in CASES} == set(lc.KINDS)
    assert all(c.probe and "lds" in c.probe and c.pens and c.dense[0] is True for c in CASES)
    lattices = {(c.want[0], c.want[1], c.want[2]) for c in CASES if c.kind in ("lattice", "past the limit")}
    for s, nxs, nys in ((1, (2, 60, 61, 62), (1, 16, 17, 31, 32, 33, 63, 64, 65)), (2, (30, 31, 32), (16, 17, 32, 33, 64))):
        assert set(nxs) <= {l[0] for l in lattices if l[2] == s} and set(nys) <= {l[1] for l in lattices if l[2] == s}
    assert all(l[0] != l[1] for l in lattices if l != (61, 61, 1)), "non-square lattices: a transposed index must show"
    assert {c.probe["na"] for c in CASES if c.kind == "angles"} == {1, 2, 3, 9}
    assert {c.probe["P"] for c in CASES if c.kind == "beams"} == {1, 63, 64, 65, 255, 256, 257, 1025, 2047, 2048}
    assert sorted(c.probe["only"] for c in CASES if c.kind == "past the limit") == ["P", "nx", "nx", "ny"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_search_and_route_are_what_the_case_says(matchers, case):
    """the search arguments give the lattice the case names, linear, and prepare_job's rule sends it where the probe says -- past a
    limit, only the named condition fails"""
    cl, ch = built(matchers, case)
    lat = cl["lat"]
    nx, ny, s, na = case.want
    assert (lat["nx"], lat["ny"], cl["na"], cl["P"]) == (nx, ny, na, case.query.n)
    assert lat["linear"] and lat["sx"] == (s if nx > 1 else 1) and lat["sy_cells"] == (s if ny > 1 else 1)
    rule = lc.lds_rule(lat, cl["P"])
    lds, loads = lc.predict(case, cl, ch)
    assert lds == case.probe["lds"]
    if not lds:
        assert [k for k, ok in rule.items() if not ok] == [case.probe["only"]]
        limit = dict(nx=(lat["nx"] - 1) * lat["sx"] + 1 - lc.TILE_SPAN, ny=lat["ny"] - lc.MAX_ROWS, P=cl["P"] - lc.MAX_BEAMS)[case.probe["only"]]
        assert limit == (2 if (case.probe["only"] == "nx" and s == 2) else 1), "just past the limit"
        assert loads > 0
    for k in ("nx", "ny", "sx"):
        if k in case.probe:
            assert lat[k] == case.probe[k]
    # no list of descriptors can overflow, and every region lies inside the slot's allocation (lds_cases.region_bounds)
    cap = lc.lds_desc_capacity(cl["P"])
    assert all(len(lst) <= cap for waves in ch["groups"] for lst in waves)
    if not lds:
        return
    assert all(d["rows"] <= lc.LDS_ROWS and d["x_extent"] <= lc.LDS_PITCH and d["windows"] <= 64 * lc.GROUP_ANGLES for d in all_chunks(ch))
    lo, hi = lc.region_bounds(cl, ch)
    grid_pad = ((lc.pad_rows(lat["side"]) * lat["ws"] + 255) // 256) * 256 + lc.GRID_PAD          # kh_matcher_create: m->grid_pad
    assert lo >= -grid_pad and hi < lat["data_size"] + grid_pad
    # every fast window is in exactly one chunk or went to the slow list through the fallback
    n_fast = int((cl["cls"] == lc.FAST).sum())
    assert sum(d["windows"] for d in all_chunks(ch)) + len(ch["fallbacks"]) == n_fast
    assert sum(ch["n_slow"]) == int((cl["cls"] == lc.SLOW).sum()) + len(ch["fallbacks"])


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "lattice"], ids=lambda c: c.name)
def test_lattice_rows_and_waves(matchers, case):
    cl, ch = built(matchers, case)
    ny = cl["lat"]["ny"]
    assert ch["row_waves"] == (1 if ny <= 16 else 2 if ny <= 32 else 4)
    assert ch["read_rows"] == (16 * ch["row_waves"] - 1) * cl["lat"]["sy_cells"] + 1 <= lc.LDS_ROWS
    # a realistic scan: several chunks per angle pair, windows in every class, tails among them
    counts = np.array([d["cnt"] for d in all_chunks(ch)])
    assert len(all_chunks(ch, 0)) > 1 and (counts.sum(axis=(0, 1)) > 0).all() and (counts % 4 != 0).any()


def test_row_wave_thresholds_are_in_the_table():
    """16 | 17 and 32 | 33 rows, for both steps; 31 rows is the kernel comment's two-wave case"""
    for s in (1, 2):
        nys = {c.want[1] for c in CASES if c.kind == "lattice" and c.want[2] == s}
        assert {16, 17, 32, 33} <= nys
    assert lc.lds_row_waves(31) == 2 and any(c.want[1] == 31 and c.want[2] == 1 for c in CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "angles"], ids=lambda c: c.name)
def test_angles(matchers, case):
    cl, ch = built(matchers, case)
    na = case.probe["na"]
    assert cl["na"] == na and len(ch["groups"]) == (na + 1) // 2
    last = all_chunks(ch, len(ch["groups"]) - 1)
    dead = all(sum(d["cnt"][1]) == 0 for d in last)
    assert dead == case.probe["dead_angle"] == (na % 2 == 1) and all(sum(d["cnt"][0]) > 0 for d in last)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("beams", "invalid runs")], ids=lambda c: c.name)
def test_beams_and_invalid_runs(matchers, case):
    cl, ch = built(matchers, case)
    n = cl["P"]
    waves = ch["groups"][0]
    if case.kind == "beams":
        assert n == case.probe["P"] and (cl["cls"] == lc.FAST).all()
        # the beams' builder waves and rounds: beam i belongs to wave (i >> 6) & 3
        for w, lst in enumerate(waves):
            assert all(((d["beam_begin"] >> 6) & 3) == w and ((d["beam_begin"] + d["beams"] - 1) >> 6) == (d["beam_begin"] >> 6) for d in lst)
        assert sum(d["beams"] for d in all_chunks(ch, 0)) == n
        assert [bool(lst) for lst in waves] == [n > 64 * w for w in range(4)]
        return
    invalid = cl["cls"][0] == lc.INVALID
    assert np.isnan(case.query.ranges).any() and np.isinf(case.query.ranges).any()
    if "empty_runs" in case.probe:
        for lo in case.probe["empty_runs"]:
            assert invalid[lo:lo + 64].all() and not invalid[lo - 1] and not invalid[lo + 64]
            assert not [d for d in all_chunks(ch, 0) if lo <= d["beam_begin"] < lo + 64]
        assert all(waves)
    if "empty_wave" in case.probe:
        w = case.probe["empty_wave"]
        assert not waves[w] and all(lst for k, lst in enumerate(waves) if k != w)
        assert all(invalid[i] == (((i >> 6) & 3) == w) for i in range(n))
    if case.probe.get("no_chunk"):
        assert invalid.all() and not all_chunks(ch) and lc.predict(case, cl, ch) == (True, 0)
        assert cl["lat"]["nx"] * cl["lat"]["ny"] * cl["na"] > case.probe["ties_over"] == lc.TIE_CAP, "every pose ties at 0: more than the tie list holds"


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "chunk per beam"], ids=lambda c: c.name)
def test_descriptor_capacity_exactly_full(matchers, case):
    cl, ch = built(matchers, case)
    cap = lc.lds_desc_capacity(cl["P"])
    assert cl["P"] % 256 == 0 and cap == cl["P"] // 4
    for waves in ch["groups"]:
        assert [len(lst) for lst in waves] == [cap] * lc.LDS_RANGES
    assert all(d["beams"] == 1 and d["windows"] == 2 for d in all_chunks(ch))


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "one chunk"], ids=lambda c: c.name)
def test_one_chunk_of_full_steps(matchers, case):
    cl, ch = built(matchers, case)
    d, = all_chunks(ch)
    for q in range(2):
        assert sorted(d["cnt"][q]) == [0, 0, 0, case.probe["one_chunk"]], "64 windows in a single class: 16 full steps, no tail"
    assert d["beams"] == 64 and d["rows"] == (cl["lat"]["ny"] - 1) + 1


def _steps(cnt):
    return sum((c + 3) // 4 for c in cnt)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "tails"], ids=lambda c: c.name)
def test_tails_of_every_class(matchers, case):
    """every class has chunks with 1, 2 and 3 windows left over, and (where the waves of an angle deal the steps among them) the running
    step number enters classes and chunks at a phase other than 0"""
    cl, ch = built(matchers, case)
    parts = 4 // ch["row_waves"]
    assert parts == case.probe["parts"]
    for g in range(len(ch["groups"])):
        lst = all_chunks(ch, g)
        assert len(lst) == 4
        for q in range(2):
            if 2 * g + q >= cl["na"]:
                continue
            rem = [{d["cnt"][q][c] % 4 for d in lst} for c in range(4)]
            assert all({1, 2, 3} <= r for r in rem), rem
            if parts > 1:
                # phases of the running step number at the start of every class of every chunk, and of every chunk
                step, class_phases, chunk_phases = 0, set(), set()
                for d in lst:
                    chunk_phases.add(step % parts)
                    for c in range(4):
                        class_phases.add(step % parts)
                        step += (d["cnt"][q][c] + 3) // 4
                assert class_phases == set(range(parts)), "step_base enters a class at every phase"
                assert len(chunk_phases) > 1, "step_base carries across chunks"
                assert all(_steps(d["cnt"][q]) % parts != 0 for d in lst)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "tails"], ids=lambda c: c.name)
def test_every_step_is_dealt_once_whatever_step_base_is(matchers, case):
    """the waves that share an angle's rows take every step of every class exactly once -- with the running step number in the
    formula and without it: step_base balances the waves' work, it decides no sum (why the mutant that drops it is equivalent)"""
    cl, ch = built(matchers, case)
    parts = 4 // ch["row_waves"]
    counts = [d["cnt"][0] for d in all_chunks(ch, 0)]
    n_steps = sum(_steps(c) for c in counts)
    for with_base in (True, False):
        taken = lc.deal(counts, parts, with_base)
        assert len(taken) == n_steps and all(len(w) == 1 for w in taken.values())
    if parts > 1:
        load = lambda t: sorted(sum(1 for w in t.values() if w == [p]) for p in range(parts))
        assert load(lc.deal(counts, parts, True))[-1] <= load(lc.deal(counts, parts, False))[-1], "what step_base is for: the busiest wave has less to do"


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("region x", "region y")], ids=lambda c: c.name)
def test_region_limits(matchers, case):
    cl, ch = built(matchers, case)
    lst = all_chunks(ch)
    assert cl["P"] == 2 and len(lst) == case.probe["n_chunks"]
    if case.kind == "region x":
        assert lst[0]["al"] == case.probe["al"]
        if case.probe["n_chunks"] == 1:
            assert lst[0]["x_extent"] == case.probe["x_extent"] == lc.LDS_PITCH, "chunk extent == limit at this value"
        else:
            other = BY_NAME[case.name.replace(", one further", "")]
            assert case.query.ranges[1] - other.query.ranges[1] == pytest.approx(lc.CELL) and case.query.ranges[0] == other.query.ranges[0]
    else:
        assert ch["read_rows"] == case.probe["read_rows"]
        if case.probe["n_chunks"] == 1:
            assert lst[0]["y_extent"] == case.probe["y_extent"] == lc.LDS_ROWS
        else:
            other = BY_NAME[case.name.replace(", one further", "")]
            assert case.query.ranges[1] - other.query.ranges[1] == pytest.approx(lc.CELL) and case.query.ranges[0] == other.query.ranges[0]


def test_region_limit_pairs():
    for kind in ("region x", "region y"):
        names = [c.name for c in CASES if c.kind == kind]
        assert all((n + ", one further") in names for n in names if not n.endswith("one further"))
    assert {c.probe["al"] for c in CASES if c.kind == "region x"} == {0, 15}
    assert {c.probe["read_rows"] for c in CASES if c.kind == "region y"} == {16, 32, 64}


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "fallback"], ids=lambda c: c.name)
def test_fallback(matchers, case):
    cl, ch = built(matchers, case)
    assert (cl["cls"] == lc.FAST).all(), "no entry is slow by itself: the slow entries are the fallback's"
    assert tuple(ch["n_slow"]) == case.probe["n_slow"] and ch["fallbacks"] == case.probe["fallbacks"]
    (a, beam), = ch["fallbacks"]
    assert abs(int(cl["gy"][a, beam]) - int(cl["gy"][a - 1, beam])) + ch["read_rows"] > lc.LDS_ROWS
    first_of_run = beam % 64 == 0
    assert first_of_run == ("at 64" in case.name)
    # the beam's other window is in a chunk; in a group whose second angle is dead the far beam needs no fallback
    assert any(d["beam_begin"] <= beam < d["beam_begin"] + d["beams"] for d in all_chunks(ch, 0))
    if cl["na"] == 3:
        assert cl["cls"][2, beam] == lc.FAST and not [f for f in ch["fallbacks"] if f[0] == 2]


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "array edges"], ids=lambda c: c.name)
def test_array_edges(matchers, case):
    cl, ch = built(matchers, case)
    lat = cl["lat"]
    assert case.dense == (True, False), "kept despite the block map: with and without dense_score"
    idx = lat["base0"] + cl["gx"] + cl["gy"] * lat["ws"]
    bspan = (lat["nx"] - 1) * lat["sx"] + (lat["ny"] - 1) * lat["sy_ws"]
    fast = cl["cls"] == lc.FAST
    if "classes" in case.probe:
        assert set(np.unique(cl["cls"]).tolist()) == case.probe["classes"]
        assert lat["ny"] > lc.pad_rows(lat["side"]), "a window taller than the pad: the only way to a slow entry through the pad"
        slow = cl["cls"] == lc.SLOW
        if case.probe["outside"] == "front":
            assert (fast & (idx < 0)).any() and (idx[fast] >= -lat["pad"]).all(), "windows that start in the zero rows in front and stay fast"
            assert (idx[slow] < -lat["pad"]).all() and (idx[slow] + bspan >= 0).all()
            assert (idx[cl["cls"] == lc.OFF] + bspan < 0).all()
        else:
            assert (fast & (idx + bspan >= lat["data_size"])).any() and (idx[fast] + bspan < lat["data_size"] + lat["pad"]).all()
            assert (idx[slow] + bspan >= lat["data_size"] + lat["pad"]).all() and (idx[slow] < lat["data_size"]).all()
            assert (idx[cl["cls"] == lc.OFF] >= lat["data_size"]).all()
        assert tuple(ch["n_slow"]) == tuple(int(slow[a].sum()) for a in range(cl["na"])) and min(ch["n_slow"]) > 0
    if case.probe.get("wraps"):
        wx0 = idx % lat["ws"]
        xs = (lat["nx"] - 1) * lat["sx"] + 1
        assert fast.all() and (wx0 + xs > lat["ws"]).sum() >= 10 and (wx0 + xs <= lat["ws"]).sum() >= 10
        assert (cl["gx"] + lat["base0"] % lat["ws"] >= lat["ws"]).any(), "and windows wholly behind the row end: in the next row, as the linear index has it"


@pytest.mark.parametrize("n", [7, 8, 9])
def test_batches(matchers, n):
    jobs = lc.batch_jobs(n)
    assert [j.query.n for j in jobs[:3]] == list(lc.BATCH_BEAMS) and len({j.args()[1:] for j in jobs}) == 1
    assert (n >= 8) == (n in (8, 9)) and 8 * ((n + 7) // 8) - n == {7: 1, 8: 0, 9: 7}[n]      # launch_score_lds: the XCD mapping and its empty job slots
    for j in jobs[:3]:
        cl, ch = built(matchers, j)
        assert lc.predict(j, cl, ch)[0] and cl["lat"]["linear"]


def test_decimated_copies_then_a_small_two_cell_search(matchers):
    """group G: the large search gives a slot column-decimated copies; the small ones are two-cell searches the windowed kernel would
    score from the copies as sx = 1 jobs (dec) and the LDS path can take; the batch's jobs take it with no debug bit set -- and get
    the copies by themselves"""
    large, small, jobs = lc.decimated_cases()

    def lat_of(case):
        cl, ch = built(matchers, case)
        return dict(cl["lat"], na=cl["na"]), cl, ch
    lat, cl, _ = lat_of(large)
    assert lc.copies_kind(lat, cl["P"]) == 2 == large.probe["copies"]
    lat, cl, ch = lat_of(small)
    assert lc.copies_kind(lat, cl["P"]) == 0 and lc.dec_rule(lat, 2) and not lc.dec_rule(lat, 0) and lc.predict(small, cl, ch)[0]
    assert not lc.lds_by_default(lat, cl["P"], 1)
    assert len(jobs) == lc.DEFAULT_BATCH and len({j.args()[1:] for j in jobs}) == 1
    for j in jobs[:2]:
        lat, cl, ch = lat_of(j)
        assert lc.lds_by_default(lat, cl["P"], len(jobs)) and not lc.lds_by_default(lat, cl["P"], len(jobs) - 1)
        assert lc.copies_kind(lat, cl["P"]) == 2 and lc.dec_rule(lat, 2) and lc.predict(j, cl, ch)[0]
