"""CPU: the case tables of tests/occupancy_cases.py, tests/lifelong_cases.py and tests/graph_cases.py run through the ORACLES alone
(oracle/occupancy_oracle.c, oracle/lifelong.py, oracle/loops.py, tests/near_by_rule.py).  Each check asserts that a case reaches the edge its name says -- a border
row really is crossed, a cell really sits at pass == min_pass -- so that editing a number cannot quietly turn an edge case
into an ordinary one.  The GPU side of the same tables: tests/test_occupancy_edges_gpu.py, tests/test_lifelong_edges_gpu.py,
tests/test_graph_edges_gpu.py."""
import numpy as np
import pytest

import graph_cases as gc
import lifelong_cases as lc
import near_by_rule
import occupancy_cases as oc
from oracle import karto, lifelong, loops

OCC = list(oc.all_cases())
LIFE = list(lc.all_cases())
LOOPS = list(gc.loop_cases())
NEAR = list(gc.near_cases())


def oracle_scans(scans):
    """[(sensor_xy, ranges, points)] -> oracle scans: ranges and points set independently (karto.Scan(..., points=...))"""
    return [karto.Scan(r, np.array([s[0], s[1], 0.0]), points=p) for s, r, p in scans]


def run_oracle(case):
    return karto.occupancy_from_scans(case.width, case.height, case.offset, case.resolution, oracle_scans(case.scans), case.gates,
                                      case.min_pass, case.threshold)


def test_case_names_are_unique():
    for cases in (OCC, LIFE, LOOPS, NEAR):
        names = [c.name for c in cases]
        assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", OCC, ids=[c.name for c in OCC])
def test_occupancy_case_reaches_its_edge(oracle_lib, case):
    cells, p, hits = run_oracle(case)
    w, h, ws, probe = case.width, case.height, oc.align8(case.width), case.probe
    assert p.shape == (h, ws)
    for a in (cells, p, hits):
        assert not a[:, w:].any(), "padding columns are never written"
    assert (hits <= p).all() and (2 * hits.astype(np.int64) <= p).all()
    for _, r, pts in case.scans:
        kept = (r > case.gates.min_range) & (r < case.gates.max_range)
        assert np.isfinite(pts[kept]).all(), "a kept beam with a non-finite point walks 2^31 cells"
        assert (np.abs((pts[kept] - np.asarray(case.offset)) / case.resolution) < 1e6).all()
    if probe.get("borders"):
        for name, line in (("bottom row", p[0, :w]), ("top row", p[h - 1, :w]), ("left column", p[:, 0]), ("right column", p[:, w - 1])):
            assert line.any(), f"{name} is never crossed"
        assert p[0, 0] and p[0, w - 1] and p[h - 1, 0] and p[h - 1, w - 1], "a corner is never crossed"
    if probe.get("no_hits"):
        assert p.any() and not hits.any()
    if probe.get("all_zero"):
        assert not p.any() and not hits.any() and not cells.any()
    if probe.get("some_hits"):
        assert hits.any() and (p > hits).any()
    for x, y in probe.get("passed", []):
        assert p[y, x] > 0 and hits[y, x] == 0, f"the beam clipped at ({x}, {y}) ends without a hit"
    for (x, y), (want_p, want_h) in probe.get("counts", {}).items():
        assert (p[y, x], hits[y, x]) == (want_p, want_h), f"cell ({x}, {y})"
    if "beams" in probe:
        assert sum(r.size for _, r, _ in case.scans) == probe["beams"]


def _star_by_bresenham(case):
    """the counters of a star of beams from the second restatement of TraceLine (occupancy_cases.bresenham)"""
    w, h = case.width, case.height
    p, hits = np.zeros((h, oc.align8(w)), dtype=np.uint32), np.zeros((h, oc.align8(w)), dtype=np.uint32)
    c = case.probe["star"]
    for radius in (0, 1, 2, 7, 40):
        for ex, ey in oc.ring(c, radius):
            for x, y in oc.bresenham(c[0], c[1], ex, ey):
                if 0 <= x < w and 0 <= y < h:
                    p[y, x] += 1
            if 0 <= ex < w and 0 <= ey < h:
                p[ey, ex] += 1
                hits[ey, ex] += 1
    return p, hits


@pytest.mark.parametrize("case", [c for c in OCC if "star" in c.probe], ids=lambda c: c.name)
def test_star_of_beams_equals_a_second_bresenham(oracle_lib, case):
    _, p, hits = run_oracle(case)
    want_p, want_h = _star_by_bresenham(case)
    assert np.array_equal(p, want_p) and np.array_equal(hits, want_h)
    c = case.probe["star"]
    n_beams = sum(r.size for _, r, _ in case.scans)
    assert n_beams == 1 + 8 + 16 + 56 + 320 and p[c[1], c[0]] == n_beams + 1      # every beam leaves the sensor's cell; radius 0 ends in it
    dx = np.array([abs(e[0] - c[0]) for e in oc.ring(c, 7)])
    dy = np.array([abs(e[1] - c[1]) for e in oc.ring(c, 7)])
    assert (dx == dy).sum() == 4 and (dx == 0).sum() == 2 and (dy == 0).sum() == 2 and (dx > dy).any() and (dy > dx).any()


def test_range_gate_rows(oracle_lib):
    case = next(c for c in OCC if c.name == "gates: one beam per gate value")
    _, p, hits = run_oracle(case)
    rows, sx = case.probe["gate_rows"], case.probe["sensor_x"]
    assert len(rows) == len(oc.gate_values()) == 18
    for label, (y, kept, hit) in rows.items():
        assert bool(p[y].any()) is kept, label
        assert bool(hits[y].any()) is hit, label
        assert not p[y - 1].any() and not p[y + 1].any()         # the rows between the beams stay empty
        if kept:
            assert p[y, sx] == 1, label
    end = lambda label: int(np.flatnonzero(p[rows[label][0]])[-1])      # noqa: E731
    # 20 m = 320 cells: everything at or over the threshold stops there, whatever its reading says
    for label in ("range_threshold", "between threshold and max_range", "below max_range", "below range_threshold",
                  "range_threshold - 1e-6", "below range_threshold - 1e-6", "above range_threshold - 1e-6"):
        assert end(label) == sx + 320, label
    # the narrow grid cuts those beams off at its right edge: no hit, but the walk up to the edge is counted
    narrow = next(c for c in OCC if c.name == "gates: clipped beams in a narrow grid")
    _, p2, h2 = run_oracle(narrow)
    y = rows["between threshold and max_range"][0]
    assert p2[y, narrow.width - 1] == 1 and not h2[y].any() and np.array_equal(p2[:, :narrow.width], p[:, :narrow.width])


@pytest.mark.parametrize("case", [c for c in OCC if c.probe.get("update")], ids=lambda c: c.name)
def test_update_cells_sit_on_the_comparisons(oracle_lib, case):
    cells, p, hits = run_oracle(case)
    mp, th = case.min_pass, case.threshold
    for (x, y), (cp, ch) in oc.UPDATE_COUNTS.items():
        assert cells[y, x] == oc.expected_state(cp, ch, mp, th), (x, y, cp, ch)
    counts = set(oc.UPDATE_COUNTS.values())
    # a cell exactly at pass == min_pass (Unknown) and its twin with one more pass (known)
    at = [c for c in oc.UPDATE_COUNTS if oc.UPDATE_COUNTS[c][0] == mp]
    over = [c for c in oc.UPDATE_COUNTS if oc.UPDATE_COUNTS[c][0] == mp + 1]
    assert at and over
    assert all(cells[y, x] == 0 for x, y in at) and all(cells[y, x] != 0 for x, y in over)
    # a known cell exactly at hits / pass == threshold is Free; its twin with one more hit and the same passes is Occupied.
    # (hits / pass cannot exceed 0.5, so at 0.5 and 1.0 there is no such twin: nothing is Occupied there)
    on = [(cp, ch) for cp, ch in counts if cp > mp and ch / cp == th]
    if th <= 0.5:
        assert on, "no cell at the threshold"
        for cp, ch in on:
            x, y = next(c for c, v in oc.UPDATE_COUNTS.items() if v == (cp, ch))
            assert cells[y, x] == 255
    if th < 0.5:
        twins = [(cp, ch) for cp, ch in on if (cp, ch + 1) in counts]
        assert twins
        for cp, ch in twins:
            x, y = next(c for c, v in oc.UPDATE_COUNTS.items() if v == (cp, ch + 1))
            assert cells[y, x] == 100
    else:
        assert not (cells == 100).any()


def test_oracle_reproduces_the_reference_on_the_range_gates(oracle_lib):
    """tests/golden/occupancy_edges.npz: the REFERENCE's OccupancyGrid::CreateFromScans on scans whose readings sit on every
    gate (tests/golden/make_golden_occupancy_edges.py); the oracle must give its counters and cells"""
    import os
    from common import LASER
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "occupancy_edges.npz"))
    w, h, ws = (int(v) for v in G["dims"])
    cells, p, hits = np.zeros(ws * h, dtype=np.uint8), np.zeros(ws * h, dtype=np.uint32), np.zeros(ws * h, dtype=np.uint32)
    cells[G["cells_idx"]] = G["cells_val"]
    p[G["count_idx"]] = G["pass_val"]
    hits[G["count_idx"]] = G["hit_val"]
    ranges = G["ranges"]
    gates = oc.Gates(LASER.min_range, LASER.range_threshold, LASER.max_range)
    for label, v, _, _ in oc.gate_values(gates):
        n = np.isnan(ranges).sum(axis=1) if np.isnan(v) else (ranges == v).sum(axis=1)
        assert (n >= 2).all(), f"the recorded scans do not hold the reading '{label}'"
    scans = [karto.Scan(ranges[k], G["poses"][k], LASER) for k in range(ranges.shape[0])]
    c, op, oh = karto.occupancy_from_scans(w, h, G["offset"], float(G["resolution"]), scans, LASER)
    assert np.array_equal(op.reshape(-1), p) and np.array_equal(oh.reshape(-1), hits) and np.array_equal(c.reshape(-1), cells)
    assert (c == 100).sum() > 500 and (c == 255).sum() > 2000
    # one reading each way across `range_threshold - 1e-6` moves one hit: the recording can tell the two comparisons apart
    edge = gates.range_threshold - 1e-06
    for wrong in (np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf)):
        moved = ranges.copy()
        moved[ranges == edge] = wrong
        _, _, mh = karto.occupancy_from_scans(w, h, G["offset"], float(G["resolution"]),
                                              [karto.Scan(moved[k], G["poses"][k], LASER) for k in range(ranges.shape[0])], LASER)
        assert (mh.sum() != hits.sum()) == (wrong < edge)


def test_reuse_sequence_grows_and_shrinks(oracle_lib):
    w, h, off, res, steps = oc.reuse_steps()
    sizes = [sum(r.size for _, r, _ in arg) if op == "add" else None for op, arg in steps]
    assert sizes[1] == 20 * sizes[0] and sizes[2] < sizes[0] and sizes[3] is None and sizes[4] == sizes[0]
    _, p, hits = karto.occupancy_from_scans(w, h, off, res, oracle_scans(steps[0][1]), oc.GATES)
    assert p.any() and hits.any()


@pytest.mark.parametrize("case", LIFE, ids=[c.name for c in LIFE])
def test_lifelong_case_sits_on_its_edge(case):
    for c in case.candidates:
        assert c.bbox_size[0] * c.bbox_size[1] > 0.0, "zero-area boxes are out of scope"
    out = lifelong.compute_scores(case.reference, case.candidates, case.params)
    assert all(a.shape == (len(case.candidates),) for a in out)
    if case.check is not None:
        with np.errstate(invalid="ignore"):
            case.check(*out)


def test_resident_form_of_the_cases_holds_the_same_readings():
    """lifelong_cases.to_resident: the flagged readings are the candidate's own, in order; the decoys behind cleared flags lie
    strictly inside the intersection wherever there is one, so an ignored mask bit changes the count; the bounds case and every
    decision case reach all three scan lengths, and the 1081-reading form uses the last, partial mask word"""
    res = list(lc.resident_cases())
    names = {(case.name, n_scan) for case, n_scan, _, _ in res}
    for case in LIFE:
        if case.name.startswith(("decision", "geometry")):
            assert all((case.name, n) in names for n in lc.RESIDENT_N_SCAN), case.name
    assert ("launch: 1000 candidates", 1081) in names and ("launch: 4 candidates", 1081) in names
    decoys_inside = last_word = 0
    for case, n_scan, readings, passed in res:
        for c, r, flag in zip(case.candidates, readings, passed):
            assert r.shape == (n_scan, 2) and flag.shape == (n_scan,) and np.isfinite(r).all()
            assert np.array_equal(r[flag], c.points)
            x_l, x_u, y_l, y_u = lifelong.intersect_bounds(case.reference, c)
            d = r[~flag]
            decoys_inside += int(((d[:, 0] < x_u) & (d[:, 0] > x_l) & (d[:, 1] < y_u) & (d[:, 1] > y_l)).sum())
            last_word += int(n_scan == 1081 and flag[1024:].any())
    assert decoys_inside > 10000 and last_word > 100
    bounds = next(c for c in LIFE if c.name == "geometry: readings on the four bounds and one ulp inside")
    for n_scan in lc.RESIDENT_N_SCAN:
        assert lc.to_resident(bounds, n_scan) is not None


def test_lifelong_launch_shapes_are_all_there():
    names = [c.name for c in LIFE]
    for n in lc.CANDIDATE_COUNTS:
        assert f"launch: {n} candidates" in names
    assert lc.call_sizes(300, 7)[:4] == [1, 1000, 2, 500] and len(lc.call_sizes(300, 7)) == 300
    # the bulk generator reaches every branch of the score: dropped, kept with its own score, matched (-1), objective, clamped
    ref, cands = lc.bulk(1000, (5, 0, 64, 1, 130, 63, 65), salt=1000)
    kept, iou, area, reading, score = lifelong.compute_scores(ref, cands, lifelong.DecayParams())
    own = np.array([c.score for c in cands])
    assert (~kept).sum() > 50 and (kept & (score == own)).sum() > 50 and (kept & (score != own)).sum() > 50
    assert (score == 1.0).any() and (score < 0.0).any() and np.isnan(reading).any()


def test_finite_twins_guard_every_case_with_nan_points(oracle_lib):
    """every case that carries a non-finite point has a twin with none, and the twin's dropped beams would be SEEN if kept (they
    point 1 m along +x into or across the grid: the twin's oracle result differs once `r <= min_range` lets min_range through)"""
    guarded = [c for c in OCC if oc.finite_twin(c) is not None]
    assert {c.name for c in guarded} >= {"gates: one beam per gate value", "gates: all readings in one scan", "shapes: every beam of the call dropped"}
    for c in guarded:
        t = oc.finite_twin(c)
        assert all(np.isfinite(p).all() for _, _, p in t.scans)
        assert all(np.array_equal(a, b, equal_nan=True) for (_, a, _), (_, b, _) in zip(c.scans, t.scans))
        same = [np.array_equal(x, y) for x, y in zip(run_oracle(c), run_oracle(t))]
        assert all(same), "dropped beams do not depend on their points"
        lenient = t._replace(gates=oc.Gates(np.nextafter(t.gates.min_range, 0.0), t.gates.range_threshold, t.gates.max_range))
        assert not np.array_equal(run_oracle(lenient)[1], run_oracle(t)[1]), c.name


def loop_oracle(case):
    starts = case.starts if case.starts is not None else [0] * len(case.queries)
    return [loops.find_possible_loop_closures(int(q), case.ref_xy, case.adj_ptr, case.adj_idx, case.max_distance, case.min_chain,
                                              start=int(s), n_visit=case.n_visit) for q, s in zip(case.queries, starts)]


def near_rule(case):
    return [gc.NearResult(near_by_rule.dist_sq(case.poses, q), near_by_rule.find_near_by_scan(case.poses, q),
                          [near_by_rule.find_near_by_vertices(case.poses, q, r) for r in case.radii]) for q in case.queries]


@pytest.mark.parametrize("case", LOOPS, ids=[c.name for c in LOOPS])
def test_loop_case_sits_on_its_edge(case):
    n = case.ref_xy.shape[0]
    assert case.adj_ptr.shape == (n + 1,) and case.adj_ptr[0] == 0 and case.adj_ptr[n] == case.adj_idx.size
    assert case.adj_idx.size == 0 or (0 <= case.adj_idx.min() and case.adj_idx.max() < n)
    assert np.isfinite(case.ref_xy).all() and len(case.queries) >= 2 and ((0 <= case.queries) & (case.queries < n)).all()
    assert case.starts is None or (len(case.starts) == len(case.queries) and (case.starts >= 0).all())
    assert case.n_visit is None or 0 <= case.n_visit <= n
    case.check(loop_oracle(case))


@pytest.mark.parametrize("case", NEAR, ids=[c.name for c in NEAR])
def test_near_by_case_sits_on_its_edge(case):
    assert np.isfinite(case.poses).all() and np.isfinite(case.queries).all(), "non-finite coordinates are out of scope"
    with np.errstate(over="ignore"):
        case.check(near_rule(case))


def test_graph_table_holds_every_size_and_goes_large_small_large():
    assert [c.ref_xy.shape[0] for c in LOOPS if c.name.startswith("sizes")] == list(gc.LOOP_SIZES)
    assert {c.ref_xy.shape[0] % 4 for c in LOOPS} == {0, 1, 2, 3}
    assert [c.poses.shape[0] for c in NEAR if c.name.startswith("near sizes")] == list(gc.NEAR_SIZES)
    sizes = [c.ref_xy.shape[0] for c in gc.reuse_order(LOOPS)]
    assert len(sizes) == len(LOOPS) and sizes[0] == max(sizes) and sizes[1] == min(sizes) and sizes[2] > sizes[1] and sizes[2] > sizes[3]
    assert any(c.starts is None for c in LOOPS) and any(c.starts is not None and not c.starts.any() for c in LOOPS)
    assert any(c.name == gc.CAP_CASE for c in NEAR)
    # k_near_by_radius: min(ceil(n / 256), 256) workgroups of 256, so a trip of its strided loop takes NEAR_TRIP vertices
    assert gc.NEAR_TRIP == 256 * 256 and max(gc.NEAR_SIZES) <= gc.NEAR_TRIP, "the size cases stay within one trip"
    trips = [c.poses.shape[0] for c in NEAR if c.name.startswith("near trips")]
    assert trips == list(gc.NEAR_TRIP_SIZES) == [c.poses.shape[0] for c in NEAR][-len(trips):], "the large stores come last"
    assert [-(-n // gc.NEAR_TRIP) for n in trips] == [1, 1, 2, 2, 3] and next(c for c in NEAR if c.name == gc.TRIP_CAP_CASE).poses.shape[0] > gc.NEAR_TRIP
    assert all(np.unique(c.poses, axis=0).shape[0] == c.poses.shape[0] for c in NEAR if c.name.startswith("near trips")), "distinct points"


# ---- tests/spa_cases.py: the pose-graph solver's table through oracle/spa.py alone (GPU side: tests/test_spa_edges_gpu.py) --------
import spa_cases as sc      # noqa: E402

SPA = list(sc.all_cases())
SPA_FAIL = list(sc.failure_cases())


def test_spa_case_names_are_unique_and_every_mode_is_there():
    names = [c.name for c in SPA] + [c.name for c, _ in SPA_FAIL]
    assert len(set(names)) == len(names)
    assert {c.mode for c in SPA} == {"zero", "one", "run"} and {c.mode for c, _ in SPA_FAIL} == {"fail"}
    for c in SPA:
        assert c.name.endswith(f"[{c.mode}]") and len(c.nodes) <= 71, c.name
        if c.mode == "zero":
            assert c.options["initial_trust_region_radius"] < sc.oracle_options(c.options).min_trust_region_radius
        if c.mode == "one":
            assert c.options["max_num_iterations"] == 1
    assert max(len(c.cons) for c in SPA) == 257


@pytest.mark.parametrize("case", SPA + [c for c, _ in SPA_FAIL], ids=lambda c: c.name)
def test_spa_case_reaches_its_edge(case):
    run = sc.oracle_run(case)
    if case.mode == "zero":
        assert run.info["iterations"] == 0 and "Minimum trust region radius" in run.info["message"] and np.array_equal(run.x, run.x0)
        assert np.isfinite(run.info["initial_cost"]) and run.info["initial_cost"] > 0.0
    if case.mode == "one":
        assert run.info["iterations"] == 1 and len(run.info["log"]) == 1 and run.info["log"][0, 7] in (0.0, 1.0, 2.0, 3.0)
    if case.mode in ("one", "run"):
        assert run.info["usable"]
    assert case.check is not None, "a case without a check of its edge"
    case.check(run)


def test_spa_rejected_options_and_reuse_sequence():
    names = {c.name: c for c in SPA + [c for c, _ in SPA_FAIL]}
    graph = names[sc.REJECTED_OPTIONS_GRAPH]
    assert len(sc.REJECTED_OPTIONS) == 6
    for options in sc.REJECTED_OPTIONS:
        assert options["loss_function"] != "None" and not options["loss_scale"] > 0.0
        with pytest.raises(ValueError):
            sc.oracle_run(graph._replace(options={**graph.options, **options}))
    assert sc.oracle_run(graph._replace(options={**graph.options, **sc.ACCEPTED_OPTIONS})).info["usable"]
    seq = [names[n] for n in sc.REUSE_SEQUENCE]
    assert [c.mode for c in seq] == ["run", "fail", "one", "run", "one"]
    runs = [sc.oracle_run(c) for c in seq]
    assert sc.verdicts(runs[0])[0] >= 3 and sc.verdicts(runs[3])[1] >= 1          # doubled decrease factors; a non-monotonic reference
    assert set(sc.ORDER_ERR) == {c.name for c in sc.modes(SPA, "run")}


def test_spa_table_reaches_every_verdict_and_termination():
    runs = [sc.oracle_run(c) for c in sc.modes(SPA, "run")]
    verdicts = set(np.concatenate([r.info["log"][:, 7] for r in runs]).tolist())
    assert verdicts == {0.0, 1.0, 2.0, 3.0}
    messages = {r.info["message"].split(" reached")[0] for r in runs}
    assert messages >= {"Maximum number of iterations", "Gradient tolerance", "Parameter tolerance", "Function tolerance", "Minimum trust region radius"}
    assert any(r.info["log"][0, 7] == 0.0 for r in [sc.oracle_run(c) for c in sc.modes(SPA, "one")]), "no `one` case whose step is rejected"
