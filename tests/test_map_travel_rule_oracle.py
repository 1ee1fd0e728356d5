"""CPU: the rule of the travel costs (tests/map_travel_rule.py) against an independent whole-grid pull relaxation in numpy on every
case of tests/map_travel_cases.py, against scipy.sparse.csgraph.dijkstra where scipy is installed, on hand values, against the
region analysis' rule, and on the small map."""
import numpy as np
import pytest

import map_field_rule as fr
import map_localize_cases as lc
import map_regions_rule as regions
import map_travel_cases as cases
import map_travel_rule as rule

CASES = cases.travel_cases()
BY_NAME = {c.name: c for c in CASES}
FAR = rule.FAR
BIG = np.int64(2 ** 62)


def relaxed(q, goal_cells, connectivity, cut_corners):
    """the values by pulls over the whole grid until nothing changes: V(u) = min(V(u), V(v) + L q(u)) over the allowed steps, with
    allowedness worked out here from q alone"""
    h, w = q.shape
    ok = np.zeros((h + 2, w + 2), dtype=bool)
    ok[1:-1, 1:-1] = q > 0
    cost = np.zeros((h + 2, w + 2), dtype=np.int64)
    cost[1:-1, 1:-1] = q
    value = np.full((h + 2, w + 2), BIG, dtype=np.int64)
    for g in goal_cells:
        value[1 + g // w, 1 + g % w] = 0
    inner = (slice(1, h + 1), slice(1, w + 1))
    shifted = lambda a, di, dj: a[1 + dj:1 + dj + h, 1 + di:1 + di + w]  # noqa: E731
    steps = [(1, 0, 5), (0, 1, 5), (-1, 0, 5), (0, -1, 5)] + ([(1, 1, 7), (-1, 1, 7), (-1, -1, 7), (1, -1, 7)] if connectivity == 8 else [])
    while True:
        best = value[inner].copy()
        for di, dj, length in steps:
            allowed = ok[inner] & shifted(ok, di, dj)
            if di and dj and not cut_corners:
                allowed = allowed & shifted(ok, di, 0) & shifted(ok, 0, dj)
            there = shifted(value, di, dj)
            best = np.where(allowed & (there < BIG), np.minimum(best, there + length * cost[inner]), best)
        if np.array_equal(best, value[inner]):
            break
        value[inner] = best
    out = value[inner]
    return np.where(out >= BIG, FAR, out).astype(np.uint32)


_answers = {}


def answer(case):
    if case.name not in _answers:
        _answers[case.name] = rule.analyse(case.view, cases.field_values(case), case.radius, case.goals, **case.params)
    return _answers[case.name]


SMALL = [c for c in CASES if c.view["width"] * c.view["height"] <= 130 * 50]


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_rule_against_the_relaxation(case):
    got = answer(case)
    p = got["params"]
    usable = [int(c) for c, s in zip(got["goal_cells"], got["goal_status"]) if s == rule.GOAL_OK]
    want = relaxed(got["weights"], usable, p["connectivity"], p["cut_corners"])
    assert np.array_equal(got["values"], want), f"{int((got['values'] != want).sum())} values differ"
    assert np.all((got["values"] != FAR) <= (got["weights"] > 0)), "a value on a cell that is not traversable"
    assert got["stats"]["n_reached"] == int((want != FAR).sum())


@pytest.mark.parametrize("across", (True, False))
def test_rule_on_the_long_strips(across):
    case = BY_NAME[f"{'32768 x 2' if across else '2 x 32768'}, sparse walls, N8"]
    got = answer(case)
    q, v = got["weights"].astype(np.int64), got["values"].astype(np.int64)
    assert got["stats"]["n_reached"] > 1000 and (v == FAR).sum() > 1000
    # along the strip a reached cell differs from its reached neighbour by at most one straight step of the dearer of the two
    a, b = (v[:, :-1], v[:, 1:]) if across else (v[:-1, :], v[1:, :])
    qa, qb = (q[:, :-1], q[:, 1:]) if across else (q[:-1, :], q[1:, :])
    both = (a != FAR) & (b != FAR)
    assert np.all(np.abs(a - b)[both] <= 5 * np.maximum(qa, qb)[both])
    assert np.all(((a == FAR) == (b == FAR)) | (qa == 0) | (qb == 0)), "two traversable neighbours, one reached and one not"


def test_against_scipy_where_it_imports():
    graph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    for name in ("40 x 50 random, p_occ 0.1, seed 1, 3 goals, N8, cut 0", "40 x 50 random, p_occ 0.4, seed 1, 1 goals, N4, cut 1", "65 x 17 mixed, N8, cut 1",
                 "two rooms, cost_weight 255, neutral_cost 1, N8"):
        case = BY_NAME[name]
        got = answer(case)
        q, p = got["weights"], got["params"]
        h, w = q.shape
        masks = rule.step_masks(q, p["connectivity"], p["cut_corners"])
        rows, cols, data = [], [], []
        for n, (di, dj) in enumerate(rule.STEPS):
            jj, ii = np.nonzero((masks >> n) & 1)
            rows.append((jj + dj) * w + ii + di); cols.append(jj * w + ii)          # the edge v -> u of a step u -> v, at L q(u)
            data.append(rule.LENGTH[n] * q[jj, ii].astype(np.float64))
        m = sparse.csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(h * w, h * w))
        usable = sorted({int(c) for c, s in zip(got["goal_cells"], got["goal_status"]) if s == rule.GOAL_OK})
        dist = graph.dijkstra(m, directed=True, indices=usable, min_only=True)
        want = np.where(np.isinf(dist), FAR, dist).astype(np.uint32).reshape(h, w)      # integers below 2^53: exact in doubles
        assert np.array_equal(got["values"], want), name


# ---------------------------------------------------------------- hand values
def solve(cells, goals, radius=0, **params):
    view = lc.view_of(cells, cases.A, cases.K)
    goal_xy = [cases.world(view, i, j) for i, j in goals]
    return view, rule.analyse(view, fr.d2_brute(view, radius), radius, goal_xy, **params)


def test_a_straight_corridor_is_five_q_summed():
    view, got = solve(cases.corridor(9), [(0, 0)], cost_weight=0, neutral_cost=50)
    assert got["values"][0].tolist() == [250 * k for k in range(9)]
    view, got = solve(cases.corridor(9), [(8, 0)], cost_weight=0, neutral_cost=3, connectivity=4)
    assert got["values"][0].tolist() == [15 * (8 - k) for k in range(9)]
    c = cases.corridor(9)
    c[0, 8] = cases.O                                          # weights that differ: the cell left is the cell paid for
    view, got = solve(c, [(0, 0)], radius=8)
    q = got["weights"][0].astype(np.int64)
    assert len(set(q[:8].tolist())) > 2 and q[8] == 0
    assert got["values"][0, :8].tolist() == [5 * int(q[1:k + 1].sum()) for k in range(8)] and got["values"][0, 8] == FAR


def test_one_diagonal():
    view, got = solve(cases.full(2, 2), [(0, 0)], cost_weight=0, neutral_cost=10)
    assert got["values"].tolist() == [[0, 50], [50, 70]]
    view, got = solve(cases.full(2, 2), [(0, 0)], cost_weight=0, neutral_cost=10, connectivity=4)
    assert got["values"].tolist() == [[0, 50], [50, 100]]


def test_a_diagonal_between_two_wall_corners_needs_cut_corners():
    for cut, conn, reached in ((0, 8, False), (1, 8, True), (1, 4, False)):
        view, got = solve(cases.wall_corners(), [(0, 4)], cost_weight=0, neutral_cost=10, cut_corners=cut, connectivity=conn)
        v = got["values"]
        assert (v[0, 4] != FAR) == reached, (cut, conn)
        assert v[2, 2] == (FAR if not reached else v[3, 1] + 70)
        assert v[4, 1] == 50 and v[3, 1] == (70 if conn == 8 else 100)


def test_raising_cost_weight_flips_the_path_from_the_corridor_to_the_detour():
    cells = cases.detour()
    start = [cases.world(lc.view_of(cells, cases.A, cases.K), 1, 1)]
    seen = {}
    for cw in (0, 255):
        view, got = solve(cells, [(28, 1)], radius=8, cost_weight=cw, inflation_radius=1.5, inscribed_radius=0.0, cost_scaling_factor=1.0)
        path = rule.paths(view, got["values"], got["weights"], start, 0, 4096, 8, 0)[0]
        assert path["status"] == rule.PATH_OK
        seen[cw] = path["cells"]
    rows = {cw: set((c[:, 1] - 0).tolist()) for cw, c in seen.items()}
    assert rows[0] == {1}, "without inflation costs the corridor along the wall is the way"
    assert max(rows[255]) >= 3 and len(seen[255]) > len(seen[0]), "with them the open detour is"


def test_the_direction_order_alone_fixes_the_path_on_a_uniform_square():
    view, got = solve(cases.full(20, 20), [(0, 0)], cost_weight=0)
    q = got["weights"]
    path = rule.paths(view, got["values"], q, [cases.world(view, 19, 7)], 0, 4096, 8, 0)[0]
    # 7 diagonals and 12 straights whatever the order: direction 2, (-1, 0), comes before direction 6, (-1, -1)
    assert path["cells"].tolist() == [[19 - k, 7] for k in range(13)] + [[6 - k, 6 - k] for k in range(7)]
    assert path["cost"] == (12 * 5 + 7 * 7) * 50 == got["values"][7, 19]
    path = rule.paths(view, got["values"], q, [cases.world(view, 7, 19)], 0, 4096, 8, 0)[0]
    assert path["cells"].tolist() == [[7, 19 - k] for k in range(13)] + [[6 - k, 6 - k] for k in range(7)], "direction 3, (0, -1), before 6"


def test_two_goals_each_cell_from_the_nearer_in_cost():
    cells = cases.corridor(11)
    view, both = solve(cells, [(0, 0), (10, 0)], cost_weight=0, neutral_cost=2)
    _, left = solve(cells, [(0, 0)], cost_weight=0, neutral_cost=2)
    _, right = solve(cells, [(10, 0)], cost_weight=0, neutral_cost=2)
    assert np.array_equal(both["values"], np.minimum(left["values"], right["values"]))
    assert both["values"][0].tolist() == [10 * min(k, 10 - k) for k in range(11)]


def test_a_blocked_goal_a_snapped_goal_and_a_snap_tie():
    cells = cases.full(5, 7)
    cells[1:4, 2:5] = cases.O                                  # a 3 x 3 block; its centre is (3, 2)
    view, got = solve(cells, [(3, 2)], goal_snap_cells=1)
    assert got["goal_status"].tolist() == [rule.GOAL_BLOCKED] and np.all(got["values"] == FAR)
    view, got = solve(cells, [(3, 2)], goal_snap_cells=2)
    # the ring at Chebyshev distance 2: dist2 4 at (3, 0), (1, 2), (5, 2), (3, 4); the smallest window index is (3, 0)'s
    assert got["goal_status"].tolist() == [rule.GOAL_OK] and got["goal_cells"].tolist() == [3] and got["values"][0, 3] == 0
    cells[0, 3] = cases.O
    view, got = solve(cells, [(3, 2)], goal_snap_cells=2)
    assert got["goal_cells"].tolist() == [2 * 7 + 1], "then (1, 2): the tie goes to the smaller index"
    view, got = solve(cells, [(-1, 2), (3, 2), (0, 0)], goal_snap_cells=0)
    assert got["goal_status"].tolist() == [rule.GOAL_OUTSIDE, rule.GOAL_BLOCKED, rule.GOAL_OK]


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_every_path_costs_the_value_at_its_start_and_takes_allowed_steps(case):
    got = answer(case)
    p, v, q, view = got["params"], got["values"], got["weights"], case.view
    masks = rule.step_masks(q, p["connectivity"], p["cut_corners"])
    paths = rule.paths(view, v, q, case.starts, 1, 4096, p["connectivity"], p["cut_corners"])
    assert len(paths) == len(case.starts)
    for path in paths:
        if path["status"] != rule.PATH_OK:
            assert path["status"] in (rule.PATH_UNREACHED, rule.PATH_OUTSIDE) and path["n_cells"] == 0
            continue
        cells = path["cells"] - np.array([view["ox"], view["oy"]])
        total = 0
        for (i, j), (a, b) in zip(cells[:-1].tolist(), cells[1:].tolist()):
            n = rule.STEPS.index((a - i, b - j))
            assert (masks[j, i] >> n) & 1, "a step that is not allowed"
            total += rule.LENGTH[n] * int(q[j, i])
        assert total == path["cost"] == int(v[cells[0][1], cells[0][0]]) and v[cells[-1][1], cells[-1][0]] == 0


def test_the_reached_mask_is_the_goal_s_region():
    """with cut_corners = 1, or under connectivity 4, travel's steps are the region analysis' neighbours"""
    names = ["40 x 50 random, p_occ 0.4, seed 1, 1 goals, N8, cut 1", "40 x 50 random, p_occ 0.4, seed 1, 1 goals, N4, cut 0", "40 x 50 random, p_occ 0.1, seed 2, 1 goals, N4",
             "two rooms and a door of 2 cells, Rc 2, N8", "two rooms and a door of 2 cells, Rc 2, N4", "129 x 33 comb, the teeth join in the last row of the last tile, N4"]
    for name in names:
        case = BY_NAME[name]
        got = answer(case)
        p = got["params"]
        if p["connectivity"] == 8 and not p["cut_corners"]:
            if "two rooms" not in name:
                continue
        ids = regions.analyse(case.view, cases.field_values(case), case.radius, min_clearance=p["min_clearance"], connectivity=p["connectivity"],
                              max_regions=1 << 20)["region_ids"]
        goal = int(got["goal_cells"][0])
        mine = ids[goal // case.view["width"], goal % case.view["width"]]
        assert mine < regions.DROPPED
        assert np.array_equal(got["values"] != FAR, ids == mine), name
    far = answer(BY_NAME["two rooms and a door of 2 cells, Rc 2, N8"])
    assert np.all(far["values"][1:21, 33:63] == FAR), "the door closes at Rc 2: the other room is FAR"
    near = answer(BY_NAME["two rooms and a door of 2 cells, Rc 0, N8"])
    assert np.all(near["values"][1:21, 32:64] != FAR)


def test_lookup_and_rank():
    case = BY_NAME["40 x 50 random, p_occ 0.4, seed 2, 3 goals, N8"]
    got = answer(case)
    pts = cases.lookup_points(case.view)
    codes = set()
    for snap in (0, 1, 16):
        status, value, cell = rule.lookup(case.view, got["values"], pts, snap)
        codes |= set(status.tolist())
        for s, v, (cx, cy) in zip(status, value, cell):
            assert (s == rule.AT_OK) == (v != FAR)
            if s == rule.AT_OK:
                assert got["values"][cy - case.view["oy"], cx - case.view["ox"]] == v
    assert codes == {rule.AT_OK, rule.AT_UNREACHED, rule.AT_OUTSIDE}
    clusters = [dict(anchor_xy=tuple(p)) for p in pts[:12]]
    order = rule.rank(case.view, got["values"], clusters, 1)
    assert sorted(k for k, _ in order) == list(range(12))
    reached = [(v, k) for k, v in order if v is not None]
    assert reached == sorted(reached) and all(v is None for _, v in order[len(reached):])


def test_refusals():
    view = lc.view_of(cases.full(4, 4), cases.A, cases.K)
    d2 = fr.d2_brute(view, 0)
    goal = [cases.world(view, 0, 0)]
    for kw, why in ((dict(connectivity=6), "connectivity"), (dict(cut_corners=2), "cut_corners"), (dict(neutral_cost=0), "neutral_cost"), (dict(neutral_cost=256), "neutral_cost"),
                    (dict(cost_weight=-1), "cost_weight"), (dict(cost_weight=256), "cost_weight"), (dict(goal_snap_cells=17), "goal_snap_cells"),
                    (dict(min_clearance=float("nan")), "min_clearance"), (dict(min_clearance=300.0), "radius"), (dict(inflation_radius=float("inf")), "inflation"),
                    (dict(inscribed_radius=1.0, inflation_radius=0.5), "inflation"), (dict(connectivity=5, neutral_cost=0, min_clearance=-1.0), "connectivity")):
        with pytest.raises(rule.Refused) as e:
            rule.analyse(view, d2, 0, goal, **kw)
        assert str(e.value) == why, kw
    for radius, kw, why in ((2, dict(min_clearance=3 / cases.K), "reach of the clearance"), (2, dict(), "reach of the inflation"), (2, dict(cost_weight=0), None), (3, dict(), None)):
        if why is None:
            rule.analyse(view, fr.d2_brute(view, radius), radius, goal, **kw)
        else:
            with pytest.raises(rule.Refused) as e:
                rule.analyse(view, fr.d2_brute(view, radius), radius, goal, **kw)
            assert str(e.value) == why
    assert rule.q_max(50, 13) == 255 and rule.q_max(255, 255) == 4287 and rule.q_max(1, 0) == 1
    assert 0xFFFFFFFE // (7 * 4287) == 143122
    assert not rule.overflows(143122, 1, 8, 4287) and rule.overflows(143123, 1, 8, 4287) and rule.overflows(1, 143123, 8, 4287)
    assert not rule.overflows(143123, 1, 4, 4287), "Lmax is 5 under connectivity 4"


# ---------------------------------------------------------------- the small map
def test_the_small_map_from_the_first_mapped_pose(oracle_lib):
    sm, m = lc.small_map()
    d2 = fr.d2_separable(m.view, 40)
    poses = np.asarray(sm.poses)[:, :2]
    for rc in (0, 3):
        got = rule.analyse(m.view, d2, 40, poses[:1], min_clearance=max(0.0, rc - 0.5) / m.view["scale"], goal_snap_cells=2)
        assert got["goal_status"].tolist() == [rule.GOAL_OK] and got["stats"]["clearance_cells"] == rc
        status, value, _ = rule.lookup(m.view, got["values"], poses, 2)
        assert np.all(status == rule.AT_OK) and value[0] == 0 and np.all(value[1:] > 0) and np.all(value != FAR), "all eight poses are reached"
        for path in rule.paths(m.view, got["values"], got["weights"], poses, 2, 4096, 8, 0):
            assert path["status"] == rule.PATH_OK and got["values"][path["cells"][-1][1] - m.view["oy"], path["cells"][-1][0] - m.view["ox"]] == 0
