"""CPU: the rule of the region analysis (tests/map_regions_rule.py) against a brute-force breadth-first search on every case of
tests/map_regions_cases.py, against scipy.ndimage.label where scipy is installed, on hand values, and on the small map."""
from collections import deque

import numpy as np
import pytest

import map_field_rule as fr
import map_localize_cases as lc
import map_regions_cases as cases
import map_regions_rule as rule

CASES = cases.region_cases()
BY_NAME = {c.name: c for c in CASES}


def bfs_roots(mask, connectivity):
    """(height, width) int64: the smallest window index of every cell's component, -1 off the mask, by a search from every cell that
    no earlier search reached (row-major order: the start is the smallest)"""
    h, w = mask.shape
    out = np.full((h, w), -1, dtype=np.int64)
    steps = rule.neighbours(connectivity)
    for j0, i0 in zip(*np.nonzero(mask)):
        if out[j0, i0] >= 0:
            continue
        out[j0, i0] = root = int(j0) * w + int(i0)
        todo = deque([(int(j0), int(i0))])
        while todo:
            j, i = todo.popleft()
            for dj, di in steps:
                nj, ni = j + dj, i + di
                if 0 <= nj < h and 0 <= ni < w and mask[nj, ni] and out[nj, ni] < 0:
                    out[nj, ni] = root
                    todo.append((nj, ni))
    return out


def brute_record(view, d2, ids, other, k):
    """one record member by member, in Python integers"""
    w = view["width"]
    members = [(int(j), int(i)) for j, i in zip(*np.nonzero(ids == k))]
    n, si, sj = len(members), sum(i for _, i in members), sum(j for j, _ in members)
    ci, cj = (2 * si + n) // (2 * n), (2 * sj + n) // (2 * n)
    anchor = min(((i - ci) ** 2 + (j - cj) ** 2, j * w + i) for j, i in members)[1]
    links = [int(other[j, i]) for j, i in members if other[j, i] < rule.DROPPED]
    xs, ys = [i for _, i in members], [j for j, _ in members]
    return dict(root=min(j * w + i for j, i in members), n_cells=n, box=(min(xs) + view["ox"], min(ys) + view["oy"], max(xs) - min(xs) + 1, max(ys) - min(ys) + 1),
                sum_i=si, sum_j=sj, max_d2=max(int(d2[j, i]) for j, i in members), n_other=sum(1 for j, i in members if other[j, i] != rule.NONE),
                link=min(links) if links else rule.NONE, anchor_cell=anchor)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_rule_against_brute_force(case):
    d2 = cases.field_values(case)
    got = rule.analyse(case.view, d2, case.radius, **case.params)
    p = dict(rule.PARAMS, **case.params)
    rc = rule.params_check(p, case.view["scale"])
    win = case.view["cells"][:case.view["height"], :case.view["width"]]
    traversable = (win == 255) & (d2.astype(np.int64) >= rc * rc)
    frontier = np.zeros_like(traversable)
    h, w = win.shape
    for j, i in zip(*np.nonzero(win == 255)):
        frontier[j, i] = any(0 <= j + dj < h and 0 <= i + di < w and win[j + dj, i + di] not in (100, 255) for dj, di in rule.neighbours(p["connectivity"]))
    assert got["stats"]["n_traversable"] == int(traversable.sum()) and got["stats"]["n_frontier_cells"] == int(frontier.sum())
    for which, (mask, key, minimum, maximum) in enumerate(((traversable, "region", p["min_region_cells"], p["max_regions"]),
                                                           (frontier, "frontier", p["min_frontier_cells"], p["max_frontiers"]))):
        roots = bfs_roots(mask, p["connectivity"])
        assert np.array_equal(roots, rule.components(mask, p["connectivity"])), key
        sizes = {int(r): int((roots == r).sum()) for r in np.unique(roots[roots >= 0])}
        passing = [r for r in sorted(sizes) if sizes[r] >= minimum]
        want = np.full(roots.shape, rule.NONE, dtype=np.uint32)
        want[roots >= 0] = rule.DROPPED
        for k, r in enumerate(passing[:maximum]):
            want[roots == r] = k
        ids = got[key + "_ids"]
        assert np.array_equal(ids, want), key
        st = got["stats"]
        assert (st["n_total"][which], st["n_kept"][which], st["truncated"][which]) == (len(sizes), min(len(passing), maximum), int(len(passing) > maximum))
        other = got["frontier_ids" if which == 0 else "region_ids"]
        records = got[key + "s"]
        assert len(records) == st["n_kept"][which]
        for k in list(range(len(records)))[:3] + list(range(len(records)))[-2:]:          # the first and the last few, member by member
            for name, value in brute_record(case.view, d2, ids, other, k).items():
                assert records[k][name] == value, (key, k, name)


def test_ids_equal_scipy_s_numbering_minus_one():
    ndimage = pytest.importorskip("scipy.ndimage")
    for case in CASES:
        if "capped" in case.name or "minimum" in case.name:
            continue
        got = rule.analyse(case.view, cases.field_values(case), case.radius, **case.params)
        structure = np.ones((3, 3)) if case.params["connectivity"] == 8 else None
        for key in ("region_ids", "frontier_ids"):
            labels, n = ndimage.label(got[key] != rule.NONE, structure=structure)
            assert n == got["stats"]["n_kept"][0 if key == "region_ids" else 1], case.name
            assert np.array_equal(np.where(labels > 0, labels - 1, rule.NONE).astype(np.uint32), got[key]), (case.name, key)


def run(name):
    case = BY_NAME[name]
    return case, rule.analyse(case.view, cases.field_values(case), case.radius, **case.params)


def test_hand_values_ring_and_diagonal():
    for conn in (4, 8):
        case, got = run(f"30 x 20, a ring of wall: inside and outside, N{conn}")
        assert got["stats"]["n_kept"][0] == 2 and got["regions"][0]["root"] == 0 and got["regions"][1]["root"] == 5 * 30 + 7
        assert got["regions"][1]["n_cells"] == 9 * 12 and got["regions"][0]["n_cells"] == 30 * 20 - 11 * 14
        assert got["regions"][0]["n_other"] == 0 and got["stats"]["n_frontier_cells"] == 0
    for name in ("down-right", "down-left"):
        _, four = run(f"130 x 34, a diagonal pair {name} across a tile corner, N4")
        _, eight = run(f"130 x 34, a diagonal pair {name} across a tile corner, N8")
        assert four["stats"]["n_kept"][0] == 2 and eight["stats"]["n_kept"][0] == 1 and eight["regions"][0]["n_cells"] == 2
    _, eight = run("130 x 34, a diagonal pair down-right across a tile corner, N8")
    assert eight["regions"][0]["root"] == 15 * 130 + 63 and eight["regions"][0]["box"] == (63, 15, 2, 2)
    _, ring = run("130 x 34, a ring around a tile corner, N4")
    assert ring["stats"]["n_kept"][0] == 1 and ring["regions"][0]["n_cells"] == 12 and ring["regions"][0]["root"] == 14 * 130 + 62


def test_hand_values_filter_and_cap():
    case = BY_NAME["66 x 18 checkerboard, capped at 100, N4"]
    d2 = cases.field_values(case)
    n = 66 * 18 // 2
    got = rule.analyse(case.view, d2, 0, connectivity=4, max_regions=100)
    assert got["stats"]["n_total"][0] == n and got["stats"]["n_kept"][0] == 100 and got["stats"]["truncated"][0] == 1
    ids = got["region_ids"]
    assert ids[0, 0] == 0 and ids[0, 2] == 1 and ids[0, 1] == rule.NONE and ids[17, 65] == rule.DROPPED and int((ids == rule.DROPPED).sum()) == n - 100
    exact = rule.analyse(case.view, d2, 0, connectivity=4, max_regions=n)
    assert exact["stats"]["n_kept"][0] == n and exact["stats"]["truncated"][0] == 0 and not (exact["region_ids"] == rule.DROPPED).any()
    below = rule.analyse(case.view, d2, 0, connectivity=4, max_regions=n - 1)
    assert below["stats"]["n_kept"][0] == n - 1 and below["stats"]["truncated"][0] == 1 and int((below["region_ids"] == rule.DROPPED).sum()) == 1
    assert below["region_ids"][17, 65] == rule.DROPPED, "the cut takes the last root"
    _, one = run("66 x 18 checkerboard, capped at 100, N8")
    assert one["stats"]["n_kept"][0] == 1 and one["regions"][0]["n_cells"] == n and one["stats"]["truncated"][0] == 0
    # a size filter at min and at min - 1: the ring's inside has 108 cells
    ring = BY_NAME["30 x 20, a ring of wall: inside and outside, N4"]
    at = rule.analyse(ring.view, cases.field_values(ring), 0, connectivity=4, min_region_cells=108)
    assert at["stats"]["n_kept"][0] == 2 and at["stats"]["truncated"][0] == 0
    above = rule.analyse(ring.view, cases.field_values(ring), 0, connectivity=4, min_region_cells=109)
    assert above["stats"]["n_kept"][0] == 1 and above["stats"]["n_total"][0] == 2 and above["region_ids"][5, 7] == rule.DROPPED and above["region_ids"][0, 0] == 0


def test_hand_values_link_anchor_and_clearance():
    for conn in (4, 8):
        case, got = run(f"a cluster whose traversable cells lie in two regions, Rc 2, N{conn}")
        assert got["stats"]["n_kept"] == [2, 1], "the neck closes at Rc 2; the frontier row is one cluster"
        f = got["frontiers"][0]
        assert f["n_cells"] == 40 and f["root"] == 7 * 40 and f["link"] == 0, "it touches regions 0 and 1: the smaller id wins"
        assert set(got["region_ids"][7][got["region_ids"][7] < rule.DROPPED].tolist()) == {0, 1}
        assert f["n_other"] == int((got["region_ids"][7] != rule.NONE).sum()) == 40 - 3, "columns 19 .. 21 of the row have d2 = 2, 1, 2 to the wall's end at (20, 6): below Rc * Rc = 4"
        assert got["regions"][0]["link"] == 0 and got["regions"][1]["link"] == 0
        # an even row of 40: the centroid cell is (2 * 780 + 40) // 80 = 20, a member: no tie
        assert f["anchor_cell"] == 7 * 40 + 20
    # an anchor tie: the ring around the tile corner has its centroid cell (64, 16) inside the hole; two members are equally near
    _, ring = run("130 x 34, a ring around a tile corner, N8")
    r = ring["regions"][0]
    assert (rule.centroid_cell(r["sum_i"], 12), rule.centroid_cell(r["sum_j"], 12)) == (64, 16) and ring["region_ids"][16, 64] == rule.NONE
    assert r["anchor_cell"] == 16 * 130 + 65, "(65, 16) and (64, 17) both lie one cell from (64, 16): the smaller window index wins"
    counts = {}
    for rc in (0, 2, 5):
        _, got = run(f"two rooms and a door of 2 cells, Rc {rc}, N8")
        counts[rc] = got["stats"]["n_kept"][0]
    assert counts == {0: 1, 2: 2, 5: 2}, "the door closes at Rc 2 and splits the region"
    _, far = run("two rooms, a field of R 3: FAR members, N8")
    assert far["regions"][0]["max_d2"] == fr.FAR
    case = BY_NAME["two rooms, a field of R 3: FAR members, N8"]
    with pytest.raises(rule.Refused):
        rule.analyse(case.view, cases.field_values(case), 3, min_clearance=5 / cases.K)
    _, room = run("a closed room beside an open one, N8")
    assert [r["n_other"] for r in room["regions"]] == [0, 18] and room["frontiers"][0]["link"] == 1
    _, edge = run("free cells at the window's edge, nothing unknown, N8")
    assert edge["stats"]["n_frontier_cells"] == 0
    _, seven = run("a cell of state 7 is unknown, N8")
    assert seven["stats"]["n_frontier_cells"] == 8 and seven["stats"]["n_kept"][1] == 1
    _, seven4 = run("a cell of state 7 is unknown, N4")
    assert seven4["stats"]["n_frontier_cells"] == 4 and seven4["stats"]["n_kept"][1] == 4


def test_refusals_and_lookup():
    good = dict(rule.PARAMS)
    for kw in (dict(min_clearance=float("nan")), dict(min_clearance=-0.1), dict(min_clearance=float("inf")), dict(min_clearance=300.0), dict(connectivity=6),
               dict(min_region_cells=0), dict(min_frontier_cells=0), dict(max_regions=0), dict(max_frontiers=(1 << 20) + 1)):
        with pytest.raises(rule.Refused):
            rule.params_check(dict(good, **kw), 4.0)
    assert rule.params_check(dict(good, min_clearance=256.0, max_regions=1 << 20), 4.0) == 1024
    case, got = run("40 x 50 random, p_occ 0.4, seed 1, minimum 3, N8")
    pts = cases.lookup_points(case.view)
    status, ids = rule.lookup(case.view, got["region_ids"], pts)
    assert set(status.tolist()) == {rule.AT_OK, rule.AT_NONE, rule.AT_DROPPED, rule.OUTSIDE}
    assert status[-1] == rule.OUTSIDE and status[-2] == rule.OUTSIDE and status[-3] == rule.OUTSIDE


@pytest.fixture(scope="module")
def small(oracle_lib):
    sm, m = lc.small_map()
    return sm, m, fr.d2_separable(m.view, 40)


@pytest.mark.parametrize("conn", (4, 8))
def test_small_map_poses_share_the_largest_region(small, conn):
    sm, m, d2 = small
    for rc in (0, 3, 8):
        got = rule.analyse(m.view, d2, 40, min_clearance=cases.clearance_of(rc, m.view["scale"]), connectivity=conn)
        assert got["stats"]["clearance_cells"] == rc
        status, ids = rule.lookup(m.view, got["region_ids"], np.asarray(sm.poses)[:, :2])
        assert (status == rule.AT_OK).all() and len(set(ids.tolist())) == 1, (rc, status, ids)
        sizes = [r["n_cells"] for r in got["regions"]]
        assert sizes[int(ids[0])] == max(sizes) and got["stats"]["n_kept"][0] > 1 and got["stats"]["n_kept"][1] > 1
        if rc == 0:
            try:
                from scipy import ndimage
            except ImportError:
                continue
            win = m.view["cells"][:m.height, :m.width]
            structure = np.ones((3, 3)) if conn == 8 else None
            labels, n = ndimage.label(win == 255, structure=structure)
            assert n == got["stats"]["n_kept"][0] and np.bincount(labels.ravel())[1:].max() == max(sizes)
            assert ndimage.label(got["frontier_ids"] != rule.NONE, structure=structure)[1] == got["stats"]["n_kept"][1]
