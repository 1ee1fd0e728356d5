"""CPU: every case of tests/map_field_limit_cases.py sits on the limit its name says -- from tests/map_field_rule.py and the launch
arithmetic of csrc/occupancy_field.hip and csrc/occupancy_field_update.hip alone.  No library, no GPU."""
import numpy as np

import map_field_limit_cases as cases
import map_field_rule as rule
import map_field_update_cases as uc

FIELD_CASES = cases.field_cases()


def test_the_field_cases_sit_on_the_limits():
    shapes = [(c.view["width"], c.view["height"], c.radius) for c in FIELD_CASES]
    assert shapes == [(32768, 2, 3), (32744, 1, 3), (32745, 1, 3), (32768, 1, 1024), (1, 32768, 1024), (4096, 3, 0), (3, 4096, 0)]
    assert rule.MAX_SIDE == 32768 and rule.MAX_UNCAPPED_SIDE == 4096 and rule.MAX_RADIUS == 1024
    for c in FIELD_CASES:
        v = c.view
        assert rule.field_check(v["width"], v["height"], v["scale"], c.radius / v["scale"], c.obstacles) == c.radius, c.name
        for grown in ((v["width"] + 1, v["height"]), (v["width"], v["height"] + 1)):
            if max(grown) > (rule.MAX_SIDE if c.radius else rule.MAX_UNCAPPED_SIDE):
                try:
                    rule.field_check(*grown, v["scale"], c.radius / v["scale"], c.obstacles)
                    raise AssertionError(f"{c.name}: one more cell on the long side is still taken")
                except rule.Refused:
                    pass
        d2 = cases.brute(v, c.radius, c.obstacles)
        st = rule.stats(d2)
        assert st["n_obstacles"] == int(rule.obstacle_mask(v).sum()) > 0
        for k, want in c.stats.items():
            assert st[k] == want, (c.name, k, st[k])
    assert cases.rows_lds_bytes(32744) == cases.LDS_DEFAULT and cases.rows_lds_bytes(32745) > cases.LDS_DEFAULT
    assert cases.rows_lds_bytes(32768) == 65584
    a, b = (next(c for c in FIELD_CASES if c.name.startswith(n)) for n in ("32768 x 1,", "1 x 32768,"))
    assert np.array_equal(cases.brute(a.view, 1024), cases.brute(b.view, 1024).T), "the transposed case is the transposed field"
    # the first case: obstacles in the first and last column, on both sides of a workgroup's stride of 256 and of 1024 columns
    first = FIELD_CASES[0]
    assert [tuple(x) for x in np.argwhere(rule.obstacle_mask(first.view))] == [(0, 0), (0, 1024), (0, 16384), (1, 1023), (1, 32744), (1, 32767)]


def test_the_reach_case_uses_the_whole_radius():
    c = cases.reach_case()
    d2 = cases.brute(c.view, c.radius)
    assert rule.stats(d2)["max_d2"] == 1024 * 1024 and d2[1, 1024] == 1024 * 1024 and d2[0, 1024] == rule.FAR
    table = rule.cost_table(c.view["scale"], **cases.REACH_INFLATION)
    assert table.size == 1024 * 1024 + 1 and table[-1] > 0 and table[0] == 254 and table[16] == 253 and table[17] < 253
    costs = rule.costs(c.view, d2, c.radius, **cases.REACH_INFLATION)
    assert costs[2, 1500] == 255 and costs[1, 1024] == table[-1] and costs[1, 1025] == 0, "the unknown cell; the last cell the table reaches"
    for x, y, w, h in cases.REACH_RECTS:
        assert 0 <= x and x + w <= 2100 and 0 <= y and y + h <= 3
    assert {r[0] % 4 for r in cases.REACH_RECTS} == {0, 1, 3}
    for n in (64, 65):
        laser, ranges, pose = cases.reach_scan(n)
        sc = rule.score(c.view, d2, c.radius, laser, ranges, pose, 1024)
        assert sc["n_kept"] == sc["n_hit"] == sc["n_inside"] == n and 0 < sc["n_near"] < n
        assert counted_above(c.view, d2, laser, ranges, pose, 2 ** 19) >= 1, "at least one counted end has d2 above 2^19"


def counted_above(view, d2, laser, ranges, pose, bound):
    """how many single beams of the scan score a counted value above `bound`"""
    import map_localize_cases as lc
    n = 0
    for k in range(laser.n_beams):
        one = lc.CaseLaser(1, laser.min_angle + k * laser.ang_res, laser.ang_res, laser.min_range, laser.max_range, laser.range_threshold)
        sc = rule.score(view, d2, 1024, one, ranges[k:k + 1], pose, 1024)
        n += sc["n_near"] == 1 and sc["sum_d2"] > bound
    return n


def boxes(before, after, radius):
    e = uc.expected(before, after, radius, rule.OCCUPIED)
    obst = uc.box_of(rule.obstacle_mask(before) != rule.obstacle_mask(after))
    return e, obst


def test_the_update_cases_take_every_loop_through_a_second_trip():
    before, after, third = cases.wide_edit()
    e, obst = boxes(before, after, 3)
    assert obst == (6, 2, 1284, 8) and obst[2] > 1024 and obst[0] % 4 != 0
    x, y, w, h = e["values_box"]
    x0, x1 = x - before["ox"], x - before["ox"] + w
    assert (x0, x1) == (3, 1293) and e["cells_recomputed"] == 1290 * 12
    quads = ((obst[0] + obst[2] + 3) >> 2) - (obst[0] >> 2)
    assert quads > 64, "k_field_columns_band: blockIdx.x >= 1"
    assert x1 - x0 > 256, "k_field_rows_region: i += 256"
    s0, s1 = max(x0 - 3, 0) & ~3, (min(x1 + 3, 1300) + 3) & ~3
    assert (s1 - s0) >> 2 > 256, "k_field_rows_region: the staging's q += 256"
    e3, obst3 = boxes(after, third, 3)
    assert obst3[0] == 600 and obst3[0] + obst3[2] == 611 and 0 < e3["cells_recomputed"] < 1300 * 12
    assert all(not np.array_equal(cases.brute(a, 3), cases.brute(b, 3)) for a, b in ((before, after), (after, third)))

    before, after = cases.widest_edit()
    e, obst = boxes(before, after, 3)
    assert (obst[0], obst[0] + obst[2]) == (2, 32766)
    x0, x1 = e["values_box"][0], e["values_box"][0] + e["values_box"][2]
    s0, s1 = max(x0 - 3, 0) & ~3, (min(x1 + 3, 32768) + 3) & ~3
    assert (s1 - s0) * 2 == 65536 == cases.LDS_DEFAULT, "the row pass stages a whole row"

    before, after = cases.count_edit()
    assert (cases.stride4(2052) >> 2) * 1024 == 525312 > cases.COUNT_THREADS, "k_field_count: a second grid-stride trip"
    d2 = cases.brute(before, 8)
    assert rule.stats(d2) == dict(n_obstacles=6, n_far=2052 * 1024 - (6 * 197 - corner_loss()), max_d2=64)
    e, obst = boxes(before, after, 8)
    assert obst == (777, 300, 1, 1) and e["cells_recomputed"] == 17 * 17


def corner_loss():
    """the cells of the discs of radius 8 (197 cells each) that the window cuts off: four obstacles sit in its corners"""
    j, i = np.mgrid[-8:9, -8:9]
    disc = i * i + j * j <= 64
    assert int(disc.sum()) == 197
    quarter = int((disc & (i >= 0) & (j >= 0)).sum())
    return 4 * (197 - quarter)
