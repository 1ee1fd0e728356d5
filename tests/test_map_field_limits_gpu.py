"""GPU: the distance field and its region update (csrc/occupancy_field.hip, csrc/occupancy_field_update.hip) on the cases of
tests/map_field_limit_cases.py -- the longest sides, the largest radius, the width at which k_field_rows needs more than 64 KiB of
dynamic LDS, and updates that take every strided loop of the update kernels through a second trip -- against
tests/map_field_rule.py's d2_brute.  Everything is an integer and is compared exactly."""
import numpy as np
import pytest

import map_field_limit_cases as cases
import map_field_rule as rule
from test_map_field_gpu import field_on, same_field
from test_map_field_update_gpu import Followed

pytestmark = pytest.mark.gpu

FIELD_CASES = cases.field_cases()


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c.name for c in FIELD_CASES])
def test_field_at_the_limits(kartohip_lib, case):
    got = field_on(case.view, case.radius, case.obstacles)
    want = cases.brute(case.view, case.radius, case.obstacles)
    same_field(got, want, case.view, case.radius)
    for k, v in case.stats.items():
        assert got.stats[k] == v, (k, got.stats[k])
    got.close()


def test_costs_and_score_at_radius_1024(kartohip_lib, oracle_lib):
    case = cases.reach_case()
    view = case.view
    got = field_on(view, case.radius)
    d2 = cases.brute(view, case.radius)
    same_field(got, d2, view, case.radius)
    for track in (0, 1):
        kw = dict(cases.REACH_INFLATION, track_unknown=track)
        want = rule.costs(view, d2, case.radius, **kw)
        assert np.array_equal(got.costs(**kw), want), f"costs, track_unknown {track}"
        for x, y, w, h in cases.REACH_RECTS:
            block = got.costs_rect(view["ox"] + x, view["oy"] + y, w, h, **kw)
            assert np.array_equal(block, want[y:y + h, x:x + w]), (track, x, y, w, h)
    for n in (64, 65):
        laser, ranges, pose = cases.reach_scan(n)
        sc = got.score(ranges, [pose], laser, truncate_cells=1024)[0]
        want = rule.score(view, d2, case.radius, laser, ranges, pose, 1024)
        assert all(sc[k] == want[k] for k in ("n_kept", "n_hit", "n_inside", "n_near", "sum_d2", "cost")), (n, sc, want)
        assert got.score(ranges, [pose], laser)[0] == sc, "T = 0 is the field's R"
    got.close()


def test_an_update_wider_than_a_workgroups_stride(kartohip_lib):
    """1300 x 12: k_field_columns_band's second workgroup along x, k_field_rows_region's second trips of the staging and of the cells"""
    before, after, third = cases.wide_edit()
    f = Followed(before, 3, d2_rule=cases.brute)
    for band in cases.WIDE_BANDS:
        f.field.set_band_rows(band)
        got = f.step(after)
        assert got["rebuilt"] == 0 and got["values_box"][2] == 1290
        f.step(before)
    f.step(after)
    got = f.step(third)
    assert 0 < got["cells_recomputed"] < 1300 * 12
    f.close()


def test_an_update_that_stages_a_whole_row_of_32768(kartohip_lib):
    before, after = cases.widest_edit()
    f = Followed(before, 3, d2_rule=cases.brute)
    got = f.step(after)
    assert got["rebuilt"] == 0 and got["values_box"] == (0, 0, 32768, 3)
    f.step(before)
    f.close()


def test_the_recount_beyond_one_grid_of_threads(kartohip_lib):
    """2052 x 1024: k_field_count's grid-stride loop; Followed.check holds the three counters against rule.stats after every step"""
    before, after = cases.count_edit()
    f = Followed(before, 8, d2_rule=cases.brute)
    assert f.field.stats["max_d2"] == 64
    got = f.step(after)
    assert got["rebuilt"] == 0 and got["cells_recomputed"] == 17 * 17
    assert f.field.stats["n_obstacles"] == 7
    f.close()
