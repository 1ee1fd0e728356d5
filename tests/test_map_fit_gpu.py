"""GPU: kh_map_fit (k_map_fit in csrc/occupancy_map.hip) against tests/map_localize_rule.py on the hand-made views of
tests/map_localize_cases.py: the six counters, the derived values and the bits of the score."""
import ctypes as C

import numpy as np
import pytest

import map_localize_cases as cases
import map_localize_rule as rule
from common import LASER, bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_localizer import map_fit
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

FIT_CASES = cases.fit_cases()


def same_fit(got, want):
    for k in rule.fr.COUNTERS + ("agree", "conflict", "known"):
        assert got[k] == want[k], (k, got, want)
    assert np.array_equal(bits(got["score"]), bits(want["score"]))


@pytest.mark.parametrize("case", FIT_CASES, ids=[c.name for c in FIT_CASES])
def test_fit_cases(kartohip_lib, oracle_lib, case):
    d = DeviceView(case.view)
    got = map_fit(d.v, case.laser, case.ranges, case.poses)
    want = [rule.fit(case.view, case.laser, case.ranges, pose) for pose in case.poses]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        same_fit(g, w)
    case.check(got)
    assert np.array_equal(d.download(), case.view["cells"].ravel()), "the view's cells were written"
    d.close()


def test_a_full_scan_on_the_small_map(kartohip_lib, oracle_lib):
    """1081 beams at 0.05 m, five poses in one launch: 17 runs of 64 beams per pose, the last one ragged"""
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    sm, m = cases.small_map()
    g = OccupancyGrid.from_nav(m.nav, m.offset, cases.RESOLUTION)
    poses = np.array([sm.true_pose, sm.true_pose + [0.35, -0.2, 0.4], sm.true_pose + [-1.0, 0.5, -2.0], [m.offset[0] - 2.0, m.offset[1] + 3.0, 0.2],
                      sm.true_pose + [0.0, 0.0, 0.001]])
    got = map_fit(g, LASER, sm.query, poses)
    for k, pose in enumerate(poses):
        same_fit(got[k], rule.fit(m.view, LASER, sm.query, pose))
    assert got[0]["score"] > 0.99 > got[2]["score"]
    g.close()


def test_refused_for_walk_length(kartohip_lib):
    case = next(c for c in FIT_CASES if c.name.startswith("all eight octants"))
    d = DeviceView(case.view)
    L = kartohip_lib
    out = (capi.KhMergeFit * 2)()
    from slam_toolbox_amd.map_localizer import _laser_of

    def call(laser, poses):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        kl = _laser_of(laser)
        return L.kh_map_fit(C.byref(d.v), C.byref(kl), case.ranges.ctypes.data, len(poses), poses.ctypes.data, out)
    good = case.poses[0]
    assert call(case.laser, [good]) == capi.KH_OK
    for pose in cases.REFUSED_POSES:
        assert rule.fit_refused(case.view, case.laser, pose)
        assert call(case.laser, [good, pose]) == capi.KH_ERR_INVALID_ARG, pose
    far = cases.circle(16, range_threshold=(2 ** 20 - 1) / case.view["scale"], max_range=1e9)
    assert rule.fit_refused(case.view, far, good) and call(far, [good]) == capi.KH_ERR_INVALID_ARG
    edge = (2.0 ** 30 / case.view["scale"], 0.0, 0.0)          # the last sensor cell that is taken: nothing of it lands in the window
    assert not rule.fit_refused(case.view, case.laser, edge) and call(case.laser, [edge]) == capi.KH_OK
    assert out[0].pass_free == 0 and out[0].known == 0 and out[0].score == 0.0
    d.close()
