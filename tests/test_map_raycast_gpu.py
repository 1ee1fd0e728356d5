"""GPU: kh_map_raycast (k_map_raycast in csrc/occupancy_map.hip) against tests/map_raycast_rule.py on the hand-made views of
tests/map_raycast_cases.py, uploaded through kh_device_upload, and on the small map: cells, steps, codes and the bits of the ranges."""
import ctypes as C
import math

import numpy as np
import pytest

import map_localize_cases as lc
import map_localize_rule as ml
import map_raycast_cases as cases
import map_raycast_rule as rule
from common import LASER, OFFLINE_PARAMS, bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_localizer import MapLocalizer, _laser_of, map_raycast, ray_no_return
from test_map_localize_gpu import PARAMS, region
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

RAY_CASES = cases.ray_cases()


def same_cast(got, want):
    assert np.array_equal(got.codes, want.codes), (got.codes.tolist(), want.codes.tolist())
    assert np.array_equal(got.steps, want.steps) and np.array_equal(got.cells, want.cells)
    assert np.array_equal(bits(got.ranges), bits(want.ranges))


@pytest.mark.parametrize("case", RAY_CASES, ids=[c.name for c in RAY_CASES])
def test_ray_cases(kartohip_lib, oracle_lib, case):
    d = DeviceView(case.view)
    got = map_raycast(d.v, case.laser, case.poses, case.max_unknown, case.no_return)
    want = rule.cast_poses(case.view, case.laser, case.poses, case.max_unknown, case.no_return)
    same_cast(got, want)
    case.check(got)
    assert np.array_equal(d.download(), case.view["cells"].ravel()), "the view's cells were written"
    d.close()


def test_default_no_return(kartohip_lib):
    assert ray_no_return(LASER) == rule.default_no_return(LASER)
    assert math.isnan(ray_no_return(lc.CaseLaser(4, 0.0, 0.1, 0.1, 5.0, 5.0)))


def test_refused_inputs(kartohip_lib):
    case = next(c for c in RAY_CASES if c.name.startswith("all eight octants"))
    d = DeviceView(case.view)
    L = kartohip_lib
    out = (capi.KhRay * 64)()

    def call(laser, poses, budget=-1):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        kl = _laser_of(laser)
        return L.kh_map_raycast(C.byref(d.v), C.byref(kl), len(poses), poses.ctypes.data, budget, math.nan, out, None)
    good = case.poses[0]
    assert call(case.laser, [good]) == capi.KH_OK
    assert call(case.laser, [good], -2) == capi.KH_ERR_INVALID_ARG
    for pose in lc.REFUSED_POSES:
        assert rule.cast_refused(case.view, case.laser, pose, -1)
        assert call(case.laser, [good, pose]) == capi.KH_ERR_INVALID_ARG, pose
    far = lc.circle(16, range_threshold=(2 ** 20 - 1) / case.view["scale"], max_range=1e9)
    assert rule.cast_refused(case.view, far, good, -1) and call(far, [good]) == capi.KH_ERR_INVALID_ARG
    edge = (2.0 ** 30 / case.view["scale"], 0.0, 0.0)          # the last sensor cell that is taken: nothing of the window on its lines
    assert call(case.laser, [edge]) == capi.KH_OK and all(out[b].code == capi.KH_RAY_FREE and math.isnan(out[b].range) for b in range(16))
    assert call(case.laser, [edge], 4) == capi.KH_OK and all(out[b].code == capi.KH_RAY_UNKNOWN and out[b].steps == 4 for b in range(16))
    w = capi.KhMapView.from_buffer_copy(d.v)
    w.device = 1 << 20
    kl, pose = _laser_of(case.laser), np.ascontiguousarray(good)
    assert L.kh_map_raycast(C.byref(w), C.byref(kl), 1, pose.ctypes.data, -1, math.nan, out, None) == capi.KH_ERR_NO_DEVICE
    assert np.array_equal(d.download(), case.view["cells"].ravel())
    d.close()


@pytest.fixture(scope="module")
def small(kartohip_lib, oracle_lib):
    sm, m = lc.small_map()
    d = DeviceView(m.view)
    loc = MapLocalizer(PARAMS, LASER, max_batch=24).set_map(d.v)
    yield sm, m, d, loc
    loc.close()
    d.close()


def test_cast_at_the_held_out_pose_equals_the_rule(small):
    """1081 beams at 0.05 m, three poses in one launch: 17 runs of 64 beams per pose, the last one ragged"""
    sm, m, d, loc = small
    before = d.download()
    poses = np.array([sm.true_pose, sm.true_pose + [0.35, -0.2, 0.4], [m.offset[0] - 2.0, m.offset[1] + 3.0, 0.2]])
    for budget, counts in cases.SMALL_MAP_COUNTS.items():
        got = loc.expected(poses, budget)
        same_cast(got, rule.cast_poses(m.view, LASER, poses, budget))
        assert cases.counts(got.codes[0]) == counts and got.kernel_ms > 0
    one = loc.expected(sm.true_pose, 20)
    assert one.ranges.shape == (1, LASER.n_beams) and np.array_equal(bits(one.ranges[0]), bits(got.ranges[0]))
    assert np.array_equal(d.download(), before), "the cast wrote the view's cells"


def test_the_cast_scan_relocalizes_where_it_was_cast(small):
    sm, m, d, loc = small
    cast = loc.expected(sm.true_pose).ranges[0]
    hyps, summary = loc.relocalize(cast, **region())
    assert summary["n_returned"] >= 1
    best = hyps[0]
    dist = math.hypot(best.robot_pose[0] - sm.true_pose[0], best.robot_pose[1] - sm.true_pose[1])
    dh = abs(ml.normalize_angle(best.robot_pose[2] - sm.true_pose[2]))
    print(f"the cast scan: fine response {best.fine_response:.4f}, {dist:.4f} m and {dh:.5f} rad from where it was cast, fit {best.fit['score']:.5f}")
    assert dist <= 0.5 * math.sqrt(2.0) * lc.RESOLUTION + 0.01
    assert dh <= OFFLINE_PARAMS["fine_search_angle_offset"]


def test_expected_needs_a_map(kartohip_lib):
    fresh = MapLocalizer(PARAMS, LASER, max_batch=2)
    with pytest.raises(capi.KartoHipError) as e:
        fresh.expected(np.zeros(3))
    assert e.value.code == capi.KH_ERR_NOT_FOUND
    fresh.close()
