"""GPU: placing one map in another (kh_map_align, MapLocalizer.align; csrc/map_align.cpp) against tests/map_align_rule.py on the two
maps of tests/map_align_cases.py.  The rule takes the relocalization as a function; here it is handed the library's own relocalize --
pinned to the oracle by tests/test_map_localize_gpu.py -- so seeds, hit counts, probes, corrections, summed counters, score bits and
order are compared exactly without a minute of oracle matching."""
import ctypes as C

import numpy as np
import pytest

import map_align_cases as cases
import map_align_rule as rule
import map_localize_cases as lc
from common import LASER, OFFLINE_PARAMS, bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_localizer import MapLocalizer, map_seeds
from test_map_fit_gpu import same_fit
from test_map_localize_gpu import PARAMS
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pair(kartohip_lib, oracle_lib):
    """both maps in device memory of the test's own, a localizer on the target, and one alignment"""
    target, moving = cases.maps()
    dt, dm = DeviceView(target.view), DeviceView(moving.view)
    loc = MapLocalizer(PARAMS, LASER, max_batch=32).set_map(dt.v)
    before = dt.download(), dm.download()
    got, times = loc.align(dm.v, relocalize=cases.RELOCALIZE, **cases.SETTING)
    yield target, moving, dt, dm, loc, got, times, before
    loc.close()
    dt.close(); dm.close()


def test_alignment_equals_the_rule(pair):
    target, moving, dt, dm, loc, got, times, before = pair

    def relocalize(ranges):
        hyps, _ = loc.relocalize(ranges, cap=cases.SETTING["top_k"], top_k=cases.SETTING["top_k"], **cases.RELOCALIZE)
        return [(h.robot_pose, h.fine_response) for h in hyps]

    want = rule.align(target.view, moving.view, LASER, relocalize, **cases.SETTING)
    assert np.array_equal(map_seeds(dm.v, cases.SETTING["probe_spacing"])[0], want.seed_cells)
    assert len(want.probes) == cases.SETTING["n_probes"] and len(got) == len(want.candidates) > 1
    assert [c.index for c in got] == want.order
    for c in got:
        w, fit = want.candidates[c.index], want.fits[c.index]
        assert np.array_equal(bits(c.correction), bits(w.correction)), (c.index, c.correction, w.correction)
        assert (c.probe_seed, c.hypothesis) == (w.probe_seed, w.hypothesis) and np.array_equal(bits(c.fine_response), bits(w.fine_response))
        assert c.enough is True
        same_fit(c.fit, fit)
    assert np.array_equal(dt.download(), before[0]) and np.array_equal(dm.download(), before[1]), "an alignment wrote a map's cells"
    assert (times > 0).all() and times[3] >= times[0] + times[1] + times[2] - 1e-3


def test_alignment_undoes_the_known_motion(pair):
    target, moving, dt, dm, loc, got, times, before = pair
    best, zero = got[0], next(c for c in got if c.index == 0)
    d, dh = cases.from_the_truth(best.correction, moving)
    print(f"{len(got)} candidates; best index {best.index} (probe seed {best.probe_seed}, hypothesis {best.hypothesis}) score {best.fit['score']!r} against "
          f"{zero.fit['score']!r} of the initial correction; {d:.4f} m and {dh:.5f} rad from the truth; times {times}")
    assert best.index != 0 and best.fit["score"] > zero.fit["score"]
    assert d <= lc.FINE[0] / 2 and dh <= OFFLINE_PARAMS["coarse_angle_resolution"]
    assert np.array_equal(zero.correction, np.zeros(3)) and (zero.probe_seed, zero.hypothesis, zero.fine_response) == (-1, -1, 0.0)


def test_initial_comes_back_as_candidate_zero_and_caps_truncate(pair):
    target, moving, dt, dm, loc, got, times, before = pair
    initial = (0.25, -1.5, 0.125)
    again, _ = loc.align(dm.v, initial=initial, min_known=2 ** 40, relocalize=cases.RELOCALIZE, **cases.SETTING)
    assert len(again) == len(got)
    zero = next(c for c in again if c.index == 0)
    assert np.array_equal(bits(zero.correction), bits(initial)) and zero.probe_seed == -1
    assert not any(c.enough for c in again), "no candidate has 2^40 known visits"
    assert [c.index for c in again if c.index] == [c.index for c in got if c.index], "the others keep their order: score, agree, index"
    few, _ = loc.align(dm.v, cap=2, relocalize=cases.RELOCALIZE, **cases.SETTING)
    assert [(c.index, c.fit) for c in few] == [(c.index, c.fit) for c in got[:2]]
    n = C.c_int32()
    p = capi.KhMapAlignParams()
    capi.lib().kh_map_align_params_default(loc._h, C.byref(p))
    assert p.probe_spacing == PARAMS["loop_search_space_dimension"] / 4, "the localizer's default seed spacing"
    p.probe_spacing, p.relocalize.seed_spacing, p.relocalize.n_headings = 2.0, 2.0, 8
    assert capi.lib().kh_map_align(loc._h, C.byref(dm.v), C.byref(p), None, 0, C.byref(n), None) == capi.KH_OK
    assert n.value == len(got), "cap 0 counts"


def test_the_localizer_is_left_as_it_was(pair):
    """the next relocalize and process of a localizer that aligned are bit-identical to those of one that never did"""
    target, moving, dt, dm, loc, got, times, before = pair
    sm, _ = lc.small_map()
    fresh = MapLocalizer(PARAMS, LASER, max_batch=32).set_map(dt.v)
    start = sm.poses[3]
    answers = []
    for one in (loc, fresh):
        hyps, summary = one.relocalize(sm.ranges[3], **cases.RELOCALIZE)
        one.set_pose(start)
        step = one.process(sm.ranges[3], start)
        answers.append((hyps, {k: v for k, v in summary.items() if not k.endswith("_ms")}, step))
    (ha, sa, ta), (hb, sb, tb) = answers
    assert sa == sb and len(ha) == len(hb) >= 1
    for a, b in zip(ha, hb):
        assert a.index == b.index and a.fit == b.fit
        for f in ("coarse_mean", "coarse_cov", "coarse_response", "fine_mean", "fine_cov", "fine_response", "robot_pose"):
            assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))), f
    for f in ("predicted_pose", "robot_pose", "sensor_pose", "covariance", "response"):
        assert np.array_equal(bits(getattr(ta, f)), bits(getattr(tb, f))), f
    assert ta.fit == tb.fit
    fresh.close()


def test_refusals_and_a_map_without_a_probe(pair):
    target, moving, dt, dm, loc, got, times, before = pair

    def refused(code, call):
        with pytest.raises(capi.KartoHipError) as e:
            call()
        assert e.value.code == code
    fresh = MapLocalizer(PARAMS, LASER, max_batch=2)
    refused(capi.KH_ERR_NOT_FOUND, lambda: fresh.align(dm.v, **cases.SETTING))
    other = capi.KhMapView.from_buffer_copy(dm.v)
    other.device = 1
    refused(capi.KH_ERR_INVALID_ARG, lambda: loc.align(other, **cases.SETTING))
    refused(capi.KH_ERR_INVALID_ARG, lambda: loc.align(dm.v, **dict(cases.SETTING, probe_spacing=4097 * lc.RESOLUTION)))
    refused(capi.KH_ERR_INVALID_ARG, lambda: loc.align(dm.v, **dict(cases.SETTING, n_probes=0)))
    # free space with no wall in range: seeds, but no probe -- candidate 0 alone, fitted with nothing
    empty = DeviceView(lc.view_of(np.full((60, 60), lc.F, dtype=np.uint8), (0.0, 0.0), 20.0))
    alone, _ = loc.align(empty.v, initial=(1.0, 2.0, 0.5), **cases.SETTING)
    assert len(alone) == 1 and alone[0].index == 0 and alone[0].fit["known"] == 0 and alone[0].fit["score"] == 0.0
    assert np.array_equal(alone[0].correction, [1.0, 2.0, 0.5])
    fresh.close(); empty.close()
