"""GPU: automatic alignment of two sessions (kh_merge_align, MapMerger.align) against tests/merge_fit_rule.py.

Ground truth: the first N_SCANS scans of the lap queue of tests/test_localization_gpu.py mapped twice -- once as they are, once
with every odometric pose moved by a known rigid G -- so the second session is the first one in a frame that G carries, and the
correction that aligns it is inverse(G) up to what the two runs' matches differ by.  The moving session's current correction is
the identity: it misplaces the session by G.

test_alignment_finds_the_known_motion prints what it measured (the first-ranked candidate composed with G, in metres and radians
from the identity) before it asserts; DESIGN.md section 7a states the bounds."""
import math

import numpy as np
import pytest

import merge_fit_rule as fr
import merge_rule as rule
import test_localization_gpu as loc
import test_merge_fit_gpu as tf
import test_merge_gpu as tm
from common import bits
from slam_toolbox_amd import capi, synth
from slam_toolbox_amd.merge import MapMerger

pytestmark = pytest.mark.gpu
RES = tm.RES
N_SCANS = 60                         # 30 m up the first aisle
G = (1.5, -0.8, 0.3)
# the relocalize region: the aisle the session drove (x = 2.5, y = 3 .. 33), so a probe is tried at about a dozen seeds, and four
# headings (-pi, -pi / 2, 0, pi / 2: the drive's heading is one of them) instead of ten: 48 hypotheses per probe
PARAMS = dict(n_probes=2, top_k=3, center_xy=(2.5, 12.0), radius=10.0, n_headings=4)


def _session(motion):
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = loc._queue()
    m = Mapper(synth.Laser(), loop_search_maximum_distance=loc.LOOP_DIST)
    accepted = sum(int(m.Process(ranges[i], rule.transform_pose(motion, odom[i]), 0.1 * i)[0]) for i in range(N_SCANS))
    assert accepted >= N_SCANS // 2          # (steps of 0.5 m against minimum_travel_distance 0.5: odometric noise decides each one)
    return m


@pytest.fixture(scope="module")
def sessions(kartohip_lib):
    a, b = _session(rule.IDENTITY), _session(G)
    yield a, b
    a.close(); b.close()


def _same_candidate(got, want, fit, index, min_known=0):
    assert np.array_equal(bits(got["correction"]), bits(want.correction)), (index, got["correction"], want.correction)
    assert (int(got["probe_scan"]), int(got["hypothesis"]), int(got["index"])) == (want.probe_scan, want.hypothesis, index)
    assert bits([got["fine_response"]])[0] == bits([want.fine_response])[0]
    assert int(got["enough"]) == int(fit["known"] >= min_known)
    tf._same([got["fit"]], [fit])


def test_alignment_finds_the_known_motion(sessions, tmp_path):
    a, b = sessions
    laser = synth.Laser()
    sa, sb = tm._submap_of(a, laser, tmp_path, "a"), tm._submap_of(b, laser, tmp_path, "b")
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    got, times = mg.align(ib, ia, **PARAMS)
    # the rule, given the library's own relocalize answers for the probes
    reloc = {k: PARAMS[k] for k in ("center_xy", "radius", "n_headings")}

    def relocalize(entry):
        hyps, _ = a.relocalize(sb["scans"][entry]["ranges"], cap=PARAMS["top_k"], top_k=PARAMS["top_k"], **reloc)
        return [(h.robot_pose, h.fine_response) for h in hyps]

    ids = b.alive()
    want = fr.candidates(rule.IDENTITY, rule.IDENTITY, ids, [s["corrected"] for s in sb["scans"]], PARAMS["n_probes"], PARAMS["top_k"], relocalize)
    assert sorted({c.probe_scan for c in want}) == [-1, int(ids[0]), int(ids[len(ids) // 2])], "a probe without an accepted hypothesis"
    fits = fr.fit(sb, [c.correction for c in want], [sa], [rule.IDENTITY], RES)
    order = fr.ranking(fits)
    assert times["n_candidates"] == len(want) == len(got) and [int(g["index"]) for g in got] == order
    for g in got:
        _same_candidate(g, want[int(g["index"])], fits[int(g["index"])], int(g["index"]))
    # candidate 0 is what the submap has, and something beats it
    zero = got[[int(g["index"]) for g in got].index(0)]
    assert np.array_equal(zero["correction"], np.zeros(3)) and (int(zero["probe_scan"]), int(zero["hypothesis"]), zero["fine_response"]) == (-1, -1, 0.0)
    best = got[0]
    assert int(best["index"]) != 0 and best["fit"]["score"] > zero["fit"]["score"]
    # the truth: best . G = identity, within what the sequential matcher could have bridged
    p = a.params()
    left = rule.compose(best["correction"], G)
    distance, heading = math.hypot(left[0], left[1]), abs(left[2])
    print(f"aligned {len(sb['scans'])} scans to {len(sa['scans'])}: {len(got)} candidates, best index {int(best['index'])} (probe scan "
          f"{int(best['probe_scan'])}, hypothesis {int(best['hypothesis'])}) score {float(best['fit']['score'])!r} against {float(zero['fit']['score'])!r} "
          f"of the current correction; best . G is {distance!r} m and {heading!r} rad from the identity; times {times}")
    assert distance <= p.correlation_search_space_dimension / 2
    assert heading <= p.match.coarse_search_angle_offset
    # a cap below n truncates the output, not the count; nothing was applied
    few, t2 = mg.align(ib, ia, cap=2, **PARAMS)
    assert t2["n_candidates"] == len(want) and few.tobytes() == got[:2].tobytes()
    assert np.array_equal(mg.transform(ib), np.zeros(3)) and mg.fit_stats()["fits"] == 2
    mg.close()


def test_alignment_leaves_the_sessions_and_the_merger_as_they_were(sessions, tmp_path):
    a, b = sessions
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    mg.set_transform(ia, tf.NEAR)
    mg.set_transform(ib, tm.T1)
    before = mg.merge()
    state = [(mg.transform(i), mg.location(i)) for i in (ia, ib)]
    a.save(tmp_path / "a0.khms"); b.save(tmp_path / "b0.khms")
    got, _ = mg.align(ib, ia, **PARAMS)
    assert len(got) > 1 and np.array_equal(bits(got[[int(g["index"]) for g in got].index(0)]["correction"]), bits(np.array(tm.T1)))
    a.save(tmp_path / "a1.khms"); b.save(tmp_path / "b1.khms")
    for name in "ab":
        assert (tmp_path / f"{name}0.khms").read_bytes() == (tmp_path / f"{name}1.khms").read_bytes(), name
    for i, (t, where) in zip((ia, ib), state):
        assert np.array_equal(bits(mg.transform(i)), bits(t)) and np.array_equal(bits(mg.location(i)), bits(where))
    after = mg.merge()
    tm._assert_same_grid(after, before)
    before.close(); after.close(); mg.close()


def test_refusals(sessions):
    a, b = sessions
    c = tf._mapper(tm.SMALL_LASER, tf._poses(2, column=2), 41)
    mg = MapMerger(RES)
    ia, ib, ic = mg.add_submap(a), mg.add_submap(b), mg.add_submap(c)
    tm._error(lambda: mg.align(ib, ib, **PARAMS), capi.KH_ERR_INVALID_ARG)              # moving == target
    tm._error(lambda: mg.align(ic, ia, **PARAMS), capi.KH_ERR_INVALID_ARG)              # another laser, either way round
    tm._error(lambda: mg.align(ia, ic, **PARAMS), capi.KH_ERR_INVALID_ARG)
    assert b"laser" in capi.lib().kh_last_error()
    tm._error(lambda: mg.align(ib, 99, **PARAMS), capi.KH_ERR_NOT_FOUND)
    tm._error(lambda: mg.align(99, ia, **PARAMS), capi.KH_ERR_NOT_FOUND)
    # a fit has no such restriction, and the merger is still usable
    assert len(mg.fit(ic, [rule.IDENTITY, tf.NEAR])) == 2
    mg.close(); c.close()
