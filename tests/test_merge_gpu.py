"""GPU: merging mapping sessions into one occupancy map (kh_merge_*, slam_toolbox_amd.merge.MapMerger).

Yardsticks: kh_mapper_build_map (tests/test_session_gpu.py pins it to the host-packed path, tests/test_occupancy_gpu.py pins that to
the reference) for one submap under the identity, and tests/merge_rule.py -- the numpy restatement of the merge arithmetic that
ends at the occupancy oracle -- for everything placed by a correction.  Equality is exact: dimensions, offset bits, cells, pass
and hit counters.  The mappers are the lap map of tests/test_localization_gpu.py and a second queue with another seed."""
import ctypes as C
import math

import numpy as np
import pytest

import merge_rule as rule
import test_localization_gpu as loc
from common import bits
from slam_toolbox_amd import capi, session, synth
from slam_toolbox_amd.merge import MapMerger

pytestmark = pytest.mark.gpu
RES = 0.05
T1, T2 = (3.0, -2.0, 0.7), (-4.5, 6.25, -2.4)
SMALL_LASER = synth.Laser(n_beams=360, min_angle=math.radians(-90.0), max_angle=math.radians(90.0), ang_res=math.radians(180.0) / 359,
                          min_range=0.2, max_range=25.0, range_threshold=12.0)
_queues = {}


def _second_queue(laser, n_scans=160):
    """another circuit of the same world (aisles 1 and 2), other drift and noise seeds"""
    key = (laser.n_beams, n_scans)
    if key not in _queues:
        world = synth.make_world(12345)
        truth, odom = synth.trajectory_laps(n_scans, seed=777, aisles=(1, 2))
        rng = np.random.default_rng(9)
        ranges = np.ascontiguousarray(np.stack([synth.make_scan(world, truth[i], rng, laser) for i in range(n_scans)]))
        _queues[key] = (ranges, np.ascontiguousarray(odom))
    return _queues[key]


def _second_mapper(laser=None):
    from slam_toolbox_amd.mapper import Mapper
    laser = laser or synth.Laser()
    ranges, odom = _second_queue(laser)
    m = Mapper(laser, loop_search_maximum_distance=loc.LOOP_DIST)
    accepted = sum(int(m.Process(ranges[i], odom[i], 0.1 * i)[0]) for i in range(len(ranges)))
    assert accepted > 40
    return m


def _submap_of(m, laser, tmp_path, name):
    """the rule's view of a mapper: the poses from its session file, the readings and the barycenter from kh_mapper_get_scan, the
    box recomputed (min / max of the sensor position and the in-range readings, LocalizedRangeScan::Update Karto.h:5694-5700)"""
    path = str(tmp_path / (name + ".khms"))
    m.save(path)
    d = session.read(path)
    assert np.array_equal(d["ids"], m.alive())
    scans = []
    for k, i in enumerate(d["ids"]):
        s, b = m.scan(int(i))
        n = s.n
        ranges = np.ctypeslib.as_array(s.ranges, (n,)).copy()
        points = np.ctypeslib.as_array(s.points_xy, (2 * n,)).copy().reshape(n, 2)
        sensor = np.array(s.sensor_pose[:])
        keep = (ranges >= laser.min_range) & (ranges <= laser.range_threshold)
        xs, ys = np.concatenate([[sensor[0]], points[keep, 0]]), np.concatenate([[sensor[1]], points[keep, 1]])
        scans.append({"ranges": ranges, "points": points, "corrected": np.array(d["corrected"][k], dtype=np.float64),
                      "odometric": np.array(d["odometric"][k], dtype=np.float64),
                      "barycenter": np.array([b.barycenter[0], b.barycenter[1], 0.0 if keep.any() else sensor[2]]),
                      "box": np.array([xs.min(), ys.min(), xs.max(), ys.max()])})
    return {"laser": laser, "scans": scans}


def _assert_is(got, want):
    """an OccupancyGrid against merge_rule.merged_grid's dict"""
    assert (got.width, got.height) == (want["width"], want["height"])
    assert np.array_equal(bits(got.offset), bits(want["offset"]))
    p, h = got.counters()
    assert np.array_equal(p, want["passes"]) and np.array_equal(h, want["hits"])
    assert np.array_equal(got.cells(), want["cells"])
    hist = np.bincount(got.cells().reshape(-1), minlength=256)
    assert hist[100] > 0 and hist[255] > 0, "an empty map shows nothing"


def _assert_same_grid(got, want):
    assert (got.width, got.height, got.width_step) == (want.width, want.height, want.width_step)
    assert np.array_equal(bits(got.offset), bits(want.offset))
    assert np.array_equal(got.cells(), want.cells())
    for x, y in zip(got.counters(), want.counters()):
        assert np.array_equal(x, y)
    assert got.stats()["beams"] == want.stats()["beams"]
    hist = np.bincount(got.cells().reshape(-1), minlength=256)
    assert hist[100] > 0 and hist[255] > 0, "an empty map shows nothing"


def _same_bits(a, b):
    """bit equality; two NaNs count as equal whatever their payload (a reading of infinite range turns into inf - inf, and the
    payload of a NaN is not arithmetic)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_one_submap_under_the_identity_is_build_map(kartohip_lib):
    m, _ = loc._build_map()
    mg = MapMerger(RES)
    sid = mg.add_submap(m)
    assert mg.num_submaps() == 1 and mg.submap_info(sid) == {"n_scans": len(m.alive()), "n_beams": synth.N_BEAMS}
    assert np.array_equal(mg.transform(sid), np.zeros(3))
    got, sub, want = mg.merge(), mg.submap_map(sid), m.build_map(RES)
    _assert_same_grid(got, want)
    _assert_same_grid(sub, want)
    st = mg.stats()
    assert st["merges"] == 1 and st["scans_traced"] == len(m.alive()) and st["beams_traced"] == len(m.alive()) * synth.N_BEAMS
    for g in (got, sub, want):
        g.close()
    mg.close(); m.close()


def test_two_submaps_equal_the_rule(kartohip_lib, tmp_path):
    a, _ = loc._build_map()
    b = _second_mapper()
    laser = synth.Laser()
    sa, sb = _submap_of(a, laser, tmp_path, "a"), _submap_of(b, laser, tmp_path, "b")
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    for t in (T1, T2):
        mg.set_transform(ib, t)
        assert np.array_equal(bits(mg.transform(ib)), bits(np.array(t)))
        got = mg.merge()
        _assert_is(got, rule.merged_grid([sa, sb], [rule.IDENTITY, t], RES))
        print(f"two submaps at {t}: {got.width} x {got.height}, trace {got.stats()['trace_ms']:.3f} ms for {got.stats()['beams']} beams")
        got.close()
    # both placed, and another Update rule
    mg.set_transform(ia, T2)
    got = mg.merge(min_pass_through=3, occupancy_threshold=0.25)
    _assert_is(got, rule.merged_grid([sa, sb], [T2, T2], RES, 3, 0.25))
    got.close(); mg.close(); a.close(); b.close()


def test_two_different_lasers(kartohip_lib, tmp_path):
    a, _ = loc._build_map()
    b = _second_mapper(SMALL_LASER)
    sa, sb = _submap_of(a, synth.Laser(), tmp_path, "a"), _submap_of(b, SMALL_LASER, tmp_path, "b")
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    assert mg.submap_info(ib)["n_beams"] == 360
    mg.set_transform(ib, T1)
    got = mg.merge()
    _assert_is(got, rule.merged_grid([sa, sb], [rule.IDENTITY, T1], RES))
    assert mg.stats()["beams_traced"] == len(a.alive()) * synth.N_BEAMS + len(b.alive()) * 360
    got.close()
    # the short laser first: the run count per scan follows the scan's submap in either order
    mg2 = MapMerger(RES)
    jb, ja = mg2.add_submap(b), mg2.add_submap(a)
    mg2.set_transform(ja, T2)
    got = mg2.merge()
    _assert_is(got, rule.merged_grid([sb, sa], [rule.IDENTITY, T2], RES))
    got.close(); mg.close(); mg2.close(); a.close(); b.close()


def test_transformed_scan_of_every_scan(kartohip_lib, tmp_path):
    b = _second_mapper()
    sb = _submap_of(b, synth.Laser(), tmp_path, "b")
    mg = MapMerger(RES)
    ib = mg.add_submap(b)
    for t in (rule.IDENTITY, T1, T2):
        mg.set_transform(ib, t)
        for k, s in enumerate(sb["scans"]):
            got, want = mg.transformed_scan(ib, k), rule.transformed_scan(t, s)
            for key in ("corrected", "odometric", "barycenter", "box"):
                assert np.array_equal(bits(got[key]), bits(want[key])), (t, k, key)
            assert _same_bits(got["points"], want["points"]), (t, k)
            assert np.isfinite(got["points"]).all(axis=1).sum() > synth.N_BEAMS // 2
    with pytest.raises(capi.KartoHipError) as e:
        mg.transformed_scan(ib, len(sb["scans"]))
    assert e.value.code == capi.KH_ERR_NOT_FOUND
    mg.close(); b.close()


def test_move_submap_follows_the_release_rule(kartohip_lib, tmp_path):
    a, _ = loc._build_map()
    b = _second_mapper()
    laser = synth.Laser()
    sa, sb = _submap_of(a, laser, tmp_path, "a"), _submap_of(b, laser, tmp_path, "b")
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    correction, location = np.zeros(3), rule.initial_location(sb, RES)
    assert np.array_equal(bits(mg.location(ib)), bits(location))
    assert np.array_equal(bits(mg.location(ia)), bits(rule.initial_location(sa, RES)))
    for marker in ((location[0] + 2.5, location[1] - 1.25, 0.0), (20.0, 11.5, 0.6), (18.75, 12.0, -1.9)):
        mg.move_submap(ib, marker)
        correction, location = rule.release(correction, location, marker)
        assert np.array_equal(bits(mg.transform(ib)), bits(correction)), marker
        assert np.array_equal(bits(mg.location(ib)), bits(location)), marker
    assert abs(correction[2]) > 0.5
    got = mg.merge()
    _assert_is(got, rule.merged_grid([sa, sb], [rule.IDENTITY, correction], RES))
    got.close(); mg.close(); a.close(); b.close()


def test_residency(kartohip_lib):
    """a re-merge after set_transform moves no reading; new scans of a borrowed mapper move exactly what build_map would move; and
    build_map between merges keeps its own counters"""
    ranges, odom = loc._queue()
    a, _ = loc._build_map()
    twin, _ = loc._build_map()                       # the same run: what build_map alone would upload
    b = _second_mapper()
    n_a, n_b = len(a.alive()), len(b.alive())
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    mg.merge().close()
    twin.build_map(RES).close()
    st, st_twin = mg.stats(), twin.map_stats()
    assert st["scans_traced"] == n_a + n_b and st["range_uploads"] == n_a + n_b and st["point_uploads"] <= n_a + n_b
    mg.set_transform(ib, T1)
    mg.merge().close()
    st = mg.stats()
    assert st["merges"] == 2 and st["point_uploads"] == 0 and st["range_uploads"] == 0
    assert 0 < st["table_bytes"] <= 64 * st["scans_traced"]
    print(f"re-merge of {st['scans_traced']} scans / {st['beams_traced']} beams: {st['table_bytes']} table bytes, no reading uploaded")
    i, more = loc.SWITCH, 0
    while more < 5:
        ok = a.Process(ranges[i], odom[i], 0.1 * i)[0]
        assert twin.Process(ranges[i], odom[i], 0.1 * i)[0] == ok
        more += int(ok)
        i += 1
    twin.build_map(RES).close()
    mg.merge().close()
    st, st_twin = mg.stats(), twin.map_stats()
    assert st["scans_traced"] == n_a + 5 + n_b and st_twin["scans_traced"] == n_a + 5
    assert st["range_uploads"] == st_twin["range_uploads"] == 5 and st["point_uploads"] == st_twin["point_uploads"]
    # build_map of the borrowed mapper between merges: its counters are its own, and the merge has left it nothing to upload
    assert a.map_stats()["calls"] == 0
    mine, theirs = a.build_map(RES), twin.build_map(RES)
    _assert_same_grid(mine, theirs)
    ms = a.map_stats()
    assert ms["calls"] == 1 and ms["scans_traced"] == n_a + 5 and ms["point_uploads"] == 0 and ms["range_uploads"] == 0
    assert ms["point_uploads_total"] == 0 and ms["range_uploads_total"] == 0
    mg.merge().close()
    st = mg.stats()
    assert st["merges"] == 4 and st["point_uploads"] == 0 and st["range_uploads"] == 0
    assert st["range_uploads_total"] == n_a + n_b + 5
    mine.close(); theirs.close(); mg.close(); a.close(); b.close(); twin.close()


def test_sessions_and_removals(kartohip_lib, tmp_path):
    """a session file is the live mapper; removed nodes and a rolled localization buffer are not traced"""
    ranges, odom = loc._queue()
    a, _ = loc._build_map()
    n = a.num_scans()
    for i in range(5, n - 2 * loc.BUFFER, 5):
        a.RemoveNode(i)
    i = loc.SWITCH
    while a.stats()["nodes_removed"] < (n - 2 * loc.BUFFER - 5 + 4) // 5 + 3:           # ... and three evictions of the rolling buffer
        a.ProcessLocalization(ranges[i], odom[i], 0.1 * i)
        i += 1
    assert len(a.localization_buffer()) == loc.BUFFER and len(a.alive()) < a.num_scans()
    b = _second_mapper()
    laser = synth.Laser()
    sa, sb = _submap_of(a, laser, tmp_path, "a"), _submap_of(b, laser, tmp_path, "b")
    live, files = MapMerger(RES), MapMerger(RES)
    for mg, subs in ((live, (a, b)), (files, (str(tmp_path / "a.khms"), str(tmp_path / "b.khms")))):
        ids = [mg.add_submap(s) for s in subs]
        mg.set_transform(ids[1], T1)
        assert mg.submap_info(ids[0])["n_scans"] == len(a.alive())
    got_live, got_files = live.merge(), files.merge()
    want = rule.merged_grid([sa, sb], [rule.IDENTITY, T1], RES)
    _assert_is(got_live, want)
    _assert_is(got_files, want)
    _assert_same_grid(got_files, got_live)
    assert live.stats()["scans_traced"] == files.stats()["scans_traced"] == len(a.alive()) + len(b.alive())
    # a submap taken out again: what is left is the other one alone
    files.remove_submap(0)
    assert files.num_submaps() == 1
    alone = files.merge()
    _assert_is(alone, rule.merged_grid([sb], [T1], RES))
    for g in (got_live, got_files, alone):
        g.close()
    live.close(); files.close(); a.close(); b.close()


def _error(call, code):
    with pytest.raises(capi.KartoHipError) as e:
        call()
    assert e.value.code == code, e.value
    assert len(capi.lib().kh_last_error()) > 10, "no kh_last_error() text"


def test_errors(kartohip_lib, tmp_path):
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = loc._queue()
    mg = MapMerger(RES)
    _error(mg.merge, capi.KH_ERR_INVALID_ARG)                                    # no submap
    empty = Mapper(synth.Laser())
    ie = mg.add_submap(empty)
    _error(mg.merge, capi.KH_ERR_INVALID_ARG)                                    # no scan in any submap
    _error(lambda: mg.add_submap(empty), capi.KH_ERR_INVALID_ARG)                # twice the same mapper
    for call in (lambda: mg.set_transform(99, T1), lambda: mg.transform(99), lambda: mg.move_submap(99, T1), lambda: mg.location(99),
                 lambda: mg.submap_map(99), lambda: mg.remove_submap(99), lambda: mg.transformed_scan(99, 0), lambda: mg.submap_info(99)):
        _error(call, capi.KH_ERR_NOT_FOUND)
    _error(lambda: mg.add_submap(str(tmp_path / "missing.khms")), capi.KH_ERR_IO)
    bad = tmp_path / "bad.khms"
    bad.write_bytes(b"not a session file" * 8)
    _error(lambda: mg.add_submap(str(bad)), capi.KH_ERR_IO)
    assert mg.num_submaps() == 1
    mg.remove_submap(ie)
    empty.close()
    # destroying the merger leaves a borrowed mapper usable
    m, _ = loc._build_map()
    mg.add_submap(m)
    mg.merge().close()
    mg.close()
    i, more = loc.SWITCH, 0
    while more < 1:
        more += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
        i += 1
    g = m.build_map(RES)
    assert g.stats()["beams"] == len(m.alive()) * synth.N_BEAMS and m.map_stats()["range_uploads"] == 1
    g.close(); m.close()


def test_a_mapper_on_another_device_is_refused(kartohip_lib):
    from slam_toolbox_amd.mapper import Mapper
    if capi.lib().kh_device_count() < 2:
        pytest.skip("one device visible")
    m = Mapper(synth.Laser(), device=1)
    mg = MapMerger(RES, device=0)
    _error(lambda: mg.add_submap(m), capi.KH_ERR_INVALID_ARG)
    assert b"device" in capi.lib().kh_last_error()
    mg.close(); m.close()
