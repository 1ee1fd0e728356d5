"""GPU: the live map (kh_live_map_*, slam_toolbox_amd.live_map.LiveMap) through the C ABI against tests/live_map_rule.py: after
every update the window is the rule's window and the counters and cells are, bit for bit, what the occupancy ORACLE gives for the
mapper's scans (pulled with kh_mapper_get_scan) on the same lattice.  No tolerance anywhere.

The mappers are the ones tests/test_localization_gpu.py builds (`_queue`, `_build_map`, BUFFER), as tests/test_session_gpu.py uses
them.  The delta path and the rebuild path are forced with rebuild_fraction inf and 0."""
import ctypes as C
import math

import numpy as np
import pytest

import live_map_rule as rule
import test_localization_gpu as loc
from common import bits
from slam_toolbox_amd import capi, synth

pytestmark = pytest.mark.gpu
BUFFER, SWITCH, LOOP_DIST = loc.BUFFER, loc.SWITCH, loc.LOOP_DIST
ANCHOR = np.array([-30.0, -30.0])           # lower left of the 60 m x 40 m world by more than the range threshold and any drift
FRACTIONS = [math.inf, 0.0, None]
FRACTION_IDS = ["delta", "rebuild", "default"]


def _mapper(**kw):
    from slam_toolbox_amd.mapper import Mapper
    return Mapper(synth.Laser(), loop_search_maximum_distance=LOOP_DIST, **kw)


def oracle_scans_of(m):
    from oracle import karto
    out = []
    for i in m.alive():
        s, _ = m.scan(int(i))
        r = np.ctypeslib.as_array(s.ranges, (s.n,)).copy()
        pts = np.ctypeslib.as_array(s.points_xy, (2 * s.n,)).copy().reshape(-1, 2)
        out.append(karto.Scan(r, np.array(s.sensor_pose[:]), points=pts))
    return out


def window_of(live):
    i = live.info()
    return i["ox"], i["oy"], i["width"], i["height"]


def assert_equals_rule(live, m, laser, previous, params=(2, 0.1), shift_cells=(0, 0), what=""):
    """window == the rule's window after `previous`; counters and cells == the oracle's on that window.  Returns the window."""
    info = live.info()
    scans = oracle_scans_of(m)
    sensors = np.array([s.sensor_pose[:2] for s in scans]).reshape(-1, 2)
    win = window_of(live)
    assert win == rule.window(previous, sensors, info["anchor"], info["resolution"], laser.range_threshold), what
    assert info["width_step"] == rule.align8(win[2]) and info["reach"] == rule.reach(laser.range_threshold, info["resolution"])
    cells, p, hits = rule.expected(win, scans, info["anchor"], info["resolution"], laser, params[0], params[1], shift_cells)
    gp, gh = live.counters()
    assert gp.shape == p.shape
    assert np.array_equal(gp, p), f"{what}: {int((gp != p).sum())} pass counters differ"
    assert np.array_equal(gh, hits), f"{what}: {int((gh != hits).sum())} hit counters differ"
    gc = live.cells()
    assert np.array_equal(gc, cells), f"{what}: {int((gc != cells).sum())} cell states differ"
    return win


def _same_live_map(a, b):
    ia, ib = a.info(), b.info()
    assert window_of(a) == window_of(b) and ia["width_step"] == ib["width_step"]
    assert np.array_equal(bits(ia["anchor"]), bits(ib["anchor"]))
    assert np.array_equal(a.cells(), b.cells())
    for x, y in zip(a.counters(), b.counters()):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("fraction", FRACTIONS, ids=FRACTION_IDS)
def test_growing_map_and_loop_closure(kartohip_lib, oracle_lib, fraction):
    """the lap queue up to the switch (1.6 laps: the first lap is closed by then) with an update every 25 accepted scans: the
    window grows, and the update behind the closure finds old scans moved"""
    laser = synth.Laser()
    ranges, odom = loc._queue()
    m = _mapper()
    live = m.live_map(0.1, ANCHOR, fraction)
    assert window_of(live) == (0, 0, 0, 0)
    win, since, poses_then, closures_then = None, 0, m.poses(), 0
    relayouts, saw_moved = 0, False
    for i in range(SWITCH):
        since += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
        if since < 25 and i != SWITCH - 1:
            continue
        last = live.update()
        win = assert_equals_rule(live, m, laser, win, what=f"queue scan {i}")
        poses = m.poses()
        moved = int(np.any(bits(poses[:len(poses_then)]) != bits(poses_then), axis=1).sum())
        closed = m.stats()["loop_closures"] > closures_then
        assert last["scans_added"] == since and last["scans_removed"] == 0
        assert last["rebuilds"] == (0 if fraction == math.inf else 1 if fraction == 0.0 else last["rebuilds"])
        if closed:
            assert moved > 0, "a closure that moved no old scan shows nothing"
        if moved:
            saw_moved = True
            # (a scan whose corrected pose moved has a moved sensor pose: the laser sits at the robot's centre)
            assert last["scans_moved"] == moved
            if fraction == math.inf:
                assert 0 < last["beams_skipped"] < moved * laser.n_beams
                print(f"closure update: {moved} scans moved, {last['beams_skipped']} beams left alone, {last['beams_traced']} lines walked")
        elif fraction == math.inf:
            assert last["scans_moved"] == 0 and last["beams_skipped"] == 0 and last["beams_traced"] <= since * laser.n_beams
        relayouts += last["relayouts"]
        since, poses_then, closures_then = 0, poses, m.stats()["loop_closures"]
    assert saw_moved and m.stats()["loop_closures"] >= 1, "the run never closed a loop"
    assert relayouts >= 2 and live.stats()["total"]["relayouts"] == relayouts, "the window never grew after the first update"
    assert live.stats()["scans_in_map"] == len(m.alive())
    live.close(); m.close()


@pytest.mark.parametrize("fraction", FRACTIONS, ids=FRACTION_IDS)
def test_removal(kartohip_lib, oracle_lib, fraction):
    """every fifth node outside the running window removed, then everything removable: the counters follow the survivors and
    nothing underflows where only removed scans had traced"""
    laser = synth.Laser()
    m, _ = loc._build_map()
    live = m.live_map(0.1, ANCHOR, fraction)
    live.update()
    win = assert_equals_rule(live, m, laser, None, what="before")
    n = m.num_scans()
    first = list(range(5, n - 2 * BUFFER, 5))
    for i in first:
        m.RemoveNode(i)
    last = live.update()
    assert last["scans_removed"] == len(first) and last["scans_added"] == 0 and last["scans_moved"] == 0
    if fraction == math.inf:
        assert last["rebuilds"] == 0 and 0 < last["beams_traced"] <= len(first) * laser.n_beams
    win = assert_equals_rule(live, m, laser, win, what="a fifth removed")
    rest = [int(i) for i in m.alive() if i < n - 2 * BUFFER]
    for i in rest:
        m.RemoveNode(i)
    assert len(m.alive()) == 2 * BUFFER
    last = live.update()
    assert last["scans_removed"] == len(rest)
    assert assert_equals_rule(live, m, laser, win, what="everything removable removed") == win, "the window never shrinks"
    p, hits = live.counters()
    assert p.max() < 2 * BUFFER * laser.n_beams, "a counter went below zero"
    assert (p == 0).sum() > p.size // 2 and hits.max() <= p.max()
    live.close(); m.close()


def test_localization_buffer(kartohip_lib, oracle_lib):
    """map, then 40 accepted localization scans with an update every 10: what the rolling buffer evicts leaves the map"""
    laser = synth.Laser()
    ranges, odom = loc._queue()
    m, _ = loc._build_map()
    n_map = m.num_scans()
    live = m.live_map(0.1, ANCHOR)
    live.update()
    win = assert_equals_rule(live, m, laser, None, what="the map")
    accepted, i, removed = 0, SWITCH, 0
    while accepted < 40:
        ok = m.ProcessLocalization(ranges[i], odom[i], 0.1 * i)[0]
        accepted += int(ok)
        i += 1
        if ok and accepted % 10 == 0:
            last = live.update()
            removed += last["scans_removed"]
            win = assert_equals_rule(live, m, laser, win, what=f"{accepted} localization scans")
            assert live.stats()["scans_in_map"] == len(m.alive()) == n_map + min(accepted, BUFFER)
    assert removed == 40 - BUFFER == m.stats()["nodes_removed"]
    live.close(); m.close()


def test_default_anchor(kartohip_lib, oracle_lib):
    """anchor NULL = kh_mapper_build_map's offset: equal to that grid on its rectangle; then the robot leaves towards negative x
    and y until the window has grown on both low sides, and a second live map made from scratch equals the first"""
    laser = synth.Laser()
    ranges, odom = loc._queue()
    m = _mapper()
    i = accepted = 0
    while accepted < 30:
        accepted += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
        i += 1
    live = m.live_map(0.05)
    live.update()
    g = m.build_map(0.05)
    info = live.info()
    assert np.array_equal(bits(info["anchor"]), bits(g.offset))
    x0, y0 = -info["ox"], -info["oy"]
    assert x0 >= 0 and y0 >= 0 and x0 + g.width <= info["width"] and y0 + g.height <= info["height"]
    for got, want in zip(live.counters() + (live.cells(),), g.counters() + (g.cells(),)):
        assert want[:, :g.width].any()
        assert np.array_equal(got[y0:y0 + g.height, x0:x0 + g.width], want[:, :g.width])
    g.close()
    first = window_of(live)
    world, rng = synth.make_world(12345), np.random.default_rng(9)
    pose = odom[i - 1].copy()                             # (HasMovedEnough measures from the last scan's ODOMETRIC pose)
    for step in range(60):
        pose[:2] -= 0.45
        assert m.Process(synth.make_scan(world, pose, rng), pose, 0.1 * (i + step))[0]
        if step % 4 == 3:
            live.update()
            if live.info()["ox"] < first[0] and live.info()["oy"] < first[1]:
                break
    live.update()
    assert live.info()["ox"] < first[0] and live.info()["oy"] < first[1], "the window never grew on the low sides"
    assert live.info()["ox"] < 0 and live.stats()["total"]["relayouts"] >= 2
    fresh = m.live_map(0.05, live.info()["anchor"], 0.0)
    assert fresh.update()["rebuilds"] == 1
    _same_live_map(fresh, live)
    assert live.counters()[0].any()
    fresh.close(); live.close(); m.close()


def test_thresholds_and_dirty_rectangle(kartohip_lib, oracle_lib):
    laser = synth.Laser()
    ranges, odom = loc._queue()
    m = _mapper()
    i = accepted = 0
    while accepted < 30:
        accepted += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
        i += 1
    live = m.live_map(0.1, ANCHOR, math.inf)
    live.update(2, 0.1)
    win = assert_equals_rule(live, m, laser, None, (2, 0.1), what="(2, 0.1)")
    before = live.cells()
    whole = live.info()["width_step"] * live.info()["height"]
    last = live.update(0, 0.5)
    assert last["scans_added"] == 0 and last["beams_traced"] == 0 and last["cells_updated"] == whole
    win = assert_equals_rule(live, m, laser, win, (0, 0.5), what="(0, 0.5)")
    assert not np.array_equal(before, live.cells())
    assert live.update(0, 0.5)["cells_updated"] == 0                  # nothing changed: nothing to do
    accepted = 0
    while accepted < 1:
        accepted += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
        i += 1
    last = live.update(0, 0.5)
    assert last["scans_added"] == 1 and last["relayouts"] == 0, "the probe scan grew the window: the rectangle is not what is tested"
    assert 0 < last["cells_updated"] < whole
    assert_equals_rule(live, m, laser, win, (0, 0.5), what="one more scan")
    live.close(); m.close()


def test_session(kartohip_lib, tmp_path):
    """a live map is not part of a session file: one made on the loaded mapper equals the original's"""
    from slam_toolbox_amd.mapper import Mapper
    m, _ = loc._build_map()
    live = m.live_map(0.1)
    live.update()
    path = str(tmp_path / "map.khms")
    m.save(path)
    m2 = Mapper.load(path)
    live2 = m2.live_map(0.1)
    last = live2.update()
    assert last["scans_added"] == len(m.alive()) and live2.stats()["updates"] == 1
    _same_live_map(live, live2)
    assert live.counters()[1].any()
    live2.close(); m2.close(); live.close(); m.close()


def test_errors(kartohip_lib):
    from slam_toolbox_amd.mapper import Mapper
    L = kartohip_lib
    m = Mapper(synth.Laser(), use_scan_matching=0, minimum_travel_distance=0.0, do_loop_closing=0)
    h = C.c_void_p()
    assert L.kh_live_map_create(None, 0.05, None, -1.0, C.byref(h)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_live_map_create(m._h, 0.05, None, -1.0, None) == capi.KH_ERR_INVALID_ARG
    anchor = np.zeros(2)
    for bad in (0.0, -0.05, math.nan, math.inf):
        assert L.kh_live_map_create(m._h, bad, anchor.ctypes.data, -1.0, C.byref(h)) == capi.KH_ERR_INVALID_ARG and not h.value
    assert L.kh_live_map_create(m._h, 0.05, None, -1.0, C.byref(h)) == capi.KH_ERR_INVALID_ARG and not h.value      # no scan, no default anchor
    assert b"anchor" in L.kh_last_error()
    assert L.kh_live_map_update(None, 2, 0.1) == capi.KH_ERR_INVALID_ARG
    assert L.kh_live_map_read(None, None, None, None) == capi.KH_ERR_INVALID_ARG
    # a window beyond the size cap: the update is refused and the map stays what it was
    scan = np.full(synth.N_BEAMS, 3.0)
    assert m.Process(scan, np.zeros(3), 0.0)[0]
    live = m.live_map(0.05, np.array([-30.0, -30.0]))
    live.update()
    info, (p, hits), cells, stats = live.info(), live.counters(), live.cells(), live.stats()
    assert p.any() and hits.any() and cells.any()
    assert m.Process(scan, np.array([1.0e5, 1.0e5, 0.0]), 1.0)[0]
    with pytest.raises(capi.KartoHipError) as err:
        live.update()
    assert err.value.code == capi.KH_ERR_INVALID_ARG and "size cap" in str(err.value)
    assert window_of(live) == (info["ox"], info["oy"], info["width"], info["height"]) and live.stats() == stats
    assert np.array_equal(live.counters()[0], p) and np.array_equal(live.counters()[1], hits) and np.array_equal(live.cells(), cells)
    # ... and a resolution so fine that one scan's window is beyond it
    fine = m.live_map(0.0004, np.array([-30.0, -30.0]))
    with pytest.raises(capi.KartoHipError) as err:
        fine.update()
    assert err.value.code == capi.KH_ERR_INVALID_ARG
    assert window_of(fine) == (0, 0, 0, 0) and fine.cells().size == 0
    # once the far scan is gone the first live map goes on (the mapper keeps its last scan, so one that traces nothing follows it)
    assert m.Process(np.full(synth.N_BEAMS, 0.05), np.zeros(3), 2.0)[0]
    m.RemoveNode(1)
    last = live.update()
    assert (last["scans_added"], last["scans_removed"], last["beams_traced"]) == (1, 0, 0)
    assert np.array_equal(live.counters()[0], p)
    fine.close(); live.close(); m.close()
