"""GPU: the map feed (kh_map_feed_*, slam_toolbox_amd.live_map.MapFeed; k_nav_feed in csrc/occupancy_live.hip) through small mappers
that place their scans where the test says (tests/test_live_map_edges_gpu.py), against tests/map_feed_rule.py and the occupancy
oracle.  After EVERY poll (Consumer.poll):

  (a) the consumer's map, patched from the tiles the poll handed out, equals to_nav of the oracle's cells on the feed's window;
  (b) the tile list equals tiles_that_differ(consumer before, expected): no tile more, none fewer, in ascending (ty, tx) order;
  (c) bytes_downloaded <= 16 + 264 * n_tiles.

No tolerance anywhere.  min_pass_through is 0 unless a test says otherwise, so that one scan already makes known cells."""
import ctypes as C
import math

import numpy as np
import pytest

import live_map_rule as rule
import map_feed_rule as mf
from slam_toolbox_amd import capi, synth
from test_live_map_edges_gpu import LOW_LEFT, _keeper, _place, _synthetic, placing_mapper
from test_live_map_gpu import oracle_scans_of, window_of

pytestmark = pytest.mark.gpu
RES = 0.1
PARAMS = (0, 0.1)


def expected_nav(live, m, laser, win, params=PARAMS, shift=(0, 0)):
    info = live.info()
    cells = rule.expected(win, oracle_scans_of(m), info["anchor"], info["resolution"], laser, params[0], params[1], shift)[0]
    return mf.to_nav(cells[:, :win[2]])


class Consumer:
    """a feed and the map of the consumer it serves"""

    def __init__(self, live, m, laser, shift=(0, 0)):
        self.live, self.m, self.laser, self.shift = live, m, laser, shift
        self.feed = live.feed()
        self.map = None                    # (nav, window), tests/map_feed_rule.patch

    def poll(self, params=PARAMS, want=None, what=""):
        """one poll with the three assertions; `want` = expected_nav of the live window where the caller has it already.
        Returns (delta, tile_xy)."""
        delta, xy, data = self.feed.poll()
        n = delta["n_tiles"]
        assert xy.shape == (n, 2) and data.shape == (n, 16, 16)
        win = (delta["ox"], delta["oy"], delta["width"], delta["height"])
        print(f"{what}: {n} tiles of {delta['tiles_scanned']} scanned, {delta['bytes_downloaded']} bytes, window {win}")
        assert delta["bytes_downloaded"] <= 16 + 264 * n, what                                  # (c)
        if win[2] == 0:
            assert n == 0 and delta["tiles_scanned"] == 0 and self.map is None, what
            return delta, xy
        assert win == window_of(self.live) or delta["tiles_scanned"] == 0, what
        if want is None:
            want = expected_nav(self.live, self.m, self.laser, win, params, self.shift)
        before = mf.patch(self.map, win, [], [])
        tiles = mf.tiles_that_differ(before[0], want, win[0], win[1])
        assert np.array_equal(xy, tiles), f"{what}: reported {xy.tolist()}, the rule says {tiles.tolist()}"      # (b)
        self.map = mf.patch(before, win, xy, data)
        assert np.array_equal(self.map[0], want), f"{what}: {int((self.map[0] != want).sum())} cells of the consumer differ"      # (a)
        assert delta["tiles_scanned"] <= win[2] * win[3] // 256
        if n:
            assert (delta["x"], delta["y"]) == (16 * int(xy[:, 0].min()), 16 * int(xy[:, 1].min())), what
            assert (delta["w"], delta["h"]) == (16 * int(np.ptp(xy[:, 0]) + 1), 16 * int(np.ptp(xy[:, 1]) + 1)), what
        else:
            assert (delta["x"], delta["y"], delta["w"], delta["h"]) == (0, 0, 0, 0), what
        return delta, xy

    def close(self):
        self.feed.close()


def _whole(live):
    i = live.info()
    return i["width"] * i["height"] // 256


def test_first_poll_idle_added_moved_removed(kartohip_lib, oracle_lib):
    laser = synth.Laser()
    _, ranges = _synthetic(2, 11)
    pose = np.array([10.0, 12.0, 0.25])
    m = placing_mapper(laser)
    live = m.live_map(RES, LOW_LEFT, math.inf)
    c = Consumer(live, m, laser)
    delta, _ = c.poll(what="before the live map has a window")
    assert delta["n_tiles"] == 0 and delta["tiles_scanned"] == 0 and delta["width"] == 0
    _place(m, ranges[0], pose, 0)
    live.update(*PARAMS)
    delta, xy = c.poll(what="first poll")
    assert 0 < delta["n_tiles"] < delta["tiles_scanned"] == _whole(live)
    assert set(np.unique(c.map[0]).tolist()) == {-1, 0, 100}
    delta, _ = c.poll(what="no update in between")
    assert (delta["n_tiles"], delta["tiles_scanned"], delta["bytes_downloaded"]) == (0, 0, 0)
    # one scan added, close enough for the window to stay: the rectangle around it is scanned, not the window
    _place(m, ranges[1], [10.5, 12.3, -1.0], 1)
    _keeper(m, [10.5, 12.3, -1.0], 2)
    last = live.update(*PARAMS)
    assert last["relayouts"] == 0 and last["scans_added"] == 2
    delta, _ = c.poll(what="one scan added")
    assert 0 < delta["n_tiles"] < delta["tiles_scanned"] < _whole(live)
    # one scan moved by exactly one cell
    cell = rule.cells_of(pose[:2], LOW_LEFT, RES)
    moved = pose + np.array([RES, 0.0, 0.0])
    assert (rule.cells_of(moved[:2], LOW_LEFT, RES) - cell).tolist() == [[1, 0]]
    m.set_scan_pose(0, moved)
    last = live.update(*PARAMS)
    assert (last["scans_added"], last["scans_moved"], last["relayouts"]) == (0, 1, 0)
    delta, _ = c.poll(what="one scan moved by one cell")
    assert 0 < delta["n_tiles"] < delta["tiles_scanned"] < _whole(live)
    # one scan removed: the tiles that revert are reported
    known = int((c.map[0] != -1).sum())
    m.RemoveNode(0)
    assert live.update(*PARAMS)["scans_removed"] == 1
    delta, _ = c.poll(what="one scan removed")
    assert delta["n_tiles"] > 0 and int((c.map[0] != -1).sum()) < known
    st = c.feed.stats()
    assert st["polls"] == 6 and st["n_tiles"] > delta["n_tiles"] and st["bytes_downloaded"] <= 6 * 16 + 264 * st["n_tiles"]
    c.close(); live.close(); m.close()


def test_counters_change_but_no_state_does(kartohip_lib, oracle_lib):
    """three identical scans at one pose, then a fourth: every counter of the scan's cells grows, every ratio stays what it was"""
    laser = synth.Laser()
    _, ranges = _synthetic(1, 12)
    pose = [9.0, 14.0, 0.5]
    m = placing_mapper(laser)
    live = m.live_map(RES, LOW_LEFT, math.inf)
    c = Consumer(live, m, laser)
    for k in range(3):
        _place(m, ranges[0], pose, k)
    live.update(*PARAMS)
    assert c.poll(what="three identical scans")[0]["n_tiles"] > 0
    before = live.counters()[0]
    _place(m, ranges[0], pose, 3)
    last = live.update(*PARAMS)
    assert last["scans_added"] == 1 and last["cells_updated"] > 0 and last["beams_traced"] > 0
    assert (live.counters()[0] != before).any()
    delta, _ = c.poll(what="a fourth")
    assert delta["tiles_scanned"] > 0 and delta["n_tiles"] == 0 and delta["bytes_downloaded"] <= 16
    c.close(); live.close(); m.close()


def test_parameter_change(kartohip_lib, oracle_lib):
    laser = synth.Laser()
    poses, ranges = _synthetic(4, 13)
    m = placing_mapper(laser)
    live = m.live_map(RES, LOW_LEFT, math.inf)
    c = Consumer(live, m, laser)
    for k in range(4):
        _place(m, ranges[k], poses[k], k)
    live.update(0, 0.1)
    c.poll((0, 0.1), what="min_pass_through 0")
    last = live.update(2, 0.1)
    assert last["scans_added"] == 0 and last["cells_updated"] == live.info()["width_step"] * live.info()["height"]
    delta, _ = c.poll((2, 0.1), what="min_pass_through 2")
    assert delta["tiles_scanned"] == _whole(live) and 0 < delta["n_tiles"] < delta["tiles_scanned"]
    c.close(); live.close(); m.close()


def test_two_updates_and_a_window_that_grows_on_both_low_sides(kartohip_lib, oracle_lib):
    laser = synth.Laser()
    poses, ranges = _synthetic(3, 14)
    m = placing_mapper(laser)
    live = m.live_map(RES, LOW_LEFT, math.inf)
    c = Consumer(live, m, laser)
    _place(m, ranges[0], [24.0, 22.0, 0.1], 0)
    live.update(*PARAMS)
    first, first_xy = c.poll(what="first window")
    old = window_of(live)
    _place(m, np.full(laser.n_beams, 1.0), [24.4, 22.2, 2.0], 1)         # (every beam ends a metre away: most old tiles stay what they were)
    assert live.update(*PARAMS)["relayouts"] == 0
    _place(m, ranges[2], [11.0, 9.0, -0.7], 2)
    assert live.update(*PARAMS)["relayouts"] == 1
    new = window_of(live)
    assert new[0] < old[0] and new[1] < old[1] and new[0] + new[2] == old[0] + old[2] and new[1] + new[3] == old[1] + old[3]
    delta, xy = c.poll(what="two updates, the second grew the window")
    assert (delta["ox"], delta["oy"], delta["width"], delta["height"]) == new and delta["tiles_scanned"] == _whole(live)
    # (assertion (b) has shown that no tile of the old window came again unless it changed; this says that some stayed away)
    again = set(map(tuple, first_xy.tolist())) & set(map(tuple, xy.tolist()))
    assert delta["n_tiles"] > 0 and len(again) < first["n_tiles"]
    assert np.array_equal(c.feed.read(*new), c.map[0])
    c.close(); live.close(); m.close()


def test_delta_and_rebuild_paths_report_the_same_tiles(kartohip_lib, oracle_lib):
    """two live maps on one mapper, rebuild_fraction inf and 0: tile for tile the same feed"""
    laser = synth.Laser()
    poses, ranges = _synthetic(5, 15)
    m = placing_mapper(laser)
    lives = [m.live_map(RES, LOW_LEFT, f) for f in (math.inf, 0.0)]
    cons = [Consumer(live, m, laser) for live in lives]

    def step(what, rebuilds):
        got = []
        want = None
        for live, c, r in zip(lives, cons, rebuilds):
            assert live.update(*PARAMS)["rebuilds"] == r
            if want is None:
                want = expected_nav(live, m, laser, window_of(live))
            assert window_of(live) == window_of(lives[0])
            delta, xy = c.poll(want=want, what=what)
            got.append((xy, c.map[0].copy(), delta["n_tiles"]))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][2] == got[1][2] > 0, what

    for k in range(3):
        _place(m, ranges[k], poses[k], k)
    step("three scans", (0, 1))
    _place(m, ranges[3], poses[3], 3)
    step("one added", (0, 1))
    m.set_scan_pose(1, poses[1] + np.array([0.3, -0.2, 0.05]))
    step("one moved", (0, 1))
    _keeper(m, poses[3], 4)
    m.RemoveNode(0)
    step("one removed", (0, 1))
    for c in cons:
        c.close()
    for live in lives:
        live.close()
    m.close()


def test_anchor_inside_the_map(kartohip_lib, oracle_lib):
    """an anchor in the middle of the scans: tiles left of and below it have negative coordinates.  The oracle sees the lattice from
    an anchor 1024 cells further down-left, which is exact here (resolution 2^-4; checked on the very points)"""
    res, anchor, shift = 0.0625, np.array([16.0, 16.0]), (1024, 1024)
    laser = synth.Laser()
    poses, ranges = _synthetic(6, 5)
    m = placing_mapper(laser)
    live = m.live_map(res, anchor, math.inf)
    c = Consumer(live, m, laser, shift)

    def exact():
        scans = oracle_scans_of(m)
        pts = np.concatenate([s.points for s in scans] + [np.array([s.sensor_pose[:2] for s in scans])])
        assert rule.shift_is_exact(pts, anchor, shift, res)

    for k in range(3):
        _place(m, ranges[k], poses[k], k)
    live.update(*PARAMS)
    exact()
    delta, xy = c.poll(what="anchor inside, three scans")
    assert delta["ox"] < 0 and delta["oy"] < 0 and (xy[:, 0] < 0).any() and (xy[:, 1] < 0).any() and (xy > 0).any()
    assert delta["x"] < 0 and delta["y"] < 0
    for k in range(3, 6):
        _place(m, ranges[k], poses[k], k)
    live.update(*PARAMS)
    exact()
    c.poll(what="anchor inside, six scans")
    m.RemoveNode(1)
    live.update(*PARAMS)
    delta, xy = c.poll(what="anchor inside, one removed")
    assert delta["n_tiles"] > 0
    win = window_of(live)
    assert np.array_equal(c.feed.read(*win), c.map[0])
    c.close(); live.close(); m.close()


def test_single_cells_in_tile_corners(kartohip_lib, oracle_lib):
    # from the rule alone, before the library is touched: one tile changes in exactly one cell in its last row and column, another
    # in exactly one cell in its first row and column
    last, first = mf.corner_precondition()
    assert last[2:] == (15, 15) and first[2:] == (0, 0)
    win, want = mf.corner_expected()
    tiles = mf.tiles_that_differ(np.full(want.shape, -1, dtype=np.int8), want, win[0], win[1])
    assert list(last[:2]) in tiles.tolist() and list(first[:2]) in tiles.tolist()
    small = synth.Laser(n_beams=3, min_angle=0.0, max_angle=math.pi, ang_res=math.pi / 2)      # beam 0 points along +x exactly
    m = placing_mapper(small)
    live = m.live_map(mf.CORNER_RESOLUTION, np.array(mf.CORNER_ANCHOR), math.inf)
    c = Consumer(live, m, small, mf.CORNER_SHIFT)
    for k, (pose, r, pts) in enumerate(mf.corner_scans()):
        _place(m, r, pose, k)
        got = np.ctypeslib.as_array(m.scan(k)[0].points_xy, (6,))[:2].copy()
        assert np.array_equal(got, pts[0]), "beam 0 does not end where the test computes"
    live.update(*PARAMS)
    assert window_of(live) == win
    delta, xy = c.poll(what="corner cells")
    assert np.array_equal(xy, tiles) and np.array_equal(c.map[0], want)
    for tx, ty, row, col in (last, first):
        assert [tx, ty] in xy.tolist()
        tile = c.feed.read(16 * tx, 16 * ty, 16, 16)
        assert tile[row, col] != -1 and int((tile != -1).sum()) == 1, (tx, ty)
    c.close(); live.close(); m.close()


def test_two_feeds_at_their_own_pace(kartohip_lib, oracle_lib):
    laser = synth.Laser()
    poses, ranges = _synthetic(6, 16)
    m = placing_mapper(laser)
    live = m.live_map(RES, LOW_LEFT, math.inf)
    every, third = Consumer(live, m, laser), Consumer(live, m, laser)
    polled = 0
    for k in range(6):
        _place(m, ranges[k], poses[k], k)
        if k == 3:
            m.set_scan_pose(0, poses[0] + np.array([0.2, 0.1, -0.02]))
        if k == 4:
            m.RemoveNode(2)
        live.update(*PARAMS)
        want = expected_nav(live, m, laser, window_of(live))
        every.poll(want=want, what=f"every update, {k}")
        if k % 3 == 2:
            delta, _ = third.poll(want=want, what=f"every third update, {k}")
            polled += 1
            assert delta["n_tiles"] > 0
    assert polled == 2 and every.feed.stats()["polls"] == 6 and third.feed.stats()["polls"] == 2
    assert every.map[1] == third.map[1] == window_of(live) and np.array_equal(every.map[0], third.map[0])
    assert np.array_equal(every.feed.read(*window_of(live)), third.feed.read(*window_of(live)))
    third.close(); every.close(); live.close(); m.close()


def test_read(kartohip_lib, oracle_lib):
    laser = synth.Laser()
    poses, ranges = _synthetic(2, 17)
    m = placing_mapper(laser)
    live = m.live_map(RES, LOW_LEFT, math.inf)
    c = Consumer(live, m, laser)
    assert (c.feed.read(-5, 7, 9, 3) == -1).all()              # no window yet: -1 everywhere
    for k in range(2):
        _place(m, ranges[k], poses[k], k)
    live.update(*PARAMS)
    c.poll(what="two scans")
    ox, oy, w, h = window_of(live)
    nav = c.map[0]
    assert np.array_equal(c.feed.read(ox, oy, w, h), nav) and (nav != -1).any()
    # a rectangle hanging over every side: the window in the middle, -1 around it
    big = c.feed.read(ox - 7, oy - 3, w + 12, h + 9)
    assert big.shape == (h + 9, w + 12)
    assert np.array_equal(big[3:3 + h, 7:7 + w], nav)
    outside = np.ones(big.shape, dtype=bool)
    outside[3:3 + h, 7:7 + w] = False
    assert (big[outside] == -1).all()
    # odd rectangles inside, over one corner, and far away
    ys, xs = np.nonzero(nav != -1)
    y, x = int(ys[0]), int(xs[0])
    padded = np.full((h + 32, w + 32), -1, dtype=np.int8)
    padded[16:16 + h, 16:16 + w] = nav
    assert np.array_equal(c.feed.read(ox + x - 1, oy + y - 2, 5, 3), padded[y + 14:y + 17, x + 15:x + 20])
    corner = c.feed.read(ox + w - 2, oy + h - 1, 4, 4)
    assert np.array_equal(corner[:1, :2], nav[h - 1:, w - 2:]) and (corner[1:] == -1).all() and (corner[:, 2:] == -1).all()
    assert (c.feed.read(2 ** 31 - 10, -2 ** 31, 10, 5) == -1).all()
    assert c.feed.read(ox, oy, 0, 5).shape == (5, 0) and c.feed.read(ox, oy, 5, 0).shape == (0, 5)
    c.close(); live.close(); m.close()


def test_errors(kartohip_lib):
    L = kartohip_lib
    laser = synth.Laser()
    m = placing_mapper(laser)
    live = m.live_map(RES, LOW_LEFT, math.inf)
    h = C.c_void_p()
    assert L.kh_map_feed_create(None, C.byref(h)) == capi.KH_ERR_INVALID_ARG and not h.value
    assert L.kh_map_feed_create(live._h, None) == capi.KH_ERR_INVALID_ARG
    feed = live.feed()
    out = np.zeros(16, dtype=np.int8)
    delta = capi.KhMapFeedDelta()
    assert L.kh_map_feed_poll(feed._h, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_poll(None, C.byref(delta)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_tiles(None, None, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_tiles(feed._h, None, None) == capi.KH_OK
    assert L.kh_map_feed_stats(feed._h, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_read(None, 0, 0, 4, 4, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_read(feed._h, 0, 0, -1, 4, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_read(feed._h, 0, 0, 4, -1, out.ctypes.data) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_read(feed._h, 0, 0, 65536, 32768, out.ctypes.data) == capi.KH_ERR_INVALID_ARG      # w * h = 2^31
    assert L.kh_map_feed_read(feed._h, 0, 0, 4, 4, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_map_feed_read(feed._h, 0, 0, 0, 4, None) == capi.KH_OK
    assert L.kh_map_feed_read(feed._h, 0, 0, 4, 4, out.ctypes.data) == capi.KH_OK and (out == -1).all()
    # a feed attached changes nothing of the live map; one destroyed is gone from it
    assert m.Process(np.full(laser.n_beams, 3.0), np.zeros(3), 0.0)[0]
    feed.close()
    live.update(*PARAMS)
    second = live.feed()
    d, xy, data = second.poll()
    assert d["n_tiles"] > 0 and d["tiles_scanned"] == _whole(live)
    second.close(); live.close(); m.close()
