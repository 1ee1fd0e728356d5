"""GPU: edge inputs of the live map's kernels (k_occ_trace_delta, k_occ_update_rect; csrc/occupancy_live.hip) through small mappers
that place their scans where the test says (use_scan_matching 0, as tests/test_occupancy_edges_gpu.py feeds kh_mapper_build_map
through a mapper), compared with tests/live_map_rule.py: dropped and clipped readings, readings on every range gate, an anchor
inside the map (negative cells, rounding ties), beam counts around the 64-beam run, a single scan added / moved / removed, and 300
delta rounds on one live map.

Not tested, on purpose: a KEPT beam whose point reading is not finite -- a mapper cannot make one: its
point readings are the sensor position plus range x direction, and a kept range is finite."""
import math

import numpy as np
import pytest

import live_map_rule as rule
import occupancy_cases as oc
from slam_toolbox_amd import synth
from test_live_map_gpu import assert_equals_rule, oracle_scans_of, window_of
from test_occupancy_edges_gpu import _write_bad_readings

pytestmark = pytest.mark.gpu
LOW_LEFT = np.array([-64.0, -64.0])


def placing_mapper(laser):
    """a mapper that accepts every scan at the pose it is given: no matching, no gate on the distance travelled"""
    from slam_toolbox_amd.mapper import Mapper
    return Mapper(laser, use_scan_matching=0, minimum_travel_distance=0.0, do_loop_closing=0)


def _place(m, ranges, pose, t, exact=True):
    """exact=False: a scan placed behind one that kh_mapper_set_scan_pose moved is carried along by that correction, as
    Mapper::Process does (Mapper.cpp:2699-2703); the rule reads the scans back from the mapper, so any pose will do"""
    ok, got, _ = m.Process(ranges, np.asarray(pose, dtype=np.float64), float(t))
    assert ok
    if exact:
        assert np.array_equal(got, np.asarray(pose, dtype=np.float64)), "the mapper did not put the scan where it was told"


def _keeper(m, pose, t):
    """a scan that traces nothing (every reading under the minimum range): kh_mapper_remove_node refuses the mapper's LAST scan,
    so the scans under test are followed by this one"""
    _place(m, np.full(m.n_beams, 0.05), pose, t)


def _synthetic(n, seed, laser=None):
    laser = laser or synth.Laser()
    world, rng = synth.make_world(12345), np.random.default_rng(seed)
    poses = np.stack([rng.uniform(8.0, 30.0, n), rng.uniform(8.0, 30.0, n), rng.uniform(-3.0, 3.0, n)], axis=1)
    return poses, np.stack([synth.make_scan(world, poses[k], rng, laser) for k in range(n)])


@pytest.mark.parametrize("fraction", [math.inf, 0.0], ids=["delta", "rebuild"])
def test_dropped_and_clipped_readings(kartohip_lib, oracle_lib, fraction):
    laser = synth.Laser()
    poses, ranges = _synthetic(12, 3)
    ranges = _write_bad_readings(ranges, laser)
    m = placing_mapper(laser)
    live = m.live_map(0.05, LOW_LEFT, fraction)
    win = None
    for k in range(12):
        _place(m, ranges[k], poses[k], k)
        if k % 4 == 3:
            live.update()
            win = assert_equals_rule(live, m, laser, win, what=f"{k + 1} scans")
    kept = sum(int(((s.ranges > laser.min_range) & (s.ranges < laser.max_range)).sum()) for s in oracle_scans_of(m))
    total = live.stats()["total"]
    if fraction == math.inf:
        assert total["beams_traced"] == kept < 12 * laser.n_beams
    for k in (1, 6, 7):
        m.RemoveNode(k)
    live.update()
    assert_equals_rule(live, m, laser, win, what="three removed")
    live.close(); m.close()


def test_range_gates(kartohip_lib, oracle_lib):
    """a reading on each range gate and one ulp either side (tests/occupancy_cases.gate_values), each at many beam angles"""
    laser = synth.Laser()
    assert (laser.min_range, laser.range_threshold, laser.max_range) == tuple(oc.GATES)
    vals = oc.gate_values()
    r = np.array([vals[i % len(vals)][1] for i in range(laser.n_beams)])
    m = placing_mapper(laser)
    live = m.live_map(0.0625, LOW_LEFT, math.inf)
    _place(m, r, [3.0, 5.0, 0.3], 0)
    _place(m, np.roll(r, 7), [4.5, 2.0, -2.0], 1)
    live.update()
    win = assert_equals_rule(live, m, laser, None, what="gates")
    kept = sum(v[2] for v in vals[:laser.n_beams % len(vals)]) + (laser.n_beams // len(vals)) * sum(v[2] for v in vals)
    assert live.stats()["total"]["beams_traced"] == 2 * kept
    hits = live.counters()[1]
    assert hits.any()
    m.set_scan_pose(0, [3.0, 5.0, 0.3 + 1e-3])           # every kept beam turns a little: SUB and ADD of the gates through MOVE
    last = live.update()
    assert last["scans_moved"] == 1 and last["scans_added"] == 0 and last["beams_traced"] + 2 * last["beams_skipped"] == 2 * kept
    assert_equals_rule(live, m, laser, win, what="gates, turned")
    _keeper(m, [4.5, 2.0, -2.0], 2)
    m.RemoveNode(0); m.RemoveNode(1)
    last = live.update()
    assert (last["scans_added"], last["scans_removed"]) == (1, 2) and last["beams_traced"] == 2 * kept
    p, hits = live.counters()
    assert not p.any() and not hits.any() and not live.cells().any()
    live.close(); m.close()


def test_anchor_inside_the_map(kartohip_lib, oracle_lib):
    """an anchor in the middle of the scans: cells are negative on one side.  The oracle sees the lattice from an anchor 4096 cells
    further down-left, which is exact here (resolution 2^-4; checked on the very points); beams that end on rounding ties LEFT of
    and BELOW the anchor -- where round-half-away and a shifted anchor disagree -- are checked against rule.trace."""
    res, anchor, shift = 0.0625, np.array([16.0, 16.0]), (4096, 4096)
    laser = synth.Laser()
    poses, ranges = _synthetic(10, 5)
    poses[0, :2] = (16.03125, 15.96875)                   # sensor cells on ties: +0.5 -> 1, -0.5 -> -1
    m = placing_mapper(laser)
    live = m.live_map(res, anchor, math.inf)
    for k in range(10):
        _place(m, ranges[k], poses[k], k)
    live.update()
    scans = oracle_scans_of(m)
    pts = np.concatenate([s.points for s in scans] + [np.array([s.sensor_pose[:2] for s in scans])])
    # (poses[0]'s y is on a negative tie: its cell is fixed by hand below, every other point must shift exactly)
    others = np.concatenate([s.points for s in scans[1:]] + [np.array([s.sensor_pose[:2] for s in scans[1:]])])
    assert rule.shift_is_exact(others, anchor, shift, res)
    c = rule.cells_of(pts[np.isfinite(pts).all(axis=1)], anchor, res)
    assert (c < 0).any() and (c > 0).any()
    info = live.info()
    assert info["ox"] < 0 and info["oy"] < 0
    # scan 0 leaves again: what is left is what the oracle can see, and the tie scan must have left nothing behind
    m.RemoveNode(0)
    live.update()
    win = assert_equals_rule(live, m, laser, rule.window(None, poses[:, :2], anchor, res, laser.range_threshold), shift_cells=shift,
                             what="anchor inside")
    assert win[0] < 0 < win[0] + win[2]
    live.close(); m.close()
    # ties on both sides of the anchor, beam by beam: a laser whose beam 0 points along +x exactly (angle 0 + 0 + 0 * resolution)
    small = synth.Laser(n_beams=3, min_angle=0.0, max_angle=math.pi, ang_res=math.pi / 2)
    m = placing_mapper(small)
    live = m.live_map(res, np.zeros(2), math.inf)
    beams = []
    for k, (sx, sy, r0) in enumerate([(-3.03125, -1.03125, 1.5), (-0.53125, 0.03125, 1.0), (-2.09375, -0.96875, 1.0625), (0.03125, -0.03125, 2.0)]):
        _place(m, np.array([r0, 0.05, 0.05]), [sx, sy, 0.0], k)           # beams 1, 2: under the minimum range, dropped
        beams.append(((sx, sy), (sx + r0, sy), True))
    live.update()
    got = [np.ctypeslib.as_array(m.scan(k)[0].points_xy, (6,))[:2].copy() for k in range(len(beams))]
    assert all(np.array_equal(g, np.array(b[1])) for g, b in zip(got, beams)), "beam 0 does not end where the test computes"
    ties = rule.cells_of(np.array([b[0] for b in beams] + [b[1] for b in beams]), (0.0, 0.0), res)
    assert (ties < 0).any() and (ties > 0).any()
    win = window_of(live)
    assert win == rule.window(None, np.array([b[0] for b in beams]), (0.0, 0.0), res, small.range_threshold)
    p, hits = rule.trace(win, beams, (0.0, 0.0), res)
    gp, gh = live.counters()
    assert np.array_equal(gp, p) and np.array_equal(gh, hits) and p.sum() > 40
    # floor(v + 0.5) instead of round-half-away would put the first sensor in cell (-48, -16) instead of (-49, -17)
    assert gp[-17 - win[1], -49 - win[0]] >= 1 and gp[-16 - win[1], -48 - win[0]] == 0
    live.close(); m.close()


@pytest.mark.parametrize("n_beams", [1, 63, 64, 65, 1081])
def test_beam_counts(kartohip_lib, oracle_lib, n_beams):
    laser = synth.Laser(n_beams=n_beams, min_angle=-0.4, max_angle=-0.4 + 0.0125 * (n_beams - 1), ang_res=0.0125 if n_beams < 1000 else synth.ANG_RES)
    rng = np.random.default_rng(n_beams)
    m = placing_mapper(laser)
    live = m.live_map(0.05, LOW_LEFT, math.inf)
    win = None
    for k in range(5):
        _place(m, rng.uniform(0.5, 25.0, n_beams), [rng.uniform(0, 9), rng.uniform(0, 9), rng.uniform(-3, 3)], k)
        if k in (1, 4):
            live.update()
            win = assert_equals_rule(live, m, laser, win, what=f"{n_beams} beams, {k + 1} scans")
    assert live.stats()["total"]["beams_traced"] == 5 * n_beams
    m.set_scan_pose(2, [4.0, 4.0, 1.0])
    m.RemoveNode(0)
    last = live.update()
    assert (last["scans_moved"], last["scans_removed"]) == (1, 1)
    assert_equals_rule(live, m, laser, win, what=f"{n_beams} beams, moved and removed")
    live.close(); m.close()


def test_single_scan_added_moved_removed(kartohip_lib, oracle_lib):
    laser = synth.Laser()
    res = 0.0625
    poses, ranges = _synthetic(1, 11)
    pose = np.array([10.0, 12.0, 0.25])                  # cell centres exactly (anchor and resolution are dyadic)
    m = placing_mapper(laser)
    live = m.live_map(res, LOW_LEFT, math.inf)
    _place(m, ranges[0], pose, 0)
    _keeper(m, pose, 1)                                  # (traces nothing; lets scan 0 be removed at the end)
    last = live.update()
    kept = last["beams_traced"]
    assert last["scans_added"] == 2 and 0 < kept <= laser.n_beams
    win = assert_equals_rule(live, m, laser, None, what="added")
    # exactly one cell: every line moves with the sensor cell
    m.set_scan_pose(0, pose + np.array([res, 0.0, 0.0]))
    last = live.update()
    assert (last["scans_added"], last["scans_moved"], last["scans_removed"]) == (0, 1, 0)
    assert last["beams_skipped"] == 0 and last["beams_traced"] == 2 * kept and last["rebuilds"] == 0
    assert 0 < last["cells_updated"] < live.info()["width_step"] * live.info()["height"]
    win = assert_equals_rule(live, m, laser, win, what="moved by one cell")
    # less than a cell: the sensor cell stays, most end cells stay, some cross a cell border
    m.set_scan_pose(0, pose + np.array([res + res / 16, 0.0, 0.0]))
    last = live.update()
    assert last["scans_moved"] == 1 and 0 < last["beams_skipped"] < kept
    assert last["beams_traced"] == 2 * (kept - last["beams_skipped"])
    win = assert_equals_rule(live, m, laser, win, what="moved by a sixteenth of a cell")
    # the same pose again: nothing to do
    m.set_scan_pose(0, pose + np.array([res + res / 16, 0.0, 0.0]))
    last = live.update()
    assert last["scans_moved"] == 0 and last["beams_traced"] == 0 and last["cells_updated"] == 0
    m.RemoveNode(0)
    last = live.update()
    assert last["scans_removed"] == 1 and last["beams_traced"] == kept
    p, hits = live.counters()
    assert not p.any() and not hits.any() and not live.cells().any()
    assert window_of(live) == win
    live.close(); m.close()


def test_many_delta_rounds(kartohip_lib, oracle_lib):
    """300 rounds of seeded adds, moves and removals on one live map: log slots are reused, the log and the delta table regrow;
    compared with the rule every 60 rounds and at the end"""
    laser = synth.Laser(n_beams=181, min_angle=-1.5, max_angle=1.5, ang_res=3.0 / 180)
    rng = np.random.default_rng(2024)
    m = placing_mapper(laser)
    live = m.live_map(0.1, LOW_LEFT, math.inf)
    win, t, peak = None, 0, 0
    for rnd in range(300):
        burst = 90 if rnd == 150 else int(rng.integers(0, 4))          # one big round: the log outgrows its first allocation
        for _ in range(burst):
            _place(m, rng.uniform(0.05, 28.0, laser.n_beams), [rng.uniform(0, 20), rng.uniform(0, 20), rng.uniform(-3, 3)], t, exact=False)
            t += 1
        alive = m.alive()
        movers = rng.choice(alive, size=min(len(alive), int(rng.integers(0, 3))), replace=False) if len(alive) else []
        for k in movers:
            p = m.poses()[int(k)] + np.array([rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.002)])
            m.set_scan_pose(int(k), p)
        alive = m.alive()
        alive = alive[alive != m.num_scans() - 1]                      # (the mapper keeps its last scan)
        n_gone = min(len(alive), int(rng.integers(0, 3)) if rnd != 200 else 70)
        for k in rng.choice(alive, size=n_gone, replace=False) if n_gone else []:
            m.RemoveNode(int(k))
        last = live.update()
        assert last["rebuilds"] == 0
        peak = max(peak, live.stats()["scans_in_map"])
        # the window remembers scans that have left: the rule is followed round by round (sensor = robot position for this laser)
        win = rule.window(win, m.poses()[m.alive()][:, :2], LOW_LEFT, 0.1, laser.range_threshold)
        assert window_of(live) == (win or (0, 0, 0, 0)), f"round {rnd}"
        if rnd % 60 == 59 or rnd == 299:
            win = assert_equals_rule(live, m, laser, win, what=f"round {rnd}")
    st = live.stats()
    # (a scan placed and removed inside one round never reaches the live map)
    assert st["scans_in_map"] == len(m.alive()) and 400 < st["total"]["scans_added"] <= m.num_scans()
    assert st["total"]["scans_added"] - st["total"]["scans_removed"] == st["scans_in_map"]
    assert st["total"]["scans_removed"] > 200 and st["total"]["scans_moved"] > 100 and st["total"]["beams_skipped"] > 0
    # slots were reused: the log never held more slots than 1.5 x the peak number of scans plus its first allocation
    assert st["log_bytes"] <= (max(64, peak + peak // 2) + peak) * 4 * (2 + 2 * laser.n_beams) and peak > 90
    live.close(); m.close()
