"""CPU: the rule the live map's GPU tests rely on (tests/live_map_rule.py), checked on the oracle alone: the minimum window holds
every counter the oracle sets for seeded synthetic scans, whole blocks only add to it, and the counters of a scan added and then
subtracted leave zero."""
import numpy as np
import pytest

import live_map_rule as rule
from slam_toolbox_amd import synth


def _scans(n, seed, laser):
    from oracle import karto
    world = synth.make_world(12345)
    rng = np.random.default_rng(seed)
    truth, _ = synth.trajectory_laps(40 * n)
    out = []
    for k in range(n):
        pose = truth[(37 * k) % truth.shape[0]].copy()
        pose[:2] += rng.uniform(-0.2, 0.2, size=2)
        out.append(karto.Scan(synth.make_scan(world, pose, rng, laser), pose, laser))
    return out


@pytest.mark.parametrize("resolution,seed", [(0.05, 1), (0.1, 2), (0.037, 3)])
def test_min_window_holds_every_counter(oracle_lib, resolution, seed):
    laser = synth.Laser()
    scans = _scans(6, seed, laser)
    anchor = np.array([-25.0, -25.0])                 # lower left of the 60 m x 40 m world by more than the range threshold
    sensors = np.array([s.sensor_pose[:2] for s in scans])
    win = rule.min_window(sensors, anchor, resolution, laser.range_threshold)
    assert win[0] >= 0 and win[1] >= 0
    cells, p, hits = rule.expected(win, scans, anchor, resolution, laser)      # asserts zero outside the window
    assert p.any() and hits.any() and (cells == 100).any() and (cells == 255).any()
    # the margin is not slack the oracle uses: the outermost ring of the minimum window stays empty
    w, h = win[2], win[3]
    assert not p[0, :w].any() and not p[h - 1, :w].any() and not p[:, 0].any() and not p[:, w - 1].any()
    # the library's window: whole blocks, containing the minimum window
    lib = rule.window(None, sensors, anchor, resolution, laser.range_threshold)
    assert lib[0] % rule.BLOCK == 0 and lib[1] % rule.BLOCK == 0 and lib[2] % rule.BLOCK == 0 and lib[3] % rule.BLOCK == 0
    assert lib[0] <= win[0] and lib[1] <= win[1] and lib[0] + lib[2] >= win[0] + win[2] and lib[1] + lib[3] >= win[1] + win[3]
    grown = rule.window(lib, sensors.max(axis=0).reshape(1, 2) + 30.0, anchor, resolution, laser.range_threshold)
    assert grown[0] == lib[0] and grown[1] == lib[1] and grown[2] > lib[2] and grown[3] > lib[3]
    assert rule.window(grown, sensors, anchor, resolution, laser.range_threshold) == grown, "the window never shrinks"
    rule.expected(lib, scans, anchor, resolution, laser)


def test_add_then_subtract_leaves_zero(oracle_lib):
    """the counters are integer sums over beams: all scans minus (all scans but one) is that one scan, in uint32 arithmetic"""
    laser = synth.Laser()
    scans = _scans(5, 7, laser)
    anchor, res = np.array([-25.0, -25.0]), 0.05
    win = rule.window(None, np.array([s.sensor_pose[:2] for s in scans]), anchor, res, laser.range_threshold)
    _, p_all, h_all = rule.expected(win, scans, anchor, res, laser)
    _, p_rest, h_rest = rule.expected(win, scans[:-1], anchor, res, laser)
    _, p_one, h_one = rule.expected(win, scans[-1:], anchor, res, laser)
    assert np.array_equal(p_all - p_one, p_rest) and np.array_equal(h_all - h_one, h_rest)
    minus_one = np.uint32(0xFFFFFFFF)
    assert not (p_one + p_one * minus_one).any() and not (h_one + h_one * minus_one).any()      # x + x * (2^32 - 1) = 0 mod 2^32


def test_negative_cells_round_away_from_zero():
    c = rule.cells_of([[-0.03125, 0.03125], [-0.09375, 0.09375], [-0.03, 0.03]], (0.0, 0.0), 0.0625)
    assert c.tolist() == [[-1, 1], [-2, 2], [0, 0]]
    assert rule.shift_is_exact([[0.03125, 0.03125], [3.0, -7.5], [-1.03, -2.51]], (0.0, 0.0), (1024, 1024), 0.0625)
    # a tie on the negative side rounds AWAY from zero, the same point seen from a lower-left anchor rounds up: not the same lattice
    assert not rule.shift_is_exact([[-0.03125, 0.03125]], (0.0, 0.0), (1024, 1024), 0.0625)
    assert rule.reach(20.0, 0.05) == 402 and rule.min_window([[0.0, 0.0]], (0.0, 0.0), 0.05, 20.0) == (-402, -402, 805, 805)
    assert rule.window(None, [[0.0, 0.0]], (0.0, 0.0), 0.05, 20.0) == (-448, -448, 896, 896)
