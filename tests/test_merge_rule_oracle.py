"""CPU: the arithmetic of a session merge (tests/merge_rule.py) pinned on its own -- the GPU tests
(tests/test_merge_gpu.py) then pin the library to this rule bit for bit."""
import math

import numpy as np

import merge_rule as rule
from common import bits
from slam_toolbox_amd import synth

RES = 0.05


def _laser(n_beams=120):
    return synth.Laser(n_beams=n_beams, ang_res=(synth.MAX_ANGLE - synth.MIN_ANGLE) / (n_beams - 1))


def _scan(ranges, pose, laser):
    """one scan of a submap the way LocalizedRangeScan::Update leaves it (laser at the robot's centre)"""
    pose = np.asarray(pose, dtype=np.float64)
    points = synth.scan_points(ranges, pose, laser)
    in_range = (ranges >= laser.min_range) & (ranges <= laser.range_threshold)
    xs = np.concatenate([[pose[0]], points[in_range, 0]])
    ys = np.concatenate([[pose[1]], points[in_range, 1]])
    bary = points[in_range].mean(axis=0) if in_range.any() else pose[:2]
    return {"ranges": np.ascontiguousarray(ranges), "points": points, "corrected": pose.copy(), "odometric": pose + np.array([0.01, -0.02, 0.003]),
            "barycenter": np.array([bary[0], bary[1], 0.0 if in_range.any() else pose[2]]), "box": np.array([xs.min(), ys.min(), xs.max(), ys.max()])}


def _lattice_submap(n_scans=8, n_beams=120):
    """scans of the synth world whose sensor positions sit on the 0.05 m lattice, a quarter cell off the cell centres"""
    world, laser, rng = synth.make_world(12345), _laser(n_beams), np.random.default_rng(21)
    scans = []
    for k in range(n_scans):
        pose = np.array([RES * (130 + 160 * (k % 4)) + RES / 4, RES * (100 + 80 * k) + RES / 4, 0.3 + 0.7 * k])       # aisle centre lines
        assert not synth.inside_obstacle(world, pose[0], pose[1], margin=0.2)
        scans.append(_scan(synth.make_scan(world, pose, rng, laser), pose, laser))
    return {"laser": laser, "scans": scans}


def test_identity_returns_the_input_bits():
    sm = _lattice_submap(3)
    for s in sm["scans"]:
        finite = np.isfinite(s["points"]).all(axis=1)
        assert finite.sum() > 100
        got = rule.transform_points(rule.IDENTITY, s["points"])
        assert np.array_equal(bits(got[finite]), bits(s["points"][finite]))
        for key in ("corrected", "odometric", "barycenter"):
            assert np.array_equal(bits(rule.transform_pose(rule.IDENTITY, s[key])), bits(s[key]))
        assert np.array_equal(bits(rule.loose_box(rule.IDENTITY, s["box"])), bits(s["box"]))
        assert np.array_equal(bits(rule.sensor_at(s["corrected"])[:2]), bits(s["corrected"][:2]))
    t = (3.0, -2.0, 0.7)
    assert np.array_equal(bits(rule.compose(rule.IDENTITY, t)), bits(np.array(t)))
    assert np.array_equal(bits(rule.compose(t, rule.IDENTITY)), bits(np.array(t)))


def _matrix(t):
    c, s = math.cos(t[2]), math.sin(t[2])
    return np.array([[c, -s, t[0]], [s, c, t[1]], [0.0, 0.0, 1.0]])


def _of_matrix(m):
    return np.array([m[0, 2], m[1, 2], math.atan2(m[1, 0], m[0, 0])])


def _close(a, b, tol=1e-12):
    d = np.asarray(a) - np.asarray(b)
    d[2] = (d[2] + math.pi) % (2 * math.pi) - math.pi
    return np.abs(d).max() <= tol


def test_compose_and_inverse_agree_with_homogeneous_matrices():
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3.1, 3.1)])
        b = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3.1, 3.1)])
        assert _close(rule.compose(a, b), _of_matrix(_matrix(a) @ _matrix(b)))
        assert _close(rule.inverse(a), _of_matrix(np.linalg.inv(_matrix(a))))
        assert _close(rule.compose(rule.inverse(a), a), np.zeros(3)) and _close(rule.compose(a, rule.inverse(a)), np.zeros(3))
        p = rng.uniform(-30, 30, size=2)
        assert np.abs(np.array(rule.transform_point(a, *p)) - (_matrix(a) @ np.array([p[0], p[1], 1.0]))[:2]).max() <= 1e-12


def test_release_from_the_identity_by_a_pure_translation_is_the_displacement():
    location = rule.initial_location(_lattice_submap(3), RES)
    marker = np.array([location[0] + 3.25, location[1] - 1.5, 0.0])
    correction, new_location = rule.release(rule.IDENTITY, location, marker)
    assert np.array_equal(bits(correction), bits(np.array([marker[0] - location[0], marker[1] - location[1], 0.0])))
    assert np.array_equal(bits(new_location), bits(marker))
    # a second release at the same place with a yaw: the translations cancel and the yaw composes on the right, so the submap
    # turns about the origin of its own frame, as in the reference (correction * inverse(previous) * new location)
    correction2, location2 = rule.release(correction, new_location, np.array([marker[0], marker[1], 0.4]))
    assert _close(correction2, [correction[0], correction[1], 0.4]) and location2[2] == 0.4


def test_transformed_points_lie_inside_the_loose_box():
    """The in-range readings and the sensor position lie inside the scan's own box, a rigid motion keeps them inside the moved
    rectangle, and the loose box contains that rectangle.  Slack 1e-12 m: four products of magnitude <= 100 m round by 1.4e-14 each."""
    sm = _lattice_submap(6)
    for t in ((3.0, -2.0, 0.7), (-10.0, 4.0, -2.9), (0.0, 0.0, math.pi / 2)):
        for s in sm["scans"]:
            ts = rule.transformed_scan(t, s)
            keep = (s["ranges"] >= sm["laser"].min_range) & (s["ranges"] <= sm["laser"].range_threshold)
            pts = np.vstack([ts["points"][keep], ts["sensor"][None, :2]])
            assert keep.sum() > 50
            assert (pts[:, 0] >= ts["box"][0] - 1e-12).all() and (pts[:, 0] <= ts["box"][2] + 1e-12).all()
            assert (pts[:, 1] >= ts["box"][1] - 1e-12).all() and (pts[:, 1] <= ts["box"][3] + 1e-12).all()


def test_quarter_turn_transposes_and_flips_the_counters():
    """A submap turned by pi / 2 about the origin, traced on the grid that is the unturned grid turned with it: cell (gx, gy) of the
    unturned trace is cell (H - 1 - gy, gx) of the turned one.  The sensor positions are a quarter cell off the cell centres, so
    cos(pi / 2) = 6e-17 moves no rounding of theirs; a reading's end point is within 8e-14 cells of a rounding boundary with
    probability 1e-13: the hit counters, which involve no walk, must agree (asserted on 99.9 % of the hit cells).  What does
    differ is Grid::TraceLine (Karto.h:4874-4927) itself: it walks a line from its low end on the major axis, the quarter turn
    reverses that direction for the lines that were steep, and where the line passes exactly between two cells
    (2 k dy = (2 m + 1) dx) the walk from the other end takes the other cell -- the same number of cells, so the sums agree.
    Measured while writing the test: 86 to 298 such cells per scan of 120 beams (about two per line), no hit cell.  Four scans
    keep that below the 0.1 % of the grid's cells allowed (8 scans: 1816 of 1126400 cells, 0.16 %, would not)."""
    sm = _lattice_submap(4, 120)
    W, H, ox, oy = 1280, 880, -2.0, -2.0
    up, uh = rule.submap_counters(sm, rule.IDENTITY, W, H, (ox, oy), RES)
    tp, th = rule.submap_counters(sm, (0.0, 0.0, math.pi / 2), H, W, (-(oy + H * RES) + RES, ox), RES)
    assert up.shape == (H, W) and tp.shape == (W, H) and int(uh.sum()) > 300
    want_p, want_h = up.T[:, ::-1], uh.T[:, ::-1]
    differ_p, differ_h = int((tp != want_p).sum()), int((th != want_h).sum())
    print(f"quarter turn: {int((up > 0).sum())} cells passed, {int((uh > 0).sum())} hit; pass counters differ in {differ_p} cells "
          f"({100.0 * differ_p / up.size:.4f} %), hit counters in {differ_h}")
    assert differ_p <= 0.001 * up.size and int(tp.sum()) == int(up.sum())
    assert differ_h <= 0.001 * int((uh > 0).sum())
