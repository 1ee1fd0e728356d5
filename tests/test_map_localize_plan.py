"""The host rules of the map localizer (slam_toolbox_amd/csrc/map_localize_plan.hpp) on the CPU, through the stand-alone program
tests/map_localize_plan_check.cpp: the pitch, block ranges for negative origins, compaction and region, ranking and suppression
chains, the walk-length guard and the odometric prediction.  Expectations come from tests/map_localize_rule.py and plain Python.
No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import map_localize_rule as rule
import map_match_rule as mr
from common import bits

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_localize_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_localize_plan_check.cpp"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout
        return out
    return run


def hx(v):
    return float(v).hex()


def test_pitch(check):
    cases = [(1.0, 20.0), (1.05, 20.0), (1.5, 20.0), (2.0, 20.0), (0.05, 20.0), (0.01, 20.0), (0.074, 20.0), (0.075, 20.0), (0.125, 20.0),
             (204.8, 20.0), (204.76, 20.0), (204.7, 20.0), (1e9, 20.0), (0.0, 20.0), (-1.0, 20.0), (math.inf, 20.0), (math.nan, 20.0)]
    got = [int(v) for v in check([f"pitch {hx(s)} {hx(k)}" for s, k in cases])]
    want = []
    for s, k in cases:
        try:
            want.append(rule.pitch_of(s, k))
        except ValueError:
            want.append(0)
    assert got == want
    assert want[:5] == [21, 21, 31, 41, 1] and want[9] == 0 and want[11] == 4095 and want[12:] == [0] * 5
    assert all(p % 2 == 1 for p in want if p), "the pitch is forced odd"


def test_block_ranges_for_negative_origins(check):
    cases = [(ox, oy, w, h, p) for p in (1, 3, 21, 31) for ox in (-65, -31, -1, 0, 1, 30, 31) for oy in (-62, 0, 5) for (w, h) in ((1, 1), (31, 62), (64, 3))]
    got = check(["blocks %d %d %d %d %d" % c for c in cases])
    for (ox, oy, w, h, p), line in zip(cases, got):
        bx0, by0 = ox // p, oy // p                          # Python's floor quotient
        want = (bx0, by0, (ox + w - 1) // p - bx0 + 1, (oy + h - 1) // p - by0 + 1)
        assert tuple(int(v) for v in line.split()) == want, (ox, oy, w, h, p)


def _local_of(view, spacing):
    """k_map_seeds' answer for the view, from the rule's seeds: per block, row-major, the local index of its seed or -1"""
    p = rule.pitch_of(spacing, view["scale"])
    ox, oy, w, h = view["ox"], view["oy"], view["width"], view["height"]
    bx0, by0 = ox // p, oy // p
    nx, ny = (ox + w - 1) // p - bx0 + 1, (oy + h - 1) // p - by0 + 1
    local = -np.ones((ny, nx), dtype=np.int64)
    cells, _ = rule.seeds(view, spacing)
    for i, j in cells:
        local[j // p - by0, i // p - bx0] = (j % p) * p + (i % p)
    return p, local


@pytest.mark.parametrize("origin", [(0, 0), (-40, -25), (17, -3)])
def test_compaction_and_region(check, origin):
    rng = np.random.default_rng(3)
    cells = rng.choice(np.array([0, 100, 255], dtype=np.uint8), size=(50, 72), p=[0.6, 0.2, 0.2])
    cells[20:40, 10:45] = 100                                # blocks without a free cell
    cells[:, 70:] = 255                                      # beyond `width`: not cells
    view = mr.view_dict(cells, (0.51, -0.27), 1.0 / 0.04, origin[0], origin[1], 70)
    spacing = 0.3                                            # 7.5 cells -> 8 -> pitch 9
    p, local = _local_of(view, spacing)
    assert p == 9 and (local < 0).any() and (local >= 0).sum() > 20
    all_cells, all_xy = rule.seeds(view, spacing)
    center = tuple(all_xy[len(all_xy) // 2] + np.array([0.07, -0.05]))
    for region, radius in ((0, 0.0), (1, 0.9), (1, 0.0), (1, 1e-3)):
        line = (f"compact {origin[0]} {origin[1]} 70 50 {p} {hx(view['anchor'][0])} {hx(view['anchor'][1])} {hx(view['scale'])} {region} "
                f"{hx(center[0])} {hx(center[1])} {hx(radius)} {local.size} " + " ".join(str(int(v)) for v in local.ravel()))
        got = check([line])[0]
        want_cells, want_xy = rule.seeds(view, spacing, center if region else None, radius)
        if radius == 0.9:
            assert 0 < len(want_cells) < len(all_cells)
        if got == "none":
            assert len(want_cells) == 0
            continue
        t = got.split()
        got_cells = np.array([[int(t[4 * k]), int(t[4 * k + 1])] for k in range(len(t) // 4)])
        got_xy = np.array([[float.fromhex(t[4 * k + 2]), float.fromhex(t[4 * k + 3])] for k in range(len(t) // 4)])
        assert np.array_equal(got_cells, want_cells) and np.array_equal(bits(got_xy), bits(want_xy))


H = dict(fine=0.8, coarse=0.6, x=1.0, y=2.0, h=0.1, known=1000, score=0.99)


def _answer(check, hyps, min_fit=0.0, merge_d=0.05, merge_h=0.0349):
    rows = [dict(H, index=k, **h) for k, h in enumerate(hyps)]
    line = f"answer {hx(min_fit)} {hx(merge_d)} {hx(merge_h)} {len(rows)} " + " ".join(
        f"{r['index']} {hx(r['fine'])} {hx(r['coarse'])} {hx(r['x'])} {hx(r['y'])} {hx(r['h'])} {r['known']} {hx(r['score'])}" for r in rows)
    order, kept, counts = (part.split() for part in check([line])[0].split("|"))
    # the same through the rule
    Hyp = rule.Hyp
    rh = [Hyp(r["index"], (0, 0), 0.0, None, None, r["coarse"], True, np.array([r["x"], r["y"], r["h"]]), None, r["fine"], True) for r in rows]
    want_order = rule.rank(rh)
    fits = {k: dict(known=rows[k]["known"], score=rows[k]["score"]) for k in want_order}
    want_kept, want_rej, want_dup = rule.suppress(want_order, {k: rh[k].fine_mean for k in want_order}, fits, min_fit, merge_d, merge_h)
    assert [int(v) for v in order] == want_order and [int(v) for v in kept] == want_kept
    assert [int(v) for v in counts] == [len(want_rej), len(want_dup)]
    return [int(v) for v in order], [int(v) for v in kept], [int(v) for v in counts]


def test_ranking(check):
    order, kept, _ = _answer(check, [dict(fine=0.5), dict(fine=0.9, coarse=0.1), dict(fine=0.9, coarse=0.7), dict(fine=0.9, coarse=0.7),
                                     dict(fine=0.7)], merge_d=0.0)
    assert order == [2, 3, 1, 4, 0] and kept == order, "fine desc, coarse desc, index asc; merge_distance 0: nothing suppressed"


def test_suppression_is_greedy(check):
    """A suppresses B, and B would have suppressed C: C survives, because only KEPT hypotheses suppress"""
    a, b, c = dict(fine=0.9, x=1.00), dict(fine=0.8, x=1.04), dict(fine=0.7, x=1.08)
    order, kept, counts = _answer(check, [a, b, c])
    assert order == [0, 1, 2] and kept == [0, 2] and counts == [0, 1]
    # ... in rank order, not index order: the same three with the responses reversed keep the other end
    order, kept, counts = _answer(check, [dict(a, fine=0.7), b, dict(c, fine=0.9)])
    assert order == [2, 1, 0] and kept == [2, 0] and counts == [0, 1]
    # a chain of five 0.04 apart: every other one
    chain = [dict(fine=0.9 - 0.01 * k, y=2.0 + 0.04 * k) for k in range(5)]
    assert _answer(check, chain)[1] == [0, 2, 4]


def test_suppression_edges(check):
    d = 0.05
    inside = math.nextafter(math.sqrt(d * d), 0.0)
    while (inside * inside) >= d * d:
        inside = math.nextafter(inside, 0.0)
    outside = inside
    while (outside * outside) < d * d:
        outside = math.nextafter(outside, math.inf)
    first = dict(fine=0.9, x=0.0, y=0.0)
    assert _answer(check, [first, dict(fine=0.8, x=inside, y=0.0)], merge_d=d)[1] == [0]
    assert _answer(check, [first, dict(fine=0.8, x=outside, y=0.0)], merge_d=d)[1] == [0, 1]
    # the heading: a different heading at the same place is another hypothesis; across the +-pi seam it is the same
    assert _answer(check, [first, dict(fine=0.8, x=0.0, y=0.0, h=0.1 + 0.0349)], merge_d=d)[1] == [0, 1]
    assert _answer(check, [dict(first, h=math.pi - 0.01), dict(fine=0.8, x=0.0, y=0.0, h=-math.pi + 0.01)], merge_d=d)[1] == [0]
    assert _answer(check, [first, dict(fine=0.8, x=0.0, y=0.0)], merge_d=-1.0)[1] == [0, 1], "merge_distance <= 0: no suppression"
    # the fit gate: known > 0 and score < min_fit_score; a hypothesis dropped by it suppresses nothing
    poor = dict(fine=0.95, x=0.0, y=0.0, score=0.5)
    order, kept, counts = _answer(check, [poor, dict(fine=0.8, x=0.01, y=0.0)], min_fit=0.9, merge_d=d)
    assert order == [0, 1] and kept == [1] and counts == [1, 0]
    assert _answer(check, [dict(poor, known=0, score=0.0)], min_fit=0.9)[1] == [0], "nothing known: not rejected"
    assert _answer(check, [dict(poor, score=0.9)], min_fit=0.9)[1] == [0], "score == min_fit_score stays"


POSES = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 2.0, 0.3)),               # identical poses: the identity
         ((1.0, 2.0, 0.3), (1.0, 2.0, 0.3), (4.0, -1.0, 2.0)),
         ((0.0, 0.0, 0.2), (0.5, -0.25, 0.31), (0.7, 0.1, 0.25)),           # a first pose at the origin: the translation is pose 2's
         ((2.5, 3.0, 1.5707963267948966), (2.53, 2.96, 1.6), (2.5, 3.6, 1.58)),
         ((-7.25, 11.5, -3.0), (-7.0, 11.0, 3.1), (-6.9, 12.0, -3.1)),       # across the seam: the heading is normalised
         ((10.0, -4.0, 0.11462314399891493), (10.2, -4.1, 0.0), (11.0, -3.0, 0.2))]


def test_prediction(check):
    got = check(["predict " + " ".join(hx(v) for p in case for v in p) for case in POSES])
    for case, line in zip(POSES, got):
        want = rule.transform_pose(*case)
        assert np.array_equal(bits([float.fromhex(t) for t in line.split()]), bits(want)), case
    assert np.array_equal(rule.transform_pose(*POSES[0]), POSES[0][2])
    assert abs(rule.transform_pose(*POSES[4])[2]) <= math.pi


def test_prediction_is_the_reference_transform():
    """where the reference build exists: the numpy restatement against karto::Transform itself"""
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    import ctypes as C
    fn = ref.lib().ref_transform_pose
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 4
    for case in POSES:
        a, b, c = (np.array(p, dtype=np.float64) for p in case)
        out = np.zeros(3)
        fn(a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data)
        assert np.array_equal(bits(out), bits(rule.transform_pose(a, b, c))), case


def test_walk_length_guard(check):
    scale = 20.0
    cases = [((12.0, 0.1, 30.0, scale, 0.0, 0.0, 1.0, 2.0, 0.3), (1, 1)),
             (((2 ** 20 - 2) / scale, 0.1, 30.0, scale, 0.0, 0.0, 1.0, 2.0, 0.3), (1, 1)),            # exactly 2^20 cells with the slack of two
             (((2 ** 20 - 1) / scale, 0.1, 30.0, scale, 0.0, 0.0, 1.0, 2.0, 0.3), (0, 1)),
             ((math.inf, 0.1, 30.0, scale, 0.0, 0.0, 1.0, 2.0, 0.3), (0, 1)),
             ((12.0, math.nan, 30.0, scale, 0.0, 0.0, 1.0, 2.0, 0.3), (0, 1)),
             ((12.0, 0.1, math.nan, scale, 0.0, 0.0, 1.0, 2.0, 0.3), (0, 1)),
             ((12.0, 0.1, math.inf, scale, 0.0, 0.0, 2.0 ** 30 / scale, 2.0, 0.3), (1, 1)),           # a sensor cell of 2^30
             ((12.0, 0.1, 30.0, scale, 0.0, 0.0, 2.0 ** 30 / scale + 1.0, 2.0, 0.3), (1, 0)),
             ((12.0, 0.1, 30.0, scale, 0.0, 0.0, 1.0, -1e12, 0.3), (1, 0)),
             ((12.0, 0.1, 30.0, scale, 0.0, 0.0, math.nan, 2.0, 0.3), (1, 0)),
             ((12.0, 0.1, 30.0, scale, 0.0, 0.0, 1.0, 2.0, math.inf), (1, 0))]
    got = check(["fitok " + " ".join(hx(v) for v in c) for c, _ in cases])
    assert [tuple(int(v) for v in g.split()) for g in got] == [w for _, w in cases]
    # ... and the rule's own statement of the refusal agrees
    from collections import namedtuple
    L = namedtuple("L", "range_threshold min_range max_range")
    for (rt, lo, hi, k, ax, ay, x, y, h), (laser_ok, pose_ok) in cases:
        if math.isnan(lo) or math.isnan(hi):
            continue
        assert rule.fit_refused(dict(scale=k, anchor=(ax, ay)), L(rt, lo, hi), (x, y, h)) == (not (laser_ok and pose_ok))


def test_laser_and_pose_check(check):
    """fit_inputs_check and fit_inputs_text: which input a call that walks beams on a view refuses, and in which words."""
    scale = 20.0
    good, far = (1.0, 2.0, 0.3), (2.0 ** 30 / scale + 1.0, 2.0, 0.3)
    laser = (12.0, 0.1, 30.0, -1.5, 0.01)
    laser_words = "who: the laser's range_threshold * scale must stay below 2^20 cells, its other fields must be numbers"
    pose_words = "who: pose %d is not finite or lies more than 2^30 cells from the anchor"
    cases = [(((2 ** 20 - 1) / scale, 0.1, 30.0, -1.5, 0.01), [good, good], (1, -1, laser_words)),       # a bad laser: the walk
             ((12.0, 0.1, 30.0, math.nan, 0.01), [good], (1, -1, laser_words)),                          # ... an angle that is no number
             ((12.0, 0.1, 30.0, -1.5, math.inf), [far], (1, -1, laser_words)),                           # ... and the laser is judged first
             (laser, [good, (1.0, math.nan, 0.3), far], (2, 1, pose_words % 1)),                         # a non-finite pose
             (laser, [good, good, (1.0, 2.0, math.inf)], (2, 2, pose_words % 2)),
             (laser, [far, good, good], (2, 0, pose_words % 0)),                                         # beyond 2^30 cells at index 0
             (laser, [good, good, far], (2, 2, pose_words % 2)),                                         # ... and at the last index
             (laser, [good] * 11 + [far], (2, 11, pose_words % 11)),                                     # (an index of two digits)
             (laser, [good, (2.0 ** 30 / scale, -2.0 ** 30 / scale, -3.0)], (0, -1, "")),                # a good input: cells of +-2^30
             (laser, [], (0, -1, ""))]
    lines = []
    for l, poses, _ in cases:
        lines.append("inputs " + " ".join(hx(v) for v in l) + f" {hx(scale)} {hx(0.0)} {hx(0.0)} {len(poses)} " + " ".join(hx(v) for p in poses for v in p))
    got = check(lines)
    for g, (_, _, (failed, pose, text)) in zip(got, cases):
        head, _, words = g.partition(" | ")
        assert tuple(int(v) for v in head.split()) == (failed, pose), g
        assert words.strip() == text, g


def _merge_fit(check, laser, resolution, offset, sensors, n_scans=1):
    """one `mergefit` line -> (failed, candidate, words); sensors: (n_candidates * n_scans, 2), candidate-major"""
    sensors = np.asarray(sensors, dtype=np.float64).reshape(-1, 2)
    n_candidates = len(sensors) // n_scans if n_scans else len(sensors)
    line = (f"mergefit {hx(laser[0])} {hx(laser[1])} {hx(laser[2])} {hx(1.0 / resolution)} {hx(offset[0])} {hx(offset[1])} {n_candidates} {n_scans} "
            + " ".join(hx(v) for v in (sensors.ravel() if n_scans else [])))
    head, _, words = check([line])[0].partition(" | ")
    failed, candidate = (int(v) for v in head.split())
    return failed, candidate, words.strip()


def test_merge_fit_guard(check):
    """merge_fit_check: what kh_merge_fit and kh_merge_align refuse before k_occ_fit_merged is launched, next to
    tests/merge_fit_rule.py's fit_refused.  One scan at the origin under a pure translation has its sensor at the translation itself,
    bit for bit, which is how the rule is fed here."""
    import merge_fit_rule as fr
    from collections import namedtuple
    L = namedtuple("L", "range_threshold min_range max_range")
    origin = {"corrected": np.zeros(3)}
    laser_words = ("kh_merge_fit: the moving submap's range_threshold * scale must stay below 2^20 cells, its minimum and maximum range "
                   "must be numbers")
    pose_words = "kh_merge_fit: correction %d puts a scan's sensor more than 2^30 cells from the offset of the reference grid"
    ok = (5.0, 0.1, 7.5)

    def both(laser, resolution, offset, candidates):
        """the program and the rule on one scan at the origin"""
        got = _merge_fit(check, laser, resolution, offset, [c[:2] for c in candidates])
        want = fr.fit_refused({"laser": L(*laser), "scans": [origin]}, [(c[0], c[1], 0.0) for c in candidates], {"offset": offset}, resolution)
        assert (got[0], got[1]) == {None: (0, -1)}.get(want, (1 if want and want[0] == "laser" else 2, want[1] if want else -1)), (got, want)
        return got

    # the example of the defect: scale 20, offset -3.2, a sensor at x = 6.5 under tx = 107374170
    res, off = 0.05, (-3.2, -3.2)
    x = 6.5 + 107374170.0
    cell = math.floor((x - off[0]) * (1.0 / res) + 0.5)
    end = ((x + 5.0) - off[0]) * (1.0 / res)
    assert cell == 2147483594 and end >= 2147483648.0, "the sensor is an int32 cell, the end of a 5 m beam is past the last one"
    assert both(ok, res, off, [(1.0, 2.0), (x, 0.0)]) == (2, 1, pose_words % 1)
    # the bound itself, on both axes and both sides: exactly 2^30 cells is accepted, a metre outward is not (0.25 m cells, offset 0.5)
    res, off = 0.25, (0.5, -1.5)
    far = 2.0 ** 30 * res
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            at = [1.0, 2.0]
            at[axis] = off[axis] + sign * far
            assert (at[axis] - off[axis]) * 4.0 == sign * 2.0 ** 30
            assert both(ok, res, off, [tuple(at)]) == (0, -1, "")
            at[axis] = off[axis] + sign * (far + 1.0)
            assert both(ok, res, off, [(1.0, 2.0), (0.0, 0.0), tuple(at)]) == (2, 2, pose_words % 2)
    # the neighbours of the int32 ends, NaN and the infinities: all refused, the first bad candidate is named
    for c in (2.0 ** 31 - 1.0, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 - 1.0, 2.0 ** 31 + 1.0, 1e300):
        assert both(ok, 1.0, (0.0, 0.0), [(c, 0.0)])[:2] == (2, 0)
        assert both(ok, 1.0, (0.0, 0.0), [(0.0, 0.0), (0.0, c), (c, c)])[:2] == (2, 1)
    for c in (math.nan, math.inf, -math.inf):
        assert _merge_fit(check, ok, 1.0, (0.0, 0.0), [(0.0, 0.0), (c, 0.0)])[:2] == (2, 1)
        assert _merge_fit(check, ok, 1.0, (0.0, 0.0), [(0.0, c)])[:2] == (2, 0)
    assert both(ok, 0.25, (-10.0, -8.0), [(1000.0, 1000.0), (0.0, 0.0)]) == (0, -1, ""), "far outside the grid is no reason"
    # several scans per candidate: a candidate is refused for any one of its scans, and the index is the candidate's
    near, bad = (1.0, 2.0), (2.0 ** 31, 0.0)
    assert _merge_fit(check, ok, 1.0, (0.0, 0.0), [near, near, near, near, near, bad, near, near, near], n_scans=3)[:2] == (2, 1)
    assert _merge_fit(check, ok, 1.0, (0.0, 0.0), [near, near, near, near, near, near, bad, near, near], n_scans=3)[:2] == (2, 2)
    assert _merge_fit(check, ok, 1.0, (0.0, 0.0), [near] * 9, n_scans=3) == (0, -1, "")
    assert _merge_fit(check, ok, 1.0, (0.0, 0.0), [], n_scans=0) == (0, -1, ""), "a submap without scans"
    # the laser: range_threshold * scale + 2 <= 2^20, judged before any position
    res = 0.25
    assert both(((2 ** 20 - 2) * res, 0.1, math.inf), res, (0.0, 0.0), [near]) == (0, -1, "")
    assert both(((2 ** 20 - 1) * res, 0.1, 30.0), res, (0.0, 0.0), [near]) == (1, -1, laser_words)
    assert both((20.0, 0.1, 30.0), 1e-5, (0.0, 0.0), [near, bad]) == (1, -1, laser_words)
    for rt in (math.inf, math.nan, 0.0, -1.0):
        assert both((rt, 0.1, 30.0), res, (0.0, 0.0), [near]) == (1, -1, laser_words)
    assert both((5.0, math.nan, 30.0), res, (0.0, 0.0), [near]) == (1, -1, laser_words)
    assert both((5.0, 0.1, math.nan), res, (0.0, 0.0), [near]) == (1, -1, laser_words)
