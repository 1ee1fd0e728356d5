"""Edge inputs of the session merger's two kernels (k_occ_trace_merged, k_occ_fit_merged in csrc/occupancy.hip, driven by
csrc/merge.cpp) as plain data: hand-made submaps -- a laser and a list of (sensor pose, ranges) -- their corrections, the update rule
and, for a fit, the candidates.  tests/test_merge_cases_oracle.py checks on the CPU that every case sits on the edge its name says
(Case.check, fed with the answer of tests/merge_rule.py and tests/merge_fit_rule.py alone); tests/test_merge_edges_gpu.py feeds the
same submaps through mappers into a MapMerger and compares exactly.  It reads nothing of the library.

The resolution is 0.25 m, a power of two, and the poses lie on multiples of an eighth of a metre where a case needs an exact
rounding tie.  Exact points exist along the sensor's heading only where cos and sin are exact: a one-beam laser (`ray`) at heading 0
has its point at (x + r, y) bit for bit, and a correction of yaw 0 adds its translation to it in one rounding.  The FRAME submap --
four sensors in the corners of [0, 10] x [0, 8] looking inward -- is in most merges: its sensor positions are the extremes of the
box, so the grid is 40 x 32 cells at offset (0, 0) whatever the case itself adds inside."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import merge_rule as rule

RES = 0.25
SCALE = 4.0
PI = math.pi
IDENTITY = rule.IDENTITY
FAR = (1000.0, 1000.0, 0.0)

Laser = namedtuple("Laser", "n_beams min_angle ang_res min_range max_range range_threshold offset")
Sub = namedtuple("Sub", "laser scans")                       # scans: list of (pose (x, y, heading), ranges (n_beams,))
TraceCase = namedtuple("TraceCase", "name subs transforms resolution min_pass threshold check")
FitCase = namedtuple("FitCase", "name others transforms moving candidates resolution min_pass threshold own check")
Ctx = namedtuple("Ctx", "case subs grid")                    # what a check gets: the case, the rule's submaps, the rule's answer


def fan(n, min_range=0.1, max_range=7.5, range_threshold=5.0):
    """n beams all around, beam 0 along -x"""
    return Laser(n, -PI, 2.0 * PI / n, min_range, max_range, range_threshold, (0.0, 0.0, 0.0))


def ray(min_range=0.1, max_range=7.5, range_threshold=5.0):
    """one beam along the sensor's heading"""
    return Laser(1, 0.0, 1.0, min_range, max_range, range_threshold, (0.0, 0.0, 0.0))


def scan(x, y, heading, ranges):
    return (np.array([x, y, heading], dtype=np.float64), np.asarray(ranges, dtype=np.float64))


FRAME = Sub(ray(), [scan(0.0, 0.0, PI / 4, [1.0]), scan(10.0, 0.0, 3 * PI / 4, [1.0]), scan(10.0, 8.0, -3 * PI / 4, [1.0]),
                    scan(0.0, 8.0, -PI / 4, [1.0])])
W, H = 40, 32                                                # the grid FRAME makes


def rule_submap(sub):
    """the rule's view of a hand-made submap (tests/merge_rule.py's dict): the poses as given (no scan matching: corrected =
    odometric), the point readings by the oracle's LocalizedRangeScan::Update, the box over the sensor position and the in-range
    readings.  What tests/test_merge_gpu.py's _submap_of reads back from a mapper fed with the same scans."""
    from oracle import karto
    laser, scans = sub.laser, []
    for pose, ranges in sub.scans:
        sensor = rule.sensor_at(pose, laser.offset)
        points = karto.scan_points(ranges, sensor, laser)
        with np.errstate(invalid="ignore"):
            keep = (ranges >= laser.min_range) & (ranges <= laser.range_threshold)
        xs, ys = np.concatenate([[sensor[0]], points[keep, 0]]), np.concatenate([[sensor[1]], points[keep, 1]])
        scans.append({"ranges": ranges.copy(), "points": points, "corrected": pose.copy(), "odometric": pose.copy(),
                      "barycenter": np.array([points[keep, 0].mean(), points[keep, 1].mean(), 0.0]) if keep.any() else sensor.copy(),
                      "box": np.array([xs.min(), ys.min(), xs.max(), ys.max()])})
    return {"laser": laser, "scans": scans}


def gate(laser, r):
    """AddScan's decision about a reading: (kept, hit, clipped)"""
    if r <= laser.min_range or r >= laser.max_range or r != r:
        return False, False, False
    return True, r < laser.range_threshold - 1e-06, r >= laser.range_threshold


def beam_cells(sm, t, grid, resolution):
    """per scan of a rule submap under correction t: the sensor's cell coordinates and per kept beam (index, end cell coordinates,
    hit) -- the real-valued (v - offset) * scale before WorldToGrid rounds it, by the operations of the trace (AddScan's clip)"""
    laser, scale, off = sm["laser"], 1.0 / resolution, grid["offset"]
    out = []
    for s in sm["scans"]:
        ts = rule.transformed_scan(t, s, laser.offset)
        sx, sy = float(ts["sensor"][0]), float(ts["sensor"][1])
        beams = []
        for i, r in enumerate(s["ranges"]):
            kept, hit, clipped = gate(laser, float(r))
            if not kept:
                continue
            px, py = float(ts["points"][i, 0]), float(ts["points"][i, 1])
            if clipped:
                ratio = laser.range_threshold / float(r)
                px, py = sx + ratio * (px - sx), sy + ratio * (py - sy)
            beams.append((i, (px - off[0]) * scale, (py - off[1]) * scale, hit))
        out.append(((sx - off[0]) * scale, (sy - off[1]) * scale, beams))
    return out


def cell(v):
    return int(rule.round_half_away(v))


def is_tie(v):
    return abs(v) % 1.0 == 0.5


def gate_values(g):
    """(reading, kept, hit): the list of map_localize_cases.fit_cases()"""
    na, inf = np.nextafter, np.inf
    edge = g.range_threshold - 1e-06
    between = 0.5 * (g.range_threshold + g.max_range)
    return [(g.min_range, False, False), (na(g.min_range, inf), True, True), (0.5 * (g.min_range + edge), True, True),
            (na(edge, -inf), True, True), (edge, True, False), (g.range_threshold, True, False), (between, True, False),
            (na(g.max_range, -inf), True, False), (g.max_range, False, False), (np.nan, False, False), (inf, False, False),
            (-inf, False, False), (0.0, False, False), (-3.0, False, False)]


YAWS = [("0", 0.0), ("pi/2", PI / 2), ("-pi/2", -PI / 2), ("pi", PI), ("just below pi", float(np.nextafter(PI, 0.0))), ("-3", -3.0),
        ("1e-9", 1e-9)]
BEAM_COUNTS = (1, 63, 64, 65, 130)
GATED = fan(14, min_range=0.5, max_range=3.5, range_threshold=2.5)
GATE_POSE = (5.0625, 4.0625, 0.3)                            # a quarter cell off the cell centres: no rounding of the sensor's is near a tie
NEAR = (0.75, -0.5, 0.7)


def about(yaw, dx=0.0, dy=0.0, cx=5.0, cy=4.0):
    """the correction that turns by yaw about (cx, cy), the middle of FRAME's grid, and then moves by (dx, dy)"""
    return tuple(float(v) for v in rule.compose((cx + dx, cy + dy, 0.0), rule.compose((0.0, 0.0, yaw), (-cx, -cy, 0.0))))


def _total(grid):
    return int(grid["passes"][:, :grid["width"]].sum()), int(grid["hits"][:, :grid["width"]].sum())


# ---------------------------------------------------------------- the trace
# A submap mapped far away and brought back by a quarter turn: its point (-64, 1000) goes to x' = (c * -64 - 1000) + 1009.875 with
# c = cos(pi / 2) = 6.1e-17.  The difference absorbs c x = -3.9e-15 (half an ulp of 1000 is 5.7e-14) and the sum is 9.875 exactly,
# 39.5 cells: column 40.  Summed as c x - (1000 - 1009.875) the product survives (half an ulp of 9.875 is 8.9e-16): column 39.
AWAY = Sub(ray(), [scan(-65.75, 1000.0, 0.0, [1.75])])
AWAY_T = (1009.875, 68.0625, PI / 2)


def other_sum(t, x, y):
    c, s_ = rule.cos_sin(t[2])
    return c * x - (s_ * y - t[0])


def has_tie(dx, dy):
    """does Grid::TraceLine pass exactly between two cells on a line of these cell deltas?  (2 k minor = (2 m + 1) major for a step k:
    there the walk from the other end takes the other cell, which is how a turned line may differ from the line turned)"""
    major, minor = max(abs(dx), abs(dy)), min(abs(dx), abs(dy))
    return any((2 * k * minor) % (2 * major) == major for k in range(1, major))


def _tieless_scan(x, y, heading, n, seed):
    """a scan of a fan of n beams whose lines on the 0.25 m lattice of offset (0, 0) all walk clear of such ties: readings drawn from
    [0.5, 2.9) until the line of each beam has none"""
    rng, ranges = np.random.default_rng(seed), []
    for i in range(n):
        a = heading + (-PI + i * (2.0 * PI / n))
        while True:
            r = float(rng.uniform(0.5, 2.9))
            dx, dy = cell((x + r * math.cos(a)) * SCALE) - cell(x * SCALE), cell((y + r * math.sin(a)) * SCALE) - cell(y * SCALE)
            if not has_tie(dx, dy):
                break
        ranges.append(r)
    return scan(x, y, heading, ranges)


TURNED = Sub(fan(16), [_tieless_scan(5.0625, 4.0625, 0.3, 16, 59), _tieless_scan(6.3125, 3.0625, -2.0, 16, 61)])


def quarter_turn(u, t, yaw):
    """u: the merge under the identity, t: the same merge with every submap turned by yaw = +-pi / 2 about the origin (two dicts of
    width, height, passes, hits).  The box turns with the scans and its low corner is the offset, so cell (gx, gy) of u is cell
    (H - gy, gx) of t for +pi / 2 and (gy, W - gx) for -pi / 2: row 0 (column 0) of u falls on the first column (row) outside t."""
    w, h = u["width"], u["height"]
    assert (t["width"], t["height"]) == (h, w)
    for key in ("passes", "hits"):
        a, b = u[key][:h, :w], t[key][:w, :h]
        if yaw > 0:
            assert np.array_equal(b[:, 1:h], a[1:h, :].T[:, ::-1]), key
        else:
            assert np.array_equal(b[1:w, :], a[:, 1:w].T[::-1, :]), key
    assert int(u["hits"].sum()) > 30

def _layout_subs(rng, counts):
    """lasers of 1, 130, 63, 64 and 65 beams in id order (the short ones first, in the middle and last), counts[k] scans each"""
    subs = []
    for n, m in zip((1, 130, 63, 64, 65), counts):
        scans = []
        for k in range(m):
            x, y = 2.0 + 0.125 * int(rng.integers(0, 48)), 2.0 + 0.125 * int(rng.integers(0, 32))
            scans.append(scan(x + 1.0 * k, y, float(rng.uniform(-3.0, 3.0)), rng.uniform(0.3, 1.9, size=n)))
        subs.append(Sub(fan(n), scans))
    return subs


def trace_cases():
    out = []
    rng = np.random.default_rng(41)

    def add(name, subs, transforms, check=lambda ctx: None, resolution=RES, min_pass=2, threshold=0.1):
        assert len(subs) == len(transforms)
        out.append(TraceCase(name, subs, [tuple(float(v) for v in t) for t in transforms], resolution, min_pass, threshold, check))

    # ---- the work layout: max_runs = 3 waves per scan, four waves per workgroup
    for counts in ((2, 1, 2, 1, 2), (2, 1, 2, 1, 1), (2, 1, 1, 1, 1), (1, 1, 1, 1, 1)):
        n_scans = len(FRAME.scans) + sum(counts)

        def layout(ctx, n_scans=n_scans):
            lasers = [sm["laser"].n_beams for sm in ctx.subs if sm["scans"]]
            assert (max(lasers) + 63) // 64 == 3 and sum(len(sm["scans"]) for sm in ctx.subs) == n_scans
            assert lasers == [1, 1, 130, 63, 64, 65], "short lasers first, in the middle and last"
            p, h = _total(ctx.grid)
            readings = sum(len(s["ranges"]) for sm in ctx.subs for s in sm["scans"])
            assert 0.9 * readings <= h <= readings and p > 2 * h, "every reading is a hit; an end on the last row or column is outside"
        add(f"lasers of 1, 130, 63, 64, 65 beams, {n_scans} scans: {(n_scans * 3) % 4} waves in the last workgroup",
            [FRAME] + _layout_subs(rng, counts), [IDENTITY, (0.5, 0.25, 0.0), IDENTITY, NEAR, about(-2.0, -0.5, 0.5), about(3.0, 0.25, -0.75)], layout,
            min_pass=0)

    def lone(ctx):
        assert len(ctx.subs) == 1 and len(ctx.subs[0]["scans"]) == 1 and ctx.subs[0]["laser"].n_beams == 1
        assert ctx.grid["width"] > 1 and ctx.grid["height"] > 1 and _total(ctx.grid)[0] >= 2
    add("one scan of one beam as the whole merge", [Sub(ray(), [scan(1.0, 2.0, 0.5, [2.0])])], [NEAR], lone, min_pass=0)

    empty = Sub(fan(130), [])

    def not_in_max_beams(ctx):
        with_scans = [sm["laser"].n_beams for sm in ctx.subs if sm["scans"]]
        assert [len(sm["scans"]) for sm in ctx.subs] == [4, 2, 0, 2] and max(with_scans) == 64 and ctx.subs[2]["laser"].n_beams == 130
    add("a submap without scans between two with scans",
        [FRAME, Sub(fan(64), [scan(3.0, 3.0, 0.2, rng.uniform(0.3, 1.9, size=64)), scan(4.5, 3.0, 1.2, rng.uniform(0.3, 1.9, size=64))]), empty,
         Sub(fan(64), [scan(6.0, 5.0, -1.0, rng.uniform(0.3, 1.9, size=64)), scan(7.5, 5.0, 2.0, rng.uniform(0.3, 1.9, size=64))])],
        [IDENTITY, (0.25, 0.0, 0.1), (3.0, 3.0, 3.0), IDENTITY], not_in_max_beams, min_pass=0)

    # ---- the per-submap record: two lasers that gate the same readings differently
    wide, tight = fan(5, 0.1, 6.0, 3.5), fan(5, 1.0, 3.0, 2.0)
    readings = [0.5, 2.5, 4.0, 1.5, 3.2]

    def two_gates(ctx):
        decisions = [(gate(wide, r), gate(tight, r)) for r in readings]
        assert decisions[0] == ((True, True, False), (False, False, False)), "kept by one, dropped by the other"
        assert decisions[1] == ((True, True, False), (True, False, True)), "a hit for one, clipped by the other"
        assert decisions[2] == ((True, False, True), (False, False, False)), "clipped by one, dropped by the other"
        assert decisions[3][0] == decisions[3][1] == (True, True, False)
        g = ctx.grid
        for k, hits in ((1, 4), (2, 1)):                     # each submap under its own gates and under submap 0's, on the same boxes
            own = rule.submap_counters(ctx.subs[k], ctx.case.transforms[k], g["width"], g["height"], g["offset"], RES)
            as_0 = rule.submap_counters(dict(ctx.subs[k], laser=ctx.subs[0]["laser"]), ctx.case.transforms[k], g["width"], g["height"], g["offset"], RES)
            assert int(own[1].sum()) == hits and int(as_0[1].sum()) == 5, "submap 0's gates make a hit of every one of the five readings"
            assert not np.array_equal(own[0], as_0[0]) and not np.array_equal(own[1], as_0[1])
        as_1 = rule.submap_counters(dict(ctx.subs[2], laser=wide), ctx.case.transforms[2], g["width"], g["height"], g["offset"], RES)
        assert int(as_1[1].sum()) == 4, "... and submap 1's gates four"
    add("two submaps with different gates",
        [FRAME, Sub(wide, [scan(4.0625, 4.0625, 0.4, readings)]), Sub(tight, [scan(5.0625, 4.0625, -0.4, readings)])],
        [IDENTITY, about(0.3, 0.5, 0.0), about(0.7, 0.25, 0.25)],
        two_gates, min_pass=0)

    # ---- the gate values, one beam each, under a correction that turns
    values = gate_values(GATED)

    def gated(ctx):
        g, sm, t = ctx.grid, ctx.subs[1], ctx.case.transforms[1]
        for i, (value, kept, hit) in enumerate(values):
            ranges = np.full(len(values), np.nan)
            ranges[i] = value
            alone = {"laser": sm["laser"], "scans": [dict(sm["scans"][0], ranges=ranges)]}
            p, h = rule.submap_counters(alone, t, g["width"], g["height"], g["offset"], RES)
            assert (int(p.sum()) > 0) == kept and int(h.sum()) == int(hit), (i, value)
            if kept and value >= GATED.range_threshold:
                assert 8 <= int(p.sum()) <= 11, "the clipped beam is 2.5 m = 10 cells long, and its end is no hit"
    add("every gate value under a correction with a yaw", [FRAME, Sub(GATED, [scan(*GATE_POSE, [v for v, _, _ in values])])],
        [IDENTITY, about(0.7, 0.75, -0.5)], gated, min_pass=0)

    # ---- a clipped end on a cell boundary: threshold 2.125 m = 8.5 cells, a reading of twice that: ratio 0.5, every operation exact
    half = ray(range_threshold=2.125)

    def clipped_tie(ctx):
        (sx, sy, beams), = beam_cells(ctx.subs[1], ctx.case.transforms[1], ctx.grid, RES)
        (i, ex, ey, hit), = beams
        assert (sx, sy, ex, ey, hit) == (21.0, 14.0, 29.5, 14.0, False) and is_tie(ex)
        row = ctx.grid["passes"][14]
        assert row[21:31].tolist() == [1] * 10 and row[31] == 0, "29.5 rounds away from zero: the end cell is 30"
    add("a clipped end on a cell boundary", [FRAME, Sub(half, [scan(4.0, 3.0, 0.0, [4.25])])], [IDENTITY, (1.25, 0.5, 0.0)], clipped_tie, min_pass=0)

    # ---- yaws
    for name, yaw in YAWS:
        def some(ctx):
            assert _total(ctx.grid)[1] >= 28
        add(f"yaw {name}", [FRAME, TURNED], [IDENTITY, about(yaw)], some, min_pass=0)
    # ... and everything turned by a quarter about the origin: the counters of the identity run, transposed and mirrored
    for name, yaw in YAWS[:3]:
        def quarter(ctx, yaw=yaw):
            if yaw:
                quarter_turn(rule.merged_grid(ctx.subs, [IDENTITY, IDENTITY], RES, 0, 0.1), ctx.grid, yaw)
        add(f"the whole merge turned by {name}", [FRAME, TURNED], [(0.0, 0.0, yaw)] * 2, quarter, min_pass=0)

    # ---- translations by whole cells and by exactly half a cell
    for name, t, want in (("whole cells", (1.0, -0.5, 0.0), (20.0, 10.0, 28.0)), ("plus half a cell", (0.125, 0.125, 0.0), (16.5, 12.5, 24.5)),
                          ("minus half a cell", (-0.125, -0.125, 0.0), (15.5, 11.5, 23.5))):
        def shifted(ctx, want=want):
            (sx, sy, beams), = beam_cells(ctx.subs[1], ctx.case.transforms[1], ctx.grid, RES)
            (i, ex, ey, hit), = beams
            assert (sx, sy, ex, ey) == (want[0], want[1], want[2], want[1]) and hit
            if want[0] % 1.0:
                assert all(is_tie(v) for v in (sx, sy, ex, ey)), "sensor and end lie on a rounding tie on both axes"
            g = ctx.grid
            assert g["hits"][cell(ey), cell(ex)] == 1 and g["passes"][cell(sy), cell(sx)] == 1
            assert g["passes"][cell(sy), cell(sx) - 1] == 0 and g["passes"][cell(ey), cell(ex) + 1] == 0
        add(f"translation by {name}", [FRAME, Sub(ray(), [scan(4.0, 3.0, 0.0, [2.0])])], [IDENTITY, t], shifted, min_pass=0)

    # ---- the order of the point's sum: x' = (c x - s y) + tx, not c x - (s y - tx)
    def summed(ctx):
        (sx, sy, beams), = beam_cells(ctx.subs[1], AWAY_T, ctx.grid, RES)
        (i, ex, ey, hit), = beams
        assert (sx, ex, hit) == (39.5, 39.5, True) and not is_tie(sy) and not is_tie(ey), "a vertical line on the tie between columns 39 and 40"
        assert other_sum(AWAY_T, -64.0, 1000.0) * SCALE < 39.5, "the other association keeps c x and lands in column 39"
        frame = rule.submap_counters(ctx.subs[0], IDENTITY, W, H, (0.0, 0.0), RES)
        assert _total(ctx.grid) == (int(frame[0].sum()), int(frame[1].sum())), "column 40 is outside: the line and its hit count nothing"
    add("the order of the point's sum decides the column", [FRAME, AWAY], [IDENTITY, AWAY_T], summed, min_pass=0)

    # ---- walks
    def star(ctx):
        (sx, sy, beams), = beam_cells(ctx.subs[1], IDENTITY, ctx.grid, RES)
        kinds = set()
        for i, ex, ey, hit in beams:
            dx, dy = cell(ex) - cell(sx), cell(ey) - cell(sy)
            kinds.add((int(np.sign(dx)), int(np.sign(dy)), abs(dy) > abs(dx)))
        assert len(beams) == 16 and len(kinds) == 12, "eight octants and the four axis directions"
        assert _total(ctx.grid)[1] == 16 + 4
    add("all eight octants and both axis directions", [FRAME, Sub(fan(16), [scan(5.0, 4.0, 0.0, np.full(16, 3.1))])], [IDENTITY, IDENTITY], star, min_pass=0)

    def on_the_spot(ctx):
        g = ctx.grid
        assert g["passes"][16, 20] == 2 and g["hits"][16, 20] == 1, "visited once by the line and once as the hit"
        frame = rule.submap_counters(ctx.subs[0], IDENTITY, g["width"], g["height"], g["offset"], RES)
        assert _total(g) == (2 + int(frame[0].sum()), 1 + int(frame[1].sum()))
    add("a zero-length beam", [FRAME, Sub(ray(min_range=0.0), [scan(5.0, 4.0, 0.7, [1e-9])])], [IDENTITY, IDENTITY], on_the_spot, min_pass=0)

    crossing = [FRAME, Sub(ray(), [scan(3.0, 3.0, 0.0, [2.0])]), Sub(ray(), [scan(5.0, 1.0, PI / 2, [2.0]), scan(4.0, 2.0, PI / 2, [2.0])])]

    def crossed(ctx):
        g = ctx.grid
        assert (g["passes"][12, 20], g["hits"][12, 20]) == (4, 2), "two ends in one cell: each visits it twice and hits it once"
        assert (g["passes"][12, 16], g["hits"][12, 16]) == (2, 0), "two lines cross"
    add("lines of two submaps that cross, ends of two submaps in one cell", crossing, [IDENTITY] * 3, crossed, min_pass=0)

    # ---- the update rule on the same counters: the shared end cell has hits / pass = 2 / 4, the crossing 0 / 2
    below = float(np.nextafter(0.5, 0.0))
    for min_pass, threshold, end, cross in ((0, 0.5, 255, 255), (0, below, 100, 255), (3, below, 100, 0), (3, 0.5, 255, 0)):
        def updated(ctx, end=end, cross=cross):
            g = ctx.grid
            assert g["hits"][12, 20] / g["passes"][12, 20] == 0.5, "the ratio equals the threshold: > decides"
            assert (g["cells"][12, 20], g["cells"][12, 16]) == (end, cross)
        add(f"min_pass_through {min_pass}, occupancy threshold {threshold!r}", crossing, [IDENTITY] * 3, updated, min_pass=min_pass, threshold=threshold)
    return out


def build_bound(case, subs, grid):
    """What kh_merge_build relies on instead of a guard: the grid is ComputeDimensions of the loose boxes of the same transformed
    scans, so the sensor cell and the end cell of every kept beam lie within range_threshold * scale + 2 cells of it."""
    n = 0
    for sm, t in zip(subs, case.transforms):
        reach = sm["laser"].range_threshold / case.resolution + 2.0
        for sx, sy, beams in beam_cells(sm, t, grid, case.resolution):
            for x, y in [(sx, sy)] + [(ex, ey) for _, ex, ey, _ in beams]:
                assert -reach <= x <= grid["width"] + reach and -reach <= y <= grid["height"] + reach, (case.name, x, y)
                n += 1
    return n


# ---------------------------------------------------------------- the fit
# The reference: FRAME and a room -- one sensor in the middle whose 130 beams end on a circle of 2.5 m.  With min_pass_through 0 the
# disc is free, its rim occupied and the rest of the 40 x 32 grid unknown, but for FRAME's four short lines.
ROOM = Sub(fan(130), [scan(5.0625, 4.0625, 0.0, np.full(130, 2.5))])
REFERENCE = ([FRAME, ROOM], [IDENTITY, IDENTITY])
ORIGIN_RAY = Sub(ray(), [scan(0.0, 0.0, 0.0, [1.75])])      # the point is (1.75, 0) exactly: a candidate alone places sensor and end


def _visits(f):
    return f["pass_unknown"] + f["pass_occupied"] + f["pass_free"], f["hits_unknown"] + f["hits_occupied"] + f["hits_free"]


def layout_candidates():
    """70 candidates about the room; numbers 1 and 3 put every beam outside the grid, so each of the lists [:2], [:5] and [:70] ..."""
    rng = np.random.default_rng(43)
    c = np.array([about(yaw, dx, dy) for yaw, dx, dy in zip(rng.uniform(-3.1, 3.1, size=70), rng.uniform(-1.0, 1.0, size=70), rng.uniform(-1.0, 1.0, size=70))])
    c[0] = IDENTITY
    c[1], c[3] = FAR, (-500.0, 300.0, 1.0)
    return c


def layout_moving():
    """(beams, scans): scans * runs % 4 = 1, 2, 3 for every beam count that has more than one such remainder"""
    rng = np.random.default_rng(47)
    out = []
    for n, m in ((1, 1), (1, 3), (63, 2), (64, 3), (65, 3), (130, 1), (130, 2), (130, 3)):
        scans = [scan(4.125 + 1.0 * k, 3.625 + 0.5 * k, float(rng.uniform(-3.0, 3.0)), rng.uniform(0.4, 3.2, size=n)) for k in range(m)]
        out.append(Sub(fan(n), scans))
    return out


def fit_cases():
    out = []
    rng = np.random.default_rng(53)

    def add(name, moving, candidates, check=lambda fits, grid: None, reference=REFERENCE, resolution=RES, min_pass=0, threshold=0.1, own=None):
        cands = np.asarray(candidates, dtype=np.float64).reshape(-1, 3)
        out.append(FitCase(name, reference[0], [tuple(t) for t in reference[1]], moving, cands, resolution, min_pass, threshold, own, check))

    # ---- the layout: one wave per (candidate, scan, run of 64 beams), a workgroup never across two candidates
    cands = layout_candidates()
    for moving in layout_moving():
        n, m = moving.laser.n_beams, len(moving.scans)
        part = (m * ((n + 63) // 64)) % 4
        for count in (1, 2, 5, 70):
            def dealt(fits, grid, count=count, part=part):
                assert part != 0, "the last workgroup of every candidate is partly empty"
                assert _visits(fits[0])[0] > 0 and (count == 2 or _visits(fits[-1])[0] > 0)
                if count > 1:
                    assert _visits(fits[1]) == (0, 0) and fits[1]["score"] == 0.0
                if count > 4:
                    assert _visits(fits[3]) == (0, 0) and _visits(fits[2])[0] > 0 and _visits(fits[4])[0] > 0, "zeros between non-zeros"
            add(f"{n} beams, {m} scans ({part} waves in a candidate's last workgroup), {count} candidates", moving, cands[:count], dealt)

    # ---- the three states under the end of a beam: the ray's end 1.75 m ahead of where the candidate puts the origin
    def states(fits, grid):
        c = grid["cells"]
        assert (c[17, 38], c[17, 30], c[17, 25]) == (0, 100, 255), "the end cells: unknown, on the rim, inside the room"
        assert [(f["hits_unknown"], f["hits_occupied"], f["hits_free"]) for f in fits] == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
        assert fits[0]["pass_unknown"] == 8 + 1 and _visits(fits[0]) == (9, 1), "eight cells of the line, the end cell once more as the hit"
        assert fits[2]["pass_free"] == 9, "the hit end is counted twice in pass and once in hits"
        assert fits[0]["known"] == 0 and fits[0]["score"] == 0.0 and fits[0]["pass_unknown"] > 0, "nothing known: the score is 0.0"
    add("ends on an unknown, an occupied and a free cell", ORIGIN_RAY, [(7.75, 4.25, 0.0), (5.75, 4.25, 0.0), (4.5, 4.25, 0.0)], states)

    # ---- the four sides of the grid
    around = Sub(fan(16), [scan(0.0, 0.0, 0.0, np.full(16, 3.0))])
    sides = [(5.0625, 4.0625), (1.0625, 4.0625), (8.9375, 4.0625), (5.0625, 1.0625), (5.0625, 6.9375), (-1.0625, 4.0625), (11.0625, 4.0625),
             (5.0625, -1.0625), (5.0625, 9.0625)]

    def through_the_sides(fits, grid):
        full = _visits(fits[0])
        assert full[1] == 16
        for f in fits[1:5]:
            assert 0 < _visits(f)[0] < full[0] and 0 < _visits(f)[1] < 16, "the sensor inside, ends leaving through one side"
        for f in fits[5:]:
            assert 0 < _visits(f)[0] < full[0] and 0 < _visits(f)[1] < 8, "the sensor outside, beams entering through one side"
    add("the sensor inside and outside on each of the four sides", around, [(x, y, 0.2) for x, y in sides], through_the_sides)

    # ---- the last cell inside and the first outside, on every side: the end 7 cells from the sensor, along +x, +y, -x, -y
    quarter = [(0.0, ((8.0, 4.0), (8.25, 4.0))), (PI / 2, ((5.0, 6.0), (5.0, 6.25))), (PI, ((1.75, 4.0), (1.5, 4.0))), (-PI / 2, ((5.0, 1.75), (5.0, 1.5)))]
    edge_cands = [(x, y, yaw) for yaw, pair in quarter for x, y in pair]

    def last_and_first(fits, grid):
        ends = []
        for f, c in zip(fits, edge_cands):
            ex, ey = rule.transform_point(c, 1.75, 0.0)
            ends.append((cell((ex - 0.0) * SCALE), cell((ey - 0.0) * SCALE)))
        assert [e[0] for e in ends[:2]] == [W - 1, W] and [e[1] for e in ends[2:4]] == [H - 1, H]
        assert [e[0] for e in ends[4:6]] == [0, -1] and [e[1] for e in ends[6:]] == [0, -1]
        assert [_visits(f) for f in fits] == [(9, 1), (7, 0)] * 4, "the first of each pair counts its end, the second does not"
    add("end cells at width - 1, width, height - 1, height, 0 and -1", ORIGIN_RAY, edge_cands, last_and_first)

    # ---- the arithmetic of the candidate: yaws, half-cell ties, gate values
    add("the yaws as candidates", TURNED, [about(yaw) for _, yaw in YAWS], lambda fits, grid: None if all(_visits(f)[1] >= 28 for f in fits) else 1 / 0)

    ties = [(4.0, 3.0, 0.0), (4.125, 3.125, 0.0), (3.875, 2.875, 0.0), (-0.625, 3.125, 0.0), (4.125, -0.625, 0.0)]

    def tied(fits, grid):
        for c, f, want in zip(ties, fits, ((9, 1), (9, 1), (9, 1), (7, 1), (0, 0))):
            sx, sy = rule.transform_point(c, 0.0, 0.0)
            ex, ey = rule.transform_point(c, 1.75, 0.0)
            coords = [v * SCALE for v in (sx, sy, ex, ey)]
            assert all(is_tie(v) for v in coords) == (c != ties[0]) and _visits(f) == want, (c, coords)
        # the ties below zero round away from it as those above do: the sensor's -2.5 to -3, so that cells 0 .. 5 and the hit count
        assert cell(-0.625 * SCALE) == -3 and cell((-0.625 + 1.75) * SCALE) == 5
    add("half-cell ties on both sides of zero", ORIGIN_RAY, ties, tied)

    def summed(fits, grid):
        ex, _ = rule.transform_point(AWAY_T, -64.0, 1000.0)
        assert ex * SCALE == 39.5 and other_sum(AWAY_T, -64.0, 1000.0) * SCALE < 39.5
        assert _visits(fits[0]) == (0, 0) and _visits(fits[1]) == (9, 1), "column 40 is outside; a cell to the left the same line counts"
    add("the order of the point's sum decides the column", AWAY, [AWAY_T, (AWAY_T[0] - RES, AWAY_T[1], AWAY_T[2])], summed)

    values = gate_values(GATED)

    def gated(fits, grid):
        kept = sum(k for _, k, _ in values)
        assert _visits(fits[0])[1] == _visits(fits[1])[1] == sum(h for _, _, h in values) and kept == 7
        assert _visits(fits[0])[0] > 7 * 3
    add("every gate value under a candidate with a yaw", Sub(GATED, [scan(*GATE_POSE, [v for v, _, _ in values])]),
        [about(0.7, 0.75, -0.5), about(0.0, 0.25, 0.0)], gated)

    # one reading per value, alone: a single beam cannot hide behind another
    for value, kept, hit in values:
        def one(fits, grid, kept=kept, hit=hit):
            assert (_visits(fits[0])[0] > 0, _visits(fits[0])[1]) == (kept, int(hit))
        add(f"reading {float(value)!r} alone", Sub(ray(GATED.min_range, GATED.max_range, GATED.range_threshold), [scan(*GATE_POSE, [value])]),
            [about(0.7, 0.75, -0.5)], one)

    # ---- the submap's own correction plays no part
    add("the submap's own correction is a quarter turn, the fit is under the identity", Sub(fan(16), [scan(5.0625, 4.0625, 0.3, rng.uniform(0.5, 2.9, size=16))]),
        [IDENTITY], lambda fits, grid: None if _visits(fits[0])[1] == 16 else 1 / 0, own=(1.0, 2.0, PI / 2))
    return out


# ---------------------------------------------------------------- the bound of the fit (kh_merge_fit's refusals)
BOUND = 2.0 ** 30 * RES                                      # metres from the offset (0, 0) of FRAME's grid to cell 2^30
ACCEPTED = [(BOUND, 4.0, 0.0), (-BOUND, 4.0, 0.0), (5.0, BOUND, 0.0), (5.0, -BOUND, 0.0), FAR]
REFUSED = [(BOUND + 1.0, 4.0, 0.0), (-BOUND - 1.0, 4.0, 0.0), (5.0, BOUND + 1.0, 0.0), (5.0, -BOUND - 1.0, 0.0)]
# a laser that walks too far at a fine resolution: 20 m are 2 000 000 cells of 1e-5 m; the reference there is a few millimetres wide
FINE_RES = 1e-5
LONG_LASER = Sub(fan(8, 0.1, 30.0, 20.0), [scan(0.0, 0.0, 0.0, np.full(8, 3.0))])
TINY = Sub(ray(min_range=1e-4), [scan(0.0, 0.0, 0.7, [0.003])])
NOT_FINITE = [tuple(v if k == place else 0.5 for k in range(3)) for place in range(3) for v in (math.nan, math.inf, -math.inf)]
