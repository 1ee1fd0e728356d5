"""The host rules of the footprint analysis (slam_toolbox_amd/csrc/map_footprint_plan.hpp) on the CPU, through the stand-alone program
tests/map_footprint_plan_check.cpp, built with the address and undefined-behaviour sanitizers where the compiler has them: every
refusal in order, convexity, the reach on, just below and just above a cell count, 255 taken and 256 refused, 64 taken and 65 refused
for the layer, the span function for every triangle of a 7 x 7 box, vertex cells and heading offsets bit for bit -- against
tests/map_footprint_rule.py.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import map_footprint_cases as cases
import map_footprint_rule as rule
import map_localize_rule as ml

HERE = os.path.dirname(os.path.abspath(__file__))
REASONS = {2: "n_vertices", 3: "finite", 4: "convex", 5: "reach"}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_footprint_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_footprint_plan_check.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)                       # a compiler without the sanitizers' runtimes

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout[-2000:]
        return out
    return run


def hx(v):
    return float(v).hex()


def flat(verts):
    return "%d %s" % (len(verts), " ".join(hx(v) for p in verts for v in p))


def rule_says(verts, scale):
    try:
        return "0 %d" % rule.create_check(verts, scale)
    except rule.Refused as e:
        return str({w: k for k, w in REASONS.items()}[str(e)])


R = cases.RECTANGLE
STAR = [(math.cos(4.0 * math.pi * k / 5), math.sin(4.0 * math.pi * k / 5)) for k in range(5)]
CREATES = [
    (R, 20.0, "0 13"), (R[::-1], 20.0, "0 13"), (cases.TRIANGLE, 20.0, "0 15"), (cases.polygon(16, 0.44), 20.0, "0 10"), (cases.ONE_CELL, 4.0, "0 2"),
    (cases.SMALL_2, 4.0, "0 2"), (cases.LONG_64, 4.0, "0 64"), (cases.DIAMOND_255, 4.0, "0 255"),
    # the count
    (R[:2], 20.0, "2"), (cases.polygon(17, 0.45), 20.0, "2"), ([], 20.0, "2"),
    # finite
    ([(math.nan, 0.0)] + R[1:], 20.0, "3"), (R[:3] + [(0.5, math.inf)], 20.0, "3"),
    # convexity: a collinear triple, a reflex vertex (both windings), a repeated vertex, a star that goes round twice
    ([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (1.0, 1.0)], 20.0, "4"), ([(0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 2.0)], 20.0, "4"),
    ([(0.0, 0.0), (2.0, 0.0), (0.5, 0.5), (0.0, 2.0)][::-1], 20.0, "4"), ([(0.0, 0.0), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], 20.0, "4"), (STAR, 4.0, "4"),
    ([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)], 20.0, "4"),
    # the reach: 255 is taken, 256 refused
    ([(63.5, 0.0), (0.0, 63.5), (-63.5, 0.0)], 4.0, "0 255"), ([(float(np.nextafter(63.5, 99.0)), 0.0), (0.0, 63.5), (-63.5, 0.0)], 4.0, "5"),
    ([(1e200, 0.0), (0.0, 1e200), (-1e200, 0.0)], 4.0, "5"), (R, 1e6, "5"),
    # the order
    ([(math.nan, 0.0), (1.0, 0.0)], 20.0, "2"), ([(math.nan, 0.0), (1.0, 0.0), (2.0, 0.0)], 20.0, "3"), ([(0.0, 0.0), (1e200, 0.0), (2e200, 0.0)], 20.0, "4"),
]


def test_every_refusal_of_create_in_order(check):
    got = check(["create 0 %s %s" % (hx(s), flat(v)) for v, s, _ in CREATES])
    for (v, s, want), text in zip(CREATES, got):
        assert text == want == rule_says(v, s), (v, s)
    assert check(["create %d %s %s" % (n, hx(20.0), flat(R)) for n in (1, 2, 4, 7)]) == ["1"] * 4
    assert check(["create 1 %s %s" % (hx(20.0), flat(R[:2]))]) == ["1"], "a NULL comes first"


def test_convexity_in_both_windings(check):
    rng = np.random.default_rng(5)
    polys = [R, R[::-1], cases.TRIANGLE, cases.TRIANGLE[::-1], STAR, STAR[::-1]]
    for n in (3, 5, 8, 16):
        good = cases.polygon(n, 1.0 + rng.uniform())
        dented = list(good)
        dented[1] = (0.1 * good[1][0], 0.1 * good[1][1])
        polys += [good, good[::-1], dented if n > 3 else good, dented[::-1] if n > 3 else good]
    got = check(["convex " + flat(p) for p in polys])
    for p, text in zip(polys, got):
        assert int(text) == int(rule.convex(p)), p
    assert [int(t) for t in got[:6]] == [1, 1, 1, 1, 0, 0] and got[8] == "1" and got[-2:] == ["0", "0"]


def test_the_reach_on_below_and_above_a_cell_count(check):
    na = np.nextafter
    tri = lambda r: [(r, 0.0), (-0.1, 0.1), (-0.1, -0.1)]  # noqa: E731
    rows = [(0.5, 20.0, 11), (float(na(0.5, 0.0)), 20.0, 11), (float(na(0.5, 9.0)), 20.0, 12), (0.25, 4.0, 2), (float(na(0.25, 9.0)), 4.0, 3), (63.5, 4.0, 255),
            (float(na(63.5, 99.0)), 4.0, 256), (15.75, 4.0, 64), (float(na(15.75, 99.0)), 4.0, 65), (0.3, 10.0, 4)]
    got = check(["reach %s %s" % (hx(s), flat(tri(r))) for r, s, _ in rows])
    for (r, s, want), text in zip(rows, got):
        assert float(text) == want == rule.reach_of(tri(r), s), (r, s)
    assert check(["layer 7 0 64", "layer 7 0 65", "layer 0 0 64", "layer 33 3 65", "layer 1 -1 65", "layer 32 2 2", "layer 1 3 2"]) == ["0", "3", "1", "1", "2", "0", "2"]
    for args, want in (((7, 0, 64), None), ((7, 0, 65), "layer reach"), ((0, 0, 64), "n_headings"), ((1, 3, 2), "max_status")):
        if want is None:
            rule.layer_check(*args)
        else:
            with pytest.raises(rule.Refused) as e:
                rule.layer_check(*args)
            assert str(e.value) == want


def test_every_refusal_of_a_check_in_order(check):
    rows = [("check 0 5 -1 0x0p+0", "0"), ("check 0 0 -1 0x0p+0", "1"), ("check 0 -2 -1 0x0p+0", "1"), ("check 0 65537 -1 0x0p+0", "1"), ("check 0 65536 -1 0x0p+0", "0"),
            ("check 1 5 -1 0x0p+0", "2"), ("check 2 5 -1 0x0p+0", "2"), ("check 0 5 7 nan", "3 2"), ("check 0 5 14 inf", "3 4"), ("check 0 5 0 -inf", "3 0"),
            ("check 0 5 3 %s" % hx(1e300), "0"), ("check 3 0 0 nan", "1"), ("check 1 5 0 nan", "2")]
    assert check([r for r, _ in rows]) == [w for _, w in rows]


def test_the_span_function_for_every_triangle_of_a_7_x_7_box(check):
    got = np.array([int(t, 16) for t in check(["triangles"])[0].split()], dtype=np.uint64)
    assert got.size == 49 ** 3
    # the rule's edges once per pair of cells: per row of the box the smallest and the largest column of TraceLine's cells
    lo, hi = np.full((49, 49, 7), 99, dtype=np.int64), np.full((49, 49, 7), -1, dtype=np.int64)
    for a in range(49):
        for b in range(49):
            x, y = ml.line_cells(a % 7, a // 7, b % 7, b // 7)
            np.minimum.at(lo[a, b], y, x)
            np.maximum.at(hi[a, b], y, x)
    k = np.arange(49)
    a, b, c = (v.ravel() for v in np.meshgrid(k, k, k, indexing="ij"))
    t_lo = np.minimum(np.minimum(lo[a, b], lo[b, c]), lo[c, a])
    t_hi = np.maximum(np.maximum(hi[a, b], hi[b, c]), hi[c, a])
    rows = np.where(t_lo <= t_hi, (np.int64(1) << (t_hi + 1)) - (np.int64(1) << np.minimum(t_lo, 62)), 0)
    want = (rows << (7 * np.arange(7, dtype=np.int64))[None, :]).sum(axis=1).astype(np.uint64)
    assert np.array_equal(got, want), f"{int((got != want).sum())} triangles differ"
    rng = np.random.default_rng(2)
    for t in rng.integers(0, 49 ** 3, 200):                    # ... and rule.spans itself on some of them, through the "spans" command
        cells = [(int(v) % 7, int(v) // 7) for v in (a[t], b[t], c[t])]
        y0, s_lo, s_hi = rule.spans(cells)
        text = check(["spans 3 " + " ".join("%d %d" % p for p in cells)])[0]
        assert [int(v) for v in text.split()] == [y0] + [int(v) for pair in zip(s_lo, s_hi) for v in pair]
        mask = sum(1 << (7 * (y0 + r) + x) for r in range(len(s_lo)) for x in range(int(s_lo[r]), int(s_hi[r]) + 1))
        assert mask == int(got[t])
    far = check(["spans 3 0 0 511 3 4 2", "spans 3 0 0 510 3 4 2", "spans 3 0 0 3 511 4 2"])
    assert far[0] == "none" and far[1] != "none" and far[2] == "none"


def test_vertex_cells_and_heading_offsets_bit_for_bit(check):
    rng = np.random.default_rng(4)
    lines, wants = [], []
    polys = [R, cases.TRIANGLE, cases.polygon(16, 0.45), cases.ONE_CELL, cases.DIAMOND_255]
    for n in range(400):
        verts = polys[n % len(polys)]
        scale, ax, ay = (4.0, 20.0, 10.0, 7.3)[n % 4], rng.uniform(-3, 3), rng.uniform(-3, 3)
        pose = (rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-7, 7))
        if n % 50 == 0:                                        # half-way cases: a vertex exactly between two cells
            ax, ay, pose = 0.0, 0.0, (0.125 * (n // 50), -0.125, 0.0)
        if n % 97 == 0:
            pose = (2.0 ** 30 / scale + rng.uniform(-2, 2), pose[1], pose[2])
        lines.append("cells %s %s %s %s %s %s %s" % (hx(scale), hx(ax), hx(ay), hx(pose[0]), hx(pose[1]), hx(pose[2]), flat(verts)))
        cells = rule.pose_cells(verts, pose, (ax, ay), scale)
        own = None if cells is None else (rule._cell((pose[0] - ax) * scale), rule._cell((pose[1] - ay) * scale))
        wants.append("L" if cells is None else " ".join(str(v) for p in [own] + cells for v in p))
    assert check(lines) == wants and "L" in wants
    lines, wants = [], []
    for verts, scale in ((R, 20.0), (cases.TRIANGLE, 10.0), (cases.LONG_64, 4.0), (cases.polygon(16, 0.45), 7.3)):
        for n_headings in (1, 7, 8, 32):
            for h in range(n_headings):
                lines.append("offsets %s %d %d %s" % (hx(scale), h, n_headings, flat(verts)))
                wants.append(" ".join(str(v) for p in rule.heading_offsets(verts, h, n_headings, scale) for v in p))
    assert check(lines) == wants


def test_the_layer_s_table_is_the_rule_s_spans(check):
    for verts, scale, reach, n_headings in ((R, 20.0, 13, 7), (cases.LONG_64, 4.0, 64, 32), (cases.SMALL_2, 4.0, 2, 1)):
        words = [int(v) for v in check(["table %s %d %d %s" % (hx(scale), reach, n_headings, flat(verts))])[0].split()]
        rows, table = words[0], words[1:]
        total = 0
        for h in range(n_headings):
            first, y0, n_rows, zero = table[4 * h:4 * h + 4]
            w_y0, lo, hi = rule.spans(rule.heading_offsets(verts, h, n_headings, scale))
            assert (y0, n_rows, zero) == (w_y0, len(lo), 0)
            assert table[first:first + 2 * n_rows] == [int(v) for pair in zip(lo, hi) for v in pair]
            total += n_rows
        assert rows == total and len(table) % 4 == 0
    assert check(["table %s 9 7 %s" % (hx(20.0), flat(R))]) == ["none"], "an offset beyond the reach"
