"""The host rules of the map merge (slam_toolbox_amd/csrc/map_merge_plan.hpp) on the CPU, through the stand-alone program
tests/map_merge_plan_check.cpp, built with the address and undefined-behaviour sanitizers where the compiler has them: the sample
offsets, the default footprint, the inverse correction, the output window with its three refusals, the derived agreement, the argument
check -- bit for bit against tests/map_merge_rule.py.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import map_merge_rule as rule
import merge_rule

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_merge_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_merge_plan_check.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)                       # a compiler without the sanitizers' runtimes

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout
        return out
    return run


def hexes(line):
    return [float.fromhex(t) for t in line.split()]


def same_bits(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


def test_sample_offsets(check):
    cases = [(n, scale) for n in (1, 2, 3, 4) for scale in (20.0, 1.0, 3.0, 1.0 / 0.03, 40.0)]
    for (n, scale), text in zip(cases, check(["offsets %d %s" % (n, float(scale).hex()) for n, scale in cases])):
        assert same_bits(hexes(text), rule.sample_offsets(n, scale)), (n, scale)
    assert rule.sample_offsets(1, 20.0) == [0.0] and rule.sample_offsets(2, 20.0) == [-0.25 / 20.0, 0.25 / 20.0]
    assert rule.sample_offsets(4, 1.0) == [-0.375, -0.125, 0.125, 0.375], "the centres of n equal parts of the cell"


def test_default_footprint(check):
    cases = [(10.0, 20.0, 1), (20.0, 20.0, 1), (40.0, 20.0, 2), (50.0, 20.0, 3), (160.0, 20.0, 4), (20.0 * (1 + 2 ** -52), 20.0, 2), (1e300, 1e-300, 4)]
    out = check(["footprint %s %s" % (float(m).hex(), float(t).hex()) for m, t, _ in cases])
    for (m, t, want), text in zip(cases, out):
        assert int(text) == rule.default_footprint(m, t) == want, (m, t)


def test_inverse_correction(check):
    rng = np.random.default_rng(31)
    cs = [rng.uniform(-20, 20, 3) * [1, 1, 0.15] for _ in range(30)] + [np.array([0.73, -0.41, 0.3]), np.zeros(3), np.array([1.0, 2.0, math.pi]),
                                                                         np.array([1.0, 2.0, -math.pi])]
    for c, text in zip(cs, check(["inverse " + " ".join(float(v).hex() for v in c) for c in cs])):
        inv = merge_rule.inverse(c)
        assert same_bits(hexes(text), [*inv, *merge_rule.cos_sin(inv[2])]), c


def views(tox=0, toy=0, tw=20, th=10, ta=(0.5, -0.25), ts=20.0, ma=(-1.0, 2.0), ms=20.0):
    return (dict(ox=tox, oy=toy, width=tw, height=th, anchor=ta, scale=ts), dict(anchor=ma, scale=ms))


WINDOWS = [
    ("an empty box", views(), None, (0.3, 0.2, 0.1), 1),
    ("a one-cell box", views(), (4, 5, 4, 5), (0.0, 0.0, 0.0), 1),
    ("a one-cell box far off", views(), (400, -500, 400, -500), (0.25, 0.5, 0.0), 1),
    ("the first quadrant", views(), (0, 0, 30, 12), (1.0, 0.5, 0.3), 1),
    ("the second quadrant", views(), (0, 0, 30, 12), (1.0, 0.5, 2.0), 1),
    ("the third quadrant", views(), (0, 0, 30, 12), (1.0, 0.5, -3.0), 1),
    ("the fourth quadrant", views(), (0, 0, 30, 12), (1.0, 0.5, -1.0), 1),
    ("a quarter turn", views(), (0, 0, 30, 12), (0.0, 0.0, math.pi / 2), 1),
    ("just below half a turn", views(), (0, 0, 30, 12), (0.0, 0.0, float(np.nextafter(math.pi, 0.0))), 1),
    ("negative origins", views(tox=-40, toy=-25, tw=33, th=17), (-70, -12, -31, 9), (0.2, -0.1, 0.7), 1),
    ("the window grows on the low side", views(), (0, 0, 9, 9), (-7.0, -5.0, 0.0), 1),
    ("the same, not grown", views(), (0, 0, 9, 9), (-7.0, -5.0, 0.0), 0),
    ("half-cell ties of the corners", views(ta=(0.0, 0.0), ts=4.0, ma=(0.0, 0.0), ms=4.0), (-3, -2, 5, 6), (0.0, 0.0, 0.0), 1),
    ("a finer moving map", views(ms=40.0), (10, 10, 90, 50), (0.4, 0.3, -0.2), 1),
    ("a coarser moving map", views(ms=10.0), (1, 1, 9, 5), (0.4, 0.3, 0.2), 1),
    ("a corner exactly 2^30 cells off", views(ta=(0.0, 0.0), ts=1.0, ma=(0.0, 0.0), ms=1.0, tox=2 ** 30 - 8, tw=8, th=1), (0, 0, 0, 0), (2.0 ** 30 - 0.5, 0.0, 0.0), 1),
    ("REFUSED: a corner beyond 2^30 cells", views(ta=(0.0, 0.0), ts=1.0, ma=(0.0, 0.0), ms=1.0), (0, 0, 0, 0), (2.0 ** 30 + 1.0, 0.0, 0.0), 1),
    ("REFUSED: a correction of 1e12 m", views(), (0, 0, 3, 3), (1e12, 0.0, 0.0), 1),
    ("REFUSED: 1e12 m along -y", views(), (0, 0, 3, 3), (0.0, -1e12, 0.3), 1),
    ("not refused when the window does not grow", views(), (0, 0, 3, 3), (1e12, 0.0, 0.0), 0),
    ("a side of exactly 32768 cells", views(tw=8, th=4), (0, 0, 0, 0), (32765.7 / 20.0 + 1.5, 2.26, 0.0), 1),
    ("REFUSED: a side of 32769 cells", views(tw=8, th=4), (0, 0, 0, 0), (32766.7 / 20.0 + 1.5, 2.26, 0.0), 1),
    ("REFUSED: the target's own side", views(tw=32769, th=1), None, (0.0, 0.0, 0.0), 0),
    ("exactly 2^28 cells", views(tw=32768, th=8192), None, (0.0, 0.0, 0.0), 1),
    ("REFUSED: above 2^28 cells", views(tw=32768, th=8193), None, (0.0, 0.0, 0.0), 0),
    ("REFUSED: grown above 2^28 cells", views(tw=32768, th=8190), (0, 8200, 0, 8200), (3.0, -2.26, 0.0), 1),
]


def test_output_windows(check):
    lines, wants = [], []
    for name, (target, moving), box, c, grow in WINDOWS:
        b = box if box is not None else (0, 0, -1, -1)
        lines.append("window %d %d %d %d %s %s %s %s %s %s %d %d %d %d %s %s %s %d" % (
            target["ox"], target["oy"], target["width"], target["height"], *(float(v).hex() for v in (*target["anchor"], target["scale"])),
            *(float(v).hex() for v in (*moving["anchor"], moving["scale"])), *b, *(float(v).hex() for v in c), grow))
        try:
            wants.append("0 %d %d %d %d %d" % tuple(rule.output_window(target, moving, c, grow, box)))
        except rule.Refused as e:
            wants.append(str(e.code))
        assert wants[-1][0] != "0" if name.startswith("REFUSED") else wants[-1][0] == "0", name
    got = check(lines)
    for (name, *_), g, w in zip(WINDOWS, got, wants):
        assert g == w, (name, g, w)
    by_name = dict(zip((w[0] for w in WINDOWS), got))
    assert by_name["an empty box"] == by_name["the same, not grown"] == "0 0 0 20 10 24", "the target's window"
    # cell (4, 5) of the moving lattice is cell (-26, 50) of the target's: its corners round to -27 and 51, one cell of padding beyond them
    assert by_name["a one-cell box"] == "0 -28 0 48 53 48"
    low = [int(t) for t in by_name["the window grows on the low side"].split()]
    assert low[1] < 0 and low[2] < 0 and low[1] + low[3] == 20 and low[2] + low[4] == 10
    assert by_name["REFUSED: a corner beyond 2^30 cells"] == by_name["REFUSED: a correction of 1e12 m"] == "1"
    assert by_name["REFUSED: a side of 32769 cells"] == by_name["REFUSED: the target's own side"] == "2"
    assert by_name["REFUSED: above 2^28 cells"] == by_name["REFUSED: grown above 2^28 cells"] == "3"
    assert by_name["a side of exactly 32768 cells"].split()[3] == "32768" and by_name["exactly 2^28 cells"] == "0 0 0 32768 8192 32768"


def test_agreement(check):
    cases = [(0, 0, 0, 0, 0, 0), (5, 7, 0, 0, 0, 0), (1, 2, 3, 4, 5, 6), (0, 0, 2, 1, 0, 0), (9, 9, 1, 0, 1, 1), (3, 3392, 90000, 7000, 200, 133),
             (0, 0, 2 ** 53 + 1, 2 ** 53 + 1, 1, 0), (0, 0, 1, 0, 2 ** 63, 0)]
    for c, text in zip(cases, check(["agreement " + " ".join(str(v) for v in c) for c in cases])):
        overlap, value = text.split()
        assert int(overlap) == sum(c[2:]) and same_bits([float.fromhex(value)], [rule.agreement(c[2], c[3], sum(c[2:]))]), c
    assert rule.agreement(0, 0, 0) == 0.0 and rule.agreement(2, 1, 3) == 1.0 and rule.agreement(1, 0, 3) == 1.0 / 3.0


def test_argument_check(check):
    good = dict(c=(0.73, -0.41, 0.3), footprint=0, conflict=2, grow=1)
    bad = [dict(c=(math.nan, 0.0, 0.0)), dict(c=(0.0, math.inf, 0.0)), dict(c=(0.0, 0.0, -math.inf)), dict(c=(0.0, 0.0, math.nan)), dict(footprint=-1),
           dict(footprint=5), dict(conflict=-1), dict(conflict=4), dict(grow=-1), dict(grow=2)]
    fine = [dict(), dict(footprint=1), dict(footprint=4), dict(conflict=0), dict(conflict=3), dict(grow=0), dict(c=(1e12, -1e12, 700.0))]

    def line(kw):
        a = dict(good, **kw)
        return "args %s %s %s %d %d %d" % (*(float(v).hex() for v in a["c"]), a["footprint"], a["conflict"], a["grow"])
    assert check([line(kw) for kw in bad]) == ["0"] * len(bad)
    assert check([line(kw) for kw in fine]) == ["1"] * len(fine)
    one = dict(cells=np.zeros((1, 8), dtype=np.uint8), ox=0, oy=0, width=1, height=1, anchor=(0.0, 0.0), scale=20.0)
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(rule.Refused):
            rule.merge(one, one, a["c"], a["footprint"], a["conflict"], a["grow"])
    assert rule.merge(one, one, good["c"]).window == rule.Window(0, 0, 1, 1, 8)
