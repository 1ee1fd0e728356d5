"""The host rules of the ray cast and the map alignment (slam_toolbox_amd/csrc/map_align_plan.hpp, RayWalk of
csrc/occupancy_device.hpp) on the CPU, through the stand-alone program tests/map_align_plan_check.cpp, built with the address and
undefined-behaviour sanitizers where the compiler has them: the outward walk of every short line against TraceLine, the default
no-return reading, probe picking with ties, corrections and candidate poses bit for bit, the ranking with ties, the argument check.
Expectations come from tests/map_raycast_rule.py, tests/map_align_rule.py and tests/merge_rule.py.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import map_align_rule as rule
import map_raycast_rule as cast_rule
import merge_fit_rule as fr
import merge_rule
import occupancy_cases as oc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_align_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_align_plan_check.cpp"), "-o", exe]
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


def test_outward_walk_is_trace_line(check):
    """every line of up to 9 cells from two start cells, and longer ones: the device's walk visits TraceLine's cells, outward"""
    rng = np.random.default_rng(5)
    lines = [(x0, y0, x0 + dx, y0 + dy) for x0, y0 in ((0, 0), (-7, 3)) for dx in range(-9, 10) for dy in range(-9, 10)]
    lines += [tuple(int(v) for v in rng.integers(-400, 400, size=4)) for _ in range(300)]
    lines += [(2 ** 30, -2 ** 30, 2 ** 30 - 2 ** 15, -2 ** 30 + 777), (-2 ** 30, 5, -2 ** 30 + 12, 5 - 2 ** 15)]      # at the edge of the lattice
    out = check(["walk %d %d %d %d" % line for line in lines])
    swapped_ties = 0
    for line, text in zip(lines, out):
        got = [tuple(int(v) for v in cell.split(",")) for cell in text.split()]
        x, y = cast_rule.beam_cells(line[:2], line[2:])
        assert got == list(zip(x.tolist(), y.tolist())), line
        if max(abs(line[2] - line[0]), abs(line[3] - line[1])) <= 400:
            want = oc.bresenham(*line)
            assert got in (want, want[::-1]), line
            mirrored = [(line[0] + line[2] - i, line[1] + line[3] - j) for i, j in want]
            swapped_ties += got == want[::-1] and got != want and sorted(mirrored) != sorted(want)
    assert swapped_ties > 50, "lines that TraceLine walks from the far end and whose mirror image is another set of cells"


def test_default_no_return(check):
    cases = [(12.0, 30.0), (5.0, 5.0), (5.0, float(np.nextafter(5.0, np.inf))), (5.0, float(np.nextafter(np.nextafter(5.0, np.inf), np.inf))), (20.0, 20.5)]
    out = check(["noreturn %r %r" % c for c in cases])
    Laser = type("Laser", (), {})
    for (threshold, max_range), text in zip(cases, out):
        laser = Laser()
        laser.range_threshold, laser.max_range = threshold, max_range
        want = cast_rule.default_no_return(laser)
        got = float.fromhex(text) if "nan" not in text else math.nan
        assert (math.isnan(got) and math.isnan(want)) or got == want, (threshold, max_range)
    assert math.isnan(float.fromhex(out[1]) if "nan" not in out[1] else math.nan) and float.fromhex(out[3]) == np.nextafter(5.0, np.inf)


def test_probe_picking(check):
    cases = [(3, [5, 9, 9, 0, 7, 9]), (2, [0, 0, 0]), (3, [4]), (1, [3, 3]), (4, [1, 2, 3, 4, 5, 6]), (3, [7, 0, 7, 0, 7, 7]), (2, [])]
    out = check(["probes %d %s" % (n, " ".join(map(str, hits))) for n, hits in cases])
    for (n, hits), text in zip(cases, out):
        assert [int(t) for t in text.split()] == rule.pick_probes(hits, n), (n, hits)
    assert out[0].split() == ["1", "2", "5"] and out[1].split() == [] and out[5].split() == ["0", "2", "4"]


def test_corrections_and_candidate_poses(check):
    rng = np.random.default_rng(17)
    pairs = [(rng.uniform(-20, 20, 3) * [1, 1, 0.15], rng.uniform(-20, 20, 3) * [1, 1, 0.15]) for _ in range(40)]
    pairs += [(np.array([1.0, 2.0, 3.1]), np.array([0.5, -4.0, -3.1])), (np.zeros(3), np.zeros(3)), (np.array([3.0, 4.0, 0.0]), np.array([3.0, 4.0, 0.0]))]
    args = lambda a, b: " ".join(float(v).hex() for v in (*a, *b))      # noqa: E731
    got = check(["correction " + args(p, q) for p, q in pairs])
    for (p, q), text in zip(pairs, got):
        assert same_bits(hexes(text), rule.correction(p, q)), (p, q)
    got = check(["pose " + args(c, s) for c, s in pairs])
    for (c, s), text in zip(pairs, got):
        assert same_bits(hexes(text), merge_rule.transform_pose(c, s)), (c, s)
    # a probe found where it stands: the identity, up to the rounding of one rotation
    assert np.abs(rule.correction(pairs[0][0], pairs[0][0])).max() < 1e-12


def test_ranking_with_ties(check):
    counter = lambda agree_free, conflict_occ, hits_occ=0: [0, conflict_occ + 2 * hits_occ, agree_free, 0, hits_occ, 0]      # noqa: E731
    sets = [
        (0, [counter(90, 10), counter(99, 1), counter(99, 1), counter(198, 2), counter(0, 0)]),      # equal scores: agree, then index
        (150, [counter(90, 10), counter(99, 1), counter(198, 2), counter(0, 0)]),                    # too few known visits rank last
        (0, [counter(0, 0), counter(0, 0)]),
        (1, [counter(5, 5, 3), counter(8, 2), counter(8, 5, 3)]),
    ]
    out = check(["rank %d %d %s" % (min_known, len(c), " ".join(str(v) for one in c for v in one)) for min_known, c in sets])
    for (min_known, cs), text in zip(sets, out):
        fits = [fr.derive(dict(zip(fr.COUNTERS, c))) for c in cs]
        want = fr.ranking(fits, min_known)
        got = [t.split(":") for t in text.split()]
        assert [int(g[0]) for g in got] == want, (min_known, cs)
        assert [int(g[1]) for g in got] == [int(fits[i]["known"] >= min_known) for i in want]
        assert same_bits([float.fromhex(g[2]) for g in got], [fits[i]["score"] for i in want])
    assert [t.split(":")[0] for t in out[0].split()] == ["3", "1", "2", "0", "4"]
    assert [t.split(":")[0] for t in out[1].split()] == ["2", "1", "0", "3"]


def test_argument_check(check):
    good = dict(probe_spacing=2.0, n_probes=3, top_k=4, max_unknown=20, initial=(0.0, 0.0, 0.0), seed_spacing=1.0, n_headings=0)
    bad = [dict(probe_spacing=0.0), dict(probe_spacing=-1.0), dict(probe_spacing=math.inf), dict(probe_spacing=math.nan), dict(n_probes=0),
           dict(top_k=0), dict(max_unknown=-2), dict(initial=(math.nan, 0.0, 0.0)), dict(initial=(0.0, math.inf, 0.0)), dict(initial=(0.0, 0.0, math.nan)),
           dict(seed_spacing=0.0), dict(n_headings=4097)]
    fine = [dict(), dict(max_unknown=-1), dict(max_unknown=0), dict(n_probes=1, top_k=1), dict(initial=(1e9, -1e9, 7.0)), dict(n_headings=4096)]

    def line(kw):
        a = dict(good, **kw)
        return "args %r %d %d %d %r %r %r %r %d" % (a["probe_spacing"], a["n_probes"], a["top_k"], a["max_unknown"], *a["initial"], a["seed_spacing"],
                                                   a["n_headings"])
    assert check([line(kw) for kw in bad]) == ["0"] * len(bad)
    assert check([line(kw) for kw in fine]) == ["1"] * len(fine)
