"""The host rules of the region analysis (slam_toolbox_amd/csrc/map_regions_plan.hpp) on the CPU, through the stand-alone program
tests/map_regions_plan_check.cpp, built with the address and undefined-behaviour sanitizers where the compiler has them: Rc and every
refusal in order, the tile grid, the centroid cell, the record's doubles -- bit for bit against tests/map_regions_rule.py.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import map_regions_cases as cases
import map_regions_rule as rule

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_regions_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_regions_plan_check.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)                       # a compiler without the sanitizers' runtimes

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout
        return out
    return run


def hx(v):
    return float(v).hex()


GOOD = dict(rule.PARAMS)
CHECKS = [
    (dict(), 20.0, "0 0"), (dict(min_clearance=0.2), 20.0, "0 4"), (dict(min_clearance=0.21), 20.0, "0 5"), (dict(min_clearance=1e-9), 20.0, "0 1"),
    (dict(min_clearance=51.2, connectivity=4), 20.0, "0 1024"), (dict(min_clearance=-0.0), 20.0, "0 0"),
    (dict(min_region_cells=2 ** 31 - 1, max_regions=1 << 20, min_frontier_cells=7, max_frontiers=1), 4.0, "0 0"),
    (dict(min_clearance=math.nan), 20.0, "1"), (dict(min_clearance=math.inf), 20.0, "1"), (dict(min_clearance=-1e-9), 20.0, "1"),
    (dict(min_clearance=51.21), 20.0, "2"), (dict(min_clearance=1e300), 1e300, "2"),
    (dict(connectivity=0), 20.0, "3"), (dict(connectivity=6), 20.0, "3"), (dict(connectivity=-8), 20.0, "3"),
    (dict(min_region_cells=0), 20.0, "4"), (dict(min_frontier_cells=0), 20.0, "4"), (dict(min_frontier_cells=-5), 20.0, "4"),
    (dict(max_regions=0), 20.0, "5"), (dict(max_regions=(1 << 20) + 1), 20.0, "5"), (dict(max_frontiers=0), 20.0, "5"), (dict(max_frontiers=(1 << 20) + 1), 20.0, "5"),
    # the order of the refusals
    (dict(min_clearance=math.nan, connectivity=5, min_region_cells=0, max_regions=0), 20.0, "1"),
    (dict(min_clearance=99.0, connectivity=5, min_region_cells=0, max_regions=0), 20.0, "2"),
    (dict(connectivity=5, min_region_cells=0, max_regions=0), 20.0, "3"), (dict(min_frontier_cells=0, max_regions=0), 20.0, "4"),
]


def test_clearance_and_every_refusal_in_order(check):
    def line(kw, scale):
        p = dict(GOOD, **kw)
        return "check %s %s %d %d %d %d %d" % (hx(p["min_clearance"]), hx(scale), p["connectivity"], p["min_region_cells"], p["max_regions"],
                                                 p["min_frontier_cells"], p["max_frontiers"])
    reasons = {"1": "min_clearance", "2": "radius", "3": "connectivity", "4": "minimum", "5": "maximum"}
    for (kw, scale, want), got in zip(CHECKS, check([line(kw, scale) for kw, scale, _ in CHECKS])):
        assert got == want, (kw, scale)
        if want[0] == "0":
            assert rule.params_check(dict(GOOD, **kw), scale) == int(want.split()[1])
        else:
            with pytest.raises(rule.Refused) as e:
                rule.params_check(dict(GOOD, **kw), scale)
            assert str(e.value) == reasons[want], kw
    reach = [(0, 0), (0, 5), (0, 1024), (3, 3), (3, 0), (40, 39), (3, 4), (1, 1024)]
    assert check([f"reach {r} {rc}" for r, rc in reach]) == ["1", "1", "1", "1", "1", "1", "0", "0"]


def test_tile_grid(check):
    sizes = [(1, 1), (64, 16), (65, 17), (32768, 2), (2, 32768), (129, 33), (481, 574), (16384, 16384)]
    want = {(1, 1): "1 1 0 1", (64, 16): "1 1 0 16", (65, 17): "2 2 82 18", (32768, 2): "512 1 1022 1024", (2, 32768): "1 2048 4094 1024"}
    for (w, h), got in zip(sizes, check([f"grid {w} {h}" for w, h in sizes])):
        tx, ty, seams = rule.tile_grid(w, h)
        assert got == f"{tx} {ty} {seams} {(w * h + 63) // 64}", (w, h)
        assert got == want.get((w, h), got), (w, h)


def test_centroid_cell(check):
    rng = np.random.default_rng(5)
    pairs = [(0, 1), (7, 1), (1, 2), (3, 2), (5, 3), (4, 3), (2 ** 43 - 1, 2 ** 28), (2 ** 43, 2 ** 28), (2 ** 43 - 2 ** 27, 2 ** 28), (32767 * 2 ** 28, 2 ** 28)]
    pairs += [(int(s), int(n)) for s, n in zip(rng.integers(0, 2 ** 43, 20), rng.integers(1, 2 ** 28, 20))]
    for (s, n), got in zip(pairs, check([f"cell {s} {n}" for s, n in pairs])):
        assert int(got) == rule.centroid_cell(s, n) == (2 * s + n) // (2 * n), (s, n)
    assert rule.centroid_cell(1, 2) == 1 and rule.centroid_cell(4, 3) == 1 and rule.centroid_cell(5, 3) == 2, "halves go up"
    assert rule.centroid_cell(7, 1) == 7 and rule.centroid_cell(2 ** 43 - 2 ** 27, 2 ** 28) == 2 ** 15, "n = 1 is the cell itself; 32767.5 goes up"


def test_record_doubles_equal_the_rule_s(check):
    """the doubles of every record of a few cases, through the header's functions, against the rule's"""
    lines, want = [], []
    for name in ("40 x 50 random, p_occ 0.1, seed 2, N8", "100 x 40, the frontier crosses tile seams both ways, N4", "32768 x 2, sparse walls, N8"):
        case = next(c for c in cases.region_cases() if c.name == name)
        got = rule.analyse(case.view, cases.field_values(case), case.radius, **case.params)
        v = case.view
        for r in got["regions"] + got["frontiers"]:
            a = (r["anchor_cell"] % v["width"], r["anchor_cell"] // v["width"])
            for k, o, total in ((0, v["ox"], r["sum_i"]), (1, v["oy"], r["sum_j"])):
                lines.append("record %s %d %d %d %d %s" % (hx(v["anchor"][k]), o, total, r["n_cells"], a[k], hx(v["scale"])))
                want.append((r["centroid"][k], r["anchor_xy"][k]))
    assert len(lines) > 100
    for (c, a), text in zip(want, check(lines)):
        got = [float.fromhex(t) for t in text.split()]
        assert [g.hex() for g in got] == [float(c).hex(), float(a).hex()]
    big = check(["record %s %d %d %d %d %s" % (hx(-3.7), -2 ** 30, 2 ** 43 - 12345, 2 ** 28 - 1, 32767, hx(1.0 / 0.03))])[0].split()
    assert float.fromhex(big[0]).hex() == (-3.7 + (float(-2 ** 30) + float(2 ** 43 - 12345) / float(2 ** 28 - 1)) / (1.0 / 0.03)).hex()
    assert float.fromhex(big[1]).hex() == (-3.7 + float(-2 ** 30 + 32767) / (1.0 / 0.03)).hex()
