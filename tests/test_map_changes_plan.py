"""The host rules of the map change layer (slam_toolbox_amd/csrc/map_changes_plan.hpp) on the CPU, through the stand-alone program
tests/map_changes_plan_check.cpp, built with the address and undefined-behaviour sanitizers where the compiler has them: the overflow
bound at 2^32 - 1 exactly and one above, its decay, and every argument check of an observe and a diff call.  Expectations come from
tests/map_changes_rule.py and tests/map_localize_rule.py.  No GPU."""
import math
import os
import subprocess

import pytest

import map_changes_rule as rule
import map_localize_cases as cases
import map_localize_rule as ml

HERE = os.path.dirname(os.path.abspath(__file__))
TOP = 2 ** 32 - 1


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_changes_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_changes_plan_check.cpp"), "-o", exe]
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


def test_bound_at_the_top_and_one_above(check):
    cases_ = [(0, 1, 1), (0, 1, 1081), (0, 5, 130), (TOP - 2, 1, 1), (TOP - 1, 1, 1), (TOP, 1, 1), (TOP - 2 * 1081, 1, 1081), (TOP - 2 * 1081 + 1, 1, 1081),
              (1, (TOP - 1) // 2, 1), (0, (TOP - 1) // 2 + 1, 1), (0, 2 ** 31 - 1, 2 ** 31 - 1), (0, 0, 5), (0, 3, 0), (0, -1, 5), (TOP + 1, 1, 1)]
    got = [tuple(int(v) for v in line.split()) for line in check(["bound %d %d %d" % c for c in cases_])]
    for (bound, n_scans, n_beams), g in zip(cases_, got):
        try:
            want = (1, rule.bound_after(bound, n_scans, n_beams))
        except rule.Refused:
            want = (0, bound)
        if bound > TOP:
            want = (0, bound)                                  # (a bound no layer can hold)
        assert g == want, (bound, n_scans, n_beams)
    assert got[3] == (1, TOP), "2^32 - 1 exactly is taken"
    assert got[4] == (0, TOP - 1), "one above is refused"
    assert got[6] == (1, TOP) and got[7][0] == 0 and got[8] == (1, TOP) and got[9][0] == 0


def test_decay_shifts_the_bound(check):
    cases_ = [(TOP, 1), (TOP, 31), (12345, 3), (1, 1), (0, 5), (TOP, 0), (TOP, 32), (TOP, -1)]
    got = [tuple(int(v) for v in line.split()) for line in check(["decay %d %d" % c for c in cases_])]
    assert got == [(1, b >> s) if 1 <= s <= 31 else (0, b) for b, s in cases_]


def test_observe_arguments(check):
    good = dict(nulls=0, n_beams=8, rt=12.0, lo=0.1, hi=30.0, a0=-1.0, da=0.25, n=2, t=1, poses=[1.0, 2.0, 0.3, 1.5, 2.5, -0.2])

    def line(**kw):
        c = dict(good, **kw)
        return " ".join(["args", str(c["nulls"]), str(c["n_beams"]), hx(c["rt"]), hx(c["lo"]), hx(c["hi"]), hx(c["a0"]), hx(c["da"]), str(c["n"]),
                         str(c["t"])] + [hx(v) for v in c["poses"][:3 * max(c["n"], 0)]])
    taken = [dict(), dict(t=0), dict(t=4), dict(n=1), dict(lo=-math.inf), dict(hi=math.inf)]
    refused = [dict(nulls=1), dict(nulls=2), dict(nulls=4), dict(n=0), dict(n=-1), dict(n_beams=0), dict(t=-1), dict(t=5), dict(rt=math.inf),
               dict(rt=0.0), dict(rt=math.nan), dict(lo=math.nan), dict(hi=math.nan), dict(a0=math.nan), dict(da=math.inf)]
    for k, bad in ((0, math.nan), (1, math.inf), (2, math.nan), (4, -math.inf), (5, math.nan)):
        poses = list(good["poses"])
        poses[k] = bad
        refused.append(dict(poses=poses))
    got = check([line(**kw) for kw in taken + refused])
    assert got == ["1"] * len(taken) + ["0"] * len(refused)


def test_observe_walk_is_the_fit_rule(check):
    """what kh_map_fit refuses for the length of a walk, kh_map_changes_observe refuses: tests/map_localize_rule.fit_refused"""
    view = dict(anchor=(0.5, -0.25), scale=20.0)
    lasers = [cases.circle(1), cases.circle(1, range_threshold=(2 ** 20 - 1) / 20.0, max_range=1e9), cases.circle(1, range_threshold=(2 ** 20 - 2) / 20.0, max_range=1e9)]
    poses = [(1.0, 2.0, 0.3), (2.0 ** 30 / 20.0 + 0.5, 0.0, 0.0), (2.0 ** 30 / 20.0 + 0.6, 0.0, 0.0), (0.0, -1e12, 0.0), (0.0, -(2.0 ** 30 / 20.0 + 1.0), 0.0)]
    lines, want = [], []
    for laser in lasers:
        for pose in poses:
            lines.append(" ".join(["walk", hx(laser.range_threshold), hx(laser.min_range), hx(laser.max_range), hx(20.0), hx(0.5), hx(-0.25), "2"] +
                                  [hx(v) for v in poses[0] + pose]))
            laser_bad = ml.fit_refused(view, laser, poses[0])
            want.append("1" if laser_bad else "2" if ml.fit_refused(view, laser, pose) else "0")
    assert check(lines) == want
    assert set(want) == {"0", "1", "2"}


def test_diff_arguments(check):
    cases_ = [(0.1, 0, 0, 1, 1), (0.1, 5, 1, 1, 1), (math.inf, 5, 1, 1, 1), (0.1, 5, 0, 1, 0), (0.1, -1, 1, 1, 0), (0.1, 0, 0, 0, 0), (math.nan, 0, 0, 1, 0)]
    got = check(["diffargs %s %d %d %d" % (hx(t), cap, cells, out) for t, cap, cells, out, _ in cases_])
    assert got == [str(c[4]) for c in cases_]
