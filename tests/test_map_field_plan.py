"""The host rules of the distance field (slam_toolbox_amd/csrc/map_field_plan.hpp) on the CPU, through the stand-alone program
tests/map_field_plan_check.cpp, built with the address and undefined-behaviour sanitizers where the compiler has them: the radius and
the limits with every refusal, the cost table, the truncation and the derived score, the refinement's candidate order, tie rule and
state machine -- bit for bit against tests/map_field_rule.py.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import map_field_rule as rule

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_field_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_field_plan_check.cpp"), "-o", exe]
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


def test_radius(check):
    cases = [(2.0, 20.0, 40), (0.0, 20.0, 0), (0.55, 20.0, 11), (0.55, 4.0, 3), (1.0, 1.0 / 0.03, 34), (51.2, 20.0, 1024), (51.21, 20.0, -1),
             (1e-9, 20.0, 1), (-0.0, 20.0, 0), (-1e-9, 20.0, -1), (math.nan, 20.0, -1), (math.inf, 20.0, -1), (1e300, 1e300, -1)]
    for (m, k, want), text in zip(cases, check([f"radius {hx(m)} {hx(k)}" for m, k, _ in cases])):
        assert int(text) == want, (m, k)
        if want >= 0:
            assert rule.radius_cells(m, k) == want
        else:
            with pytest.raises(rule.Refused):
                rule.radius_cells(m, k)


FIELDS = [
    ((20, 10, 20.0, 2.0, 0), "0 40 20"), ((13, 7, 4.0, 0.0, 1), "0 0 16"), ((1, 1, 4.0, 0.25, 0), "0 1 4"),
    ((32768, 8192, 20.0, 2.0, 0), "0 40 32768"), ((4096, 4096, 20.0, 0.0, 0), "0 0 4096"), ((8, 8, 20.0, 51.2, 0), "0 1024 8"),
    ((8, 8, 20.0, 51.3, 0), "1"), ((8, 8, 20.0, -1.0, 0), "1"), ((8, 8, 20.0, math.nan, 0), "1"), ((8, 8, 20.0, math.inf, 0), "1"),
    ((8, 8, 20.0, 2.0, -1), "2"), ((8, 8, 20.0, 2.0, 2), "2"),
    ((32769, 1, 20.0, 2.0, 0), "3"), ((1, 32769, 20.0, 2.0, 0), "3"),
    ((32768, 8193, 20.0, 2.0, 0), "4"),
    ((4097, 1, 20.0, 0.0, 0), "5"), ((1, 4097, 20.0, 0.0, 0), "5"),
    ((32769, 1, 20.0, math.nan, 5), "1"),                      # the order of the refusals
]


def test_limits_and_every_refusal(check):
    out = check(["field %d %d %s %s %d" % (w, h, hx(k), hx(m), o) for (w, h, k, m, o), _ in FIELDS])
    for ((w, h, k, m, o), want), got in zip(FIELDS, out):
        assert got == want, (w, h, k, m, o)
        if want[0] == "0":
            assert rule.field_check(w, h, k, m, o) == int(want.split()[1])
        else:
            with pytest.raises(rule.Refused):
                rule.field_check(w, h, k, m, o)


TABLES = [dict(scale=20.0), dict(scale=20.0, inscribed_radius=0.4, inflation_radius=0.4), dict(scale=20.0, cost_scaling_factor=0.0),
          dict(scale=1.0 / 0.03, inscribed_radius=0.1, inflation_radius=0.8, cost_scaling_factor=3.0), dict(scale=4.0, inscribed_radius=0.0, inflation_radius=2.5, cost_scaling_factor=1.3)]
BAD_TABLES = [dict(scale=20.0, inscribed_radius=0.6), dict(scale=20.0, inscribed_radius=-0.1), dict(scale=20.0, inflation_radius=math.nan),
              dict(scale=20.0, inflation_radius=math.inf), dict(scale=20.0, cost_scaling_factor=-1.0), dict(scale=20.0, cost_scaling_factor=math.inf),
              dict(scale=20.0, inflation_radius=51.3), dict(scale=20.0, track_unknown=2), dict(scale=20.0, inflate_unknown=-1), dict(scale=0.0),
              dict(scale=math.nan), dict(scale=20.0, inscribed_radius=math.nan)]


def table_line(kw):
    p = dict(rule.INFLATION, **{k: v for k, v in kw.items() if k != "scale"})
    return "table %s %s %s %d %d %s" % (hx(p["inscribed_radius"]), hx(p["inflation_radius"]), hx(p["cost_scaling_factor"]), p["track_unknown"],
                                        p["inflate_unknown"], hx(kw["scale"]))


def test_cost_tables_equal_the_rule(check):
    for kw, text in zip(TABLES, check([table_line(kw) for kw in TABLES])):
        got = [int(t) for t in text.split()]
        want = rule.cost_table(**kw)
        assert got[0] == want.size and got[1:] == want.tolist(), kw
    assert check([table_line(kw) for kw in BAD_TABLES]) == ["-1"] * len(BAD_TABLES)
    for kw in BAD_TABLES:
        with pytest.raises(rule.Refused):
            rule.cost_table(**kw)
    t = rule.cost_table(20.0)
    # 0.22 m are 4.4 cells: d2 = 19 is the last inscribed entry; 0.55 m are 11 cells: d2 = 121 is the last entry
    assert t.size == 122 and t[0] == 254 and t[1] == t[19] == 253 and t[20] == int(252.0 * math.exp(-10.0 * (math.sqrt(20.0) / 20.0 - 0.22))) == 243
    assert t[121] == int(252.0 * math.exp(-10.0 * (0.55 - 0.22))) == 9
    same = rule.cost_table(20.0, inscribed_radius=0.4, inflation_radius=0.4)
    assert same.size == 65 and set(same.tolist()) == {254, 253}, "inscribed == inflation: no decay branch within the radius"
    flat = rule.cost_table(20.0, cost_scaling_factor=0.0)
    assert set(flat[20:].tolist()) == {252} and flat[19] == 253


def test_truncation_and_derived_score(check):
    cases = [(0, 40, 40), (7, 40, 7), (7, 0, 7), (0, 0, -1), (-1, 40, -1), (1025, 40, -1), (1024, 0, 1024)]
    for (t, r, want), text in zip(cases, check([f"truncation {t} {r}" for t, r, _ in cases])):
        assert int(text) == want
        if want > 0:
            assert rule.truncation(t, r) == want
        else:
            with pytest.raises(rule.Refused):
                rule.truncation(t, r)
    sums = [(10, 8, 7, 5, 123, 11), (0, 0, 0, 0, 0, 5), (1081, 1081, 1081, 1081, 0, 40), (1081, 1000, 0, 0, 0, 1024), (3, 3, 3, 3, 3 * 1024 ** 2, 1024)]
    for c, text in zip(sums, check(["derive " + " ".join(str(v) for v in c) for c in sums])):
        cost, score = text.split()[:2]
        t2 = c[5] ** 2
        want_cost = c[4] + (c[1] - c[3]) * t2
        want_score = 1.0 - float(want_cost) / (float(c[1]) * float(t2)) if c[1] else 0.0
        assert int(cost) == want_cost and float.fromhex(score).hex() == want_score.hex(), c
        assert [int(v) for v in text.split()[2:]] == list(c[:5])


def test_refine_arguments(check):
    good = dict(step_xy=0.1, step_heading=0.02, n_halvings=4, max_rounds=64, truncate_cells=0)
    bad = [dict(step_xy=0.0), dict(step_xy=-1.0), dict(step_xy=math.nan), dict(step_xy=math.inf), dict(step_heading=-0.1), dict(step_heading=math.nan),
           dict(n_halvings=-1), dict(n_halvings=33), dict(max_rounds=0), dict(max_rounds=4097), dict(truncate_cells=-1), dict(truncate_cells=1025)]
    fine = [dict(), dict(step_heading=0.0), dict(n_halvings=0), dict(n_halvings=32), dict(max_rounds=1), dict(max_rounds=4096), dict(truncate_cells=1024)]

    def line(kw):
        p = dict(good, **kw)
        return "refine_args %s %s %d %d %d" % (hx(p["step_xy"]), hx(p["step_heading"]), p["n_halvings"], p["max_rounds"], p["truncate_cells"])
    assert check([line(kw) for kw in bad]) == ["0"] * len(bad)
    assert check([line(kw) for kw in fine]) == ["1"] * len(fine)
    for kw in bad:
        with pytest.raises(rule.Refused):
            rule.refine_params_check(dict(good, **kw))
    for kw in fine:
        rule.refine_params_check(dict(good, **kw))


def test_candidate_order(check):
    rng = np.random.default_rng(3)
    cases = [(*rng.uniform(-30, 30, 3), 0.1, 0.02) for _ in range(5)] + [(1.0, 2.0, 3.0, 0.1 / 16, 0.02 / 16), (-0.0, 0.0, -3.2, 0.05, 0.0), (0.1, 0.2, 0.3, 1e-300, 1e300)]
    for case, text in zip(cases, check(["candidates " + " ".join(hx(v) for v in c) for c in cases])):
        got = [float.fromhex(t) for t in text.split()]
        want = [v for c in range(27) for v in rule.candidate(case[:3], case[3], case[4], c)]
        assert [g.hex() for g in got] == [w.hex() for w in want], case
    x, y, h, s, a = 1.0, 2.0, 3.0, 0.5, 0.25
    assert rule.candidate((x, y, h), s, a, 13) == (x, y, h) and rule.candidate((x, y, h), s, a, 0) == (x - s, y - s, h - a)
    assert rule.candidate((x, y, h), s, a, 5) == (x + s, y, h - a) and rule.candidate((x, y, h), s, a, 26) == (x + s, y + s, h + a)


def test_tie_rule(check):
    flat = [5] * 27
    cases = [(flat, 13), ([5] * 13 + [6] + [5] * 13, 0), ([9] * 27, 13), (list(range(27)), 0), (list(range(27, 0, -1)), 26),
             ([7] * 4 + [3] + [7] * 8 + [3] + [7] * 13, 13), ([7] * 4 + [3] + [7] * 8 + [4] + [7] * 6 + [3] + [7] * 6, 4), ([2 ** 63] * 26 + [2 ** 63 - 1], 26)]
    for (costs, want), text in zip(cases, check(["pick " + " ".join(str(v) for v in c) for c, _ in cases])):
        assert len(costs) == 27 and int(text) == rule.pick(costs) == want, costs


def scripted(target):
    def cost(p):
        return int(math.floor(64.0 * abs(p[0] - target[0]) + 0.5) + math.floor(64.0 * abs(p[1] - target[1]) + 0.5) + math.floor(1024.0 * abs(p[2] - target[2]) + 0.5)), 5
    return cost


MACHINES = [
    ("converges on the target", (0.0, 0.0, 0.0), dict(step_xy=0.25, step_heading=0.0625, n_halvings=4, max_rounds=64), (1.0, -0.75, 0.125), 4.0, rule.CONVERGED),
    ("already there", (1.0, -0.75, 0.125), dict(step_xy=0.25, step_heading=0.0625, n_halvings=2, max_rounds=64), (1.0, -0.75, 0.125), 4.0, rule.CONVERGED),
    ("no halvings", (0.0, 0.0, 0.0), dict(step_xy=0.25, step_heading=0.0625, n_halvings=0, max_rounds=64), (1.0, -0.75, 0.125), 4.0, rule.CONVERGED),
    ("two rounds only", (0.0, 0.0, 0.0), dict(step_xy=0.25, step_heading=0.0625, n_halvings=4, max_rounds=2), (5.0, 5.0, 0.0), 4.0, rule.MAX_ROUNDS),
    ("the last round converges", (0.0, 0.0, 0.0), dict(step_xy=0.25, step_heading=0.0625, n_halvings=0, max_rounds=1), (0.0, 0.0, 0.0), 4.0, rule.CONVERGED),
    ("the last round halves", (0.0, 0.0, 0.0), dict(step_xy=0.25, step_heading=0.0625, n_halvings=1, max_rounds=1), (0.0, 0.0, 0.0), 4.0, rule.MAX_ROUNDS),
    ("walks off the lattice", (2.0 ** 28 - 1.0, 0.0, 0.0), dict(step_xy=0.5, step_heading=0.0, n_halvings=4, max_rounds=64), (2.0 ** 29, 0.0, 0.0), 4.0, rule.LEFT_LATTICE),
    ("starts at the edge", (2.0 ** 28, 0.0, 0.0), dict(step_xy=0.5, step_heading=0.0, n_halvings=4, max_rounds=64), (0.0, 0.0, 0.0), 4.0, rule.LEFT_LATTICE),
    ("an irrational step", (0.3, 0.1, -0.2), dict(step_xy=0.1, step_heading=0.02, n_halvings=4, max_rounds=64), (0.77, -0.41, 0.013), 20.0, rule.CONVERGED),
]


def test_state_machine_with_a_scripted_cost(check):
    lines = ["machine %s %s %s %s %s %d %d %s %s %s %s" % (*(hx(v) for v in start), hx(p["step_xy"]), hx(p["step_heading"]), p["n_halvings"], p["max_rounds"],
                                                         *(hx(v) for v in target), hx(scale)) for _, start, p, target, scale, _ in MACHINES]
    from collections import namedtuple
    Laser = namedtuple("Laser", "range_threshold")
    for (name, start, p, target, scale, status), text in zip(MACHINES, check(lines)):
        view = dict(anchor=(0.0, 0.0), scale=scale)
        want = rule.refine_with(scripted(target), lambda q, view=view: rule.ml.fit_refused(view, Laser(12.0), q), start, p)
        t = text.split()
        got_pose = [float.fromhex(v) for v in t[:3]]
        assert [v.hex() for v in got_pose] == [float(v).hex() for v in want.pose], name
        assert [int(v) for v in t[3:]] == [want.cost_start, want.cost, want.n_hit, want.rounds, want.halvings, want.status], (name, text, want)
        assert want.status == status, (name, want)
    by_name = {m[0]: rule.refine_with(scripted(m[3]), lambda q: False, m[1], m[2]) for m in MACHINES[:6]}
    assert by_name["converges on the target"].pose.tolist() == [1.0, -0.75, 0.125] and by_name["converges on the target"].cost == 0
    assert (by_name["already there"].rounds, by_name["already there"].halvings) == (3, 2)
    assert by_name["two rounds only"].rounds == 2 and by_name["two rounds only"].pose.tolist() == [0.5, 0.5, 0.0]
    assert by_name["the last round halves"].halvings == 1 and by_name["the last round converges"].rounds == 1
