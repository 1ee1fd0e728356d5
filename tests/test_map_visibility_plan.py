"""The host rules of the visibility analysis (slam_toolbox_amd/csrc/map_visibility_plan.hpp) on the CPU, through the stand-alone program
tests/map_visibility_plan_check.cpp, built with the address and undefined-behaviour sanitizers where the compiler has them: every
refusal in order, the reach at ranges on, just below and just above a cell count, reach 511 taken and 512 refused, the bitmap's bytes,
the select bounds, the mask's words, what counts as the same window -- against tests/map_visibility_rule.py.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import map_localize_cases as lc
import map_visibility_rule as rule

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "map_visibility_plan_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "map_visibility_plan_check.cpp"), "-o", exe]
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


VIEW = dict(width=60, height=50, width_step=64, ox=-3, oy=4, anchor_x=0.5, anchor_y=-0.25, scale=4.0)
LASER = dict(n_beams=16, min_angle=-math.pi, ang_res=math.pi / 8, min_range=0.1, max_range=7.5, range_threshold=5.0)
PARAMS = dict(rule.PARAMS)
REASONS = {2: "view", 3: "laser", 4: "max_unknown", 5: "weights", 6: "reach"}


def create_line(nulls=0, **kw):
    v, l, p = dict(VIEW), dict(LASER), dict(PARAMS)
    for k, value in kw.items():
        next(d for d in (v, l, p) if k in d)[k] = value
    return "create %d %d %d %d %d %d %s %s %s %d %s %s %s %s %s %d %d %d %d" % (
        nulls, v["width"], v["height"], v["width_step"], v["ox"], v["oy"], hx(v["anchor_x"]), hx(v["anchor_y"]), hx(v["scale"]), l["n_beams"], hx(l["min_angle"]),
        hx(l["ang_res"]), hx(l["min_range"]), hx(l["max_range"]), hx(l["range_threshold"]), p["max_unknown"], p["w_unknown"], p["w_free"], p["w_occupied"])


def rule_says(kw):
    """the rule's answer to the same create: "0 reach" or the refusal's number (a view is the rule's to refuse only by its shape)"""
    v, l, p = dict(VIEW), dict(LASER), dict(PARAMS)
    for k, value in kw.items():
        next(d for d in (v, l, p) if k in d)[k] = value
    view = dict(width=v["width"], height=v["height"], ox=v["ox"], oy=v["oy"], anchor=(v["anchor_x"], v["anchor_y"]), scale=v["scale"])
    laser = lc.CaseLaser(l["n_beams"], l["min_angle"], l["ang_res"], l["min_range"], l["max_range"], l["range_threshold"])
    try:
        return "0 %d" % rule.params_check(view, laser, p)
    except rule.Refused as e:
        return str({w: k for k, w in REASONS.items()}[str(e)])


CREATES = [
    (dict(), "0 22"), (dict(max_unknown=-1, w_unknown=0, w_free=255), "0 22"), (dict(w_unknown=255, w_free=255, w_occupied=255), "0 22"), (dict(n_beams=1), "0 22"),
    # the view
    (dict(width=0), "2"), (dict(height=-1), "2"), (dict(width_step=59), "2"), (dict(scale=0.0), "2"), (dict(scale=math.inf), "2"), (dict(anchor_x=math.nan), "2"),
    (dict(width=65536, width_step=65536, height=32768), "2"), (dict(ox=2 ** 31 - 60), "2"), (dict(oy=2 ** 31 - 50), "2"), (dict(ox=2 ** 31 - 61), "0 22"),
    # the laser
    (dict(n_beams=0), "3"), (dict(range_threshold=0.0), "3"), (dict(range_threshold=math.nan), "3"), (dict(range_threshold=2.0 ** 18), "3"), (dict(min_range=math.nan), "3"),
    (dict(max_range=math.nan), "3"), (dict(min_angle=math.inf), "3"), (dict(ang_res=math.nan), "3"),
    # the budget and the weights
    (dict(max_unknown=-2), "4"), (dict(w_unknown=0), "5"), (dict(w_unknown=-1), "5"), (dict(w_free=256), "5"), (dict(w_occupied=-1), "5"), (dict(w_unknown=0, w_occupied=1), "0 22"),
    # the reach: 511 is taken, 512 refused
    (dict(range_threshold=509 / 4.0), "0 511"), (dict(range_threshold=float(np.nextafter(510 / 4.0, 0.0))), "0 511"), (dict(range_threshold=510 / 4.0), "6"),
    (dict(range_threshold=1000.0), "6"), (dict(range_threshold=5.0, scale=128.0), "6"), (dict(range_threshold=361 / 4.0), "0 363"),
    # the order of the refusals
    (dict(width=0, n_beams=0, max_unknown=-2, w_unknown=0, range_threshold=1000.0), "2"), (dict(n_beams=0, max_unknown=-2, w_unknown=0, range_threshold=1000.0), "3"),
    (dict(max_unknown=-2, w_unknown=0, range_threshold=1000.0), "4"), (dict(w_unknown=0, range_threshold=1000.0), "5"),
]


def test_every_refusal_of_create_in_order(check):
    got = check([create_line(**kw) for kw, _ in CREATES])
    for (kw, want), text in zip(CREATES, got):
        assert text == want, kw
        if want != "2":
            assert rule_says(kw) == want, kw
    assert check([create_line(nulls=n) for n in (1, 2, 4, 8, 15)]) == ["1"] * 5
    assert check([create_line(nulls=1, width=0, n_beams=0)]) == ["1"], "a NULL comes first"


def test_the_reach_on_below_and_above_a_cell_count(check):
    na = np.nextafter
    rows = [(5.0, 4.0, 22), (float(na(5.0, 0.0)), 4.0, 21), (float(na(5.0, 9.0)), 4.0, 22), (5.25, 4.0, 23), (float(na(5.25, 0.0)), 4.0, 22), (0.05, 4.0, 2), (0.25, 4.0, 3),
            (float(na(0.25, 0.0)), 4.0, 2), (12.0, 20.0, 242), (25.45, 20.0, 511), (25.5, 20.0, 512), (float(na(25.5, 0.0)), 20.0, 511), (1e-300, 1e-300, 2)]
    got = check(["reach %s %s" % (hx(r), hx(s)) for r, s, _ in rows])
    for (r, s, want), text in zip(rows, got):
        assert int(text) == want == rule.reach_of(lc.circle(4, range_threshold=r), s), (r, s)


def test_bitmap_bytes_and_mask_words(check):
    want = {0: "1 1 4 148", 1: "3 1 4 148", 363: "727 16517 66068 66212", 511: "1023 32705 130820 130964"}
    reaches = [0, 1, 2, 22, 361, 362, 363, 511]
    for reach, text in zip(reaches, check([f"bitmap {r}" for r in reaches])):
        side, words, nbytes, lds = (int(t) for t in text.split())
        assert side == 2 * reach + 1 and words == (side * side + 31) // 32 and nbytes == 4 * words == rule.bitmap_bytes(reach) and lds == nbytes + 4 * 36
        assert text == want.get(reach, text)
        assert lds <= 160 * 1024
    assert rule.bitmap_bytes(361) <= 65536 < rule.bitmap_bytes(362), "the first bitmap above 64 KB"
    assert 1023 * 1023 * 765 < 2 ** 32, "gain cannot overflow"
    sizes = [(1, 1), (7, 1), (32, 1), (33, 1), (60, 50), (521, 802), (13, 9)]
    assert [int(t) for t in check(["mask %d %d" % s for s in sizes])] == [(w * h + 31) // 32 for w, h in sizes]


def call_line(nulls=0, n=5, k=1, min_gain=1, select=1, n_beams=16, scale=4.0, bad_pose=-1, value=0.0):
    return "call %d %d %d %d %d %d %s %d %s" % (nulls, n, k, min_gain, select, n_beams, hx(scale), bad_pose, hx(value))


def test_the_select_bounds_and_every_refusal_of_a_call_in_order(check):
    rows = [(dict(), "0"), (dict(nulls=1), "1"), (dict(nulls=2), "1"), (dict(n=0), "2"), (dict(n=-3), "2"), (dict(n=65537), "2"), (dict(n=65536, k=4096), "0"),
            (dict(n=65536, k=4097), "4"), (dict(k=0), "4"), (dict(k=5), "0"), (dict(k=6), "4"), (dict(k=6, select=0), "0"), (dict(min_gain=0), "5"),
            (dict(min_gain=0, select=0), "0"), (dict(min_gain=0xFFFFFFFF), "0"),
            (dict(bad_pose=3, value=math.nan), "3 3"), (dict(bad_pose=0, value=math.inf), "3 0"), (dict(bad_pose=4, value=2.0 ** 30 / 4.0 + 1.0), "3 4"),
            (dict(bad_pose=4, value=2.0 ** 30 / 4.0), "0"), (dict(n=1024, n_beams=16384), "0"), (dict(n=1025, n_beams=16384), "6"), (dict(n=65536, n_beams=257), "6"),
            # the order
            (dict(nulls=1, n=0, k=0, min_gain=0), "1"), (dict(n=0, k=0, min_gain=0, bad_pose=0, value=math.nan), "2"), (dict(k=0, min_gain=0, bad_pose=1, value=math.nan), "3 1"),
            (dict(k=0, min_gain=0), "4"), (dict(min_gain=0, n=1025, n_beams=16384), "5"), (dict(n=1025, n_beams=16384), "6")]
    got = check([call_line(**kw) for kw, _ in rows])
    for (kw, want), text in zip(rows, got):
        assert text == want, kw
    names = {"2": "n", "4": "k", "5": "min_gain"}
    for kw, want in rows:
        if kw.get("select", 1) and want in ("0", "2", "4", "5") and not kw.get("nulls") and "n_beams" not in kw:
            if want == "0":
                rule.select_check(kw.get("n", 5), kw.get("k", 1), kw.get("min_gain", 1))
            else:
                with pytest.raises(rule.Refused) as e:
                    rule.select_check(kw.get("n", 5), kw.get("k", 1), kw.get("min_gain", 1))
                assert str(e.value) == names[want]


def test_what_counts_as_the_same_window(check):
    fields = ["none", "cells", "step", "width", "height", "ox", "oy", "anchor_x", "anchor_y", "scale", "device"]
    assert check([f"same {f}" for f in fields]) == ["1", "1", "1"] + ["0"] * 8
