"""The host rules of the live map and its feed (slam_toolbox_amd/csrc/live_map_plan.hpp) on the CPU: floor division, the window,
classification and slots over a scripted history, the touched rectangle and the feed's tile job, through the stand-alone program
tests/live_map_plan_check.cpp.  Expectations come from tests/live_map_rule.py, tests/map_feed_rule.py and plain Python.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import live_map_rule as rule
import map_feed_rule as feed_rule

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 2 ** 31 - 4096


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "live_map_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(HERE, "live_map_plan_check.cpp"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout
        return out
    return run


def hx(v):
    return float(v).hex()


def test_floor_div(check):
    cases = [(a, b) for b in (4, 16, 64) for a in range(-130, 131)]
    got = check([f"floordiv {a} {b}" for a, b in cases])
    assert [int(g) for g in got] == [a // b for a, b in cases]


def _window(check, previous, sensor_xy, anchor, resolution, range_threshold):
    px, py, pw, ph = previous if previous is not None else (0, 0, 0, 0)
    xy = np.asarray(sensor_xy, dtype=np.float64).reshape(-1, 2)
    line = (f"window {hx(anchor[0])} {hx(anchor[1])} {hx(resolution)} {hx(range_threshold)} {px} {py} {px + pw} {py + ph} {len(xy)} " +
            " ".join(f"{hx(x)} {hx(y)}" for x, y in xy))
    return tuple(int(v) for v in check([line])[0].split())


def test_window(check):
    res, rt, anchor = 0.05, 12.0, (1.25, -0.75)
    r = rule.reach(rt, res)

    def at(cx, cy):                                    # a sensor position in the middle of lattice cell (cx, cy)
        return (anchor[0] + cx * res, anchor[1] + cy * res)

    def same(previous, xy):
        want = rule.window(previous, np.asarray(xy).reshape(-1, 2), anchor, res, rt)
        assert _window(check, previous, xy, anchor, res, rt) == tuple(int(v) for v in want)
        return want

    first = same(None, [at(3, 5)])                     # no previous window, one scan
    assert first[2] % rule.BLOCK == 0 and first[0] % rule.BLOCK == 0
    # cell - reach exactly on a multiple of 64, one below, one above; right of and left of the anchor
    for block in (rule.BLOCK * 5, -rule.BLOCK * 7):
        for d in (-1, 0, 1):
            cx = block + r + d
            assert rule.cells_of(at(cx, 9), anchor, res)[0, 0] == cx
            want = same(None, [at(cx, 9)])
            assert want[0] == (block if d >= 0 else block - rule.BLOCK)
            same(first, [at(cx, 9)])
    grown = same(first, [at(first[0] - 1, first[1] - 1)])          # growth on both low sides at once
    assert grown[0] < first[0] and grown[1] < first[1] and grown[0] + grown[2] == first[0] + first[2]
    assert same(grown, [at(3, 5), at(4, 4)]) == grown              # a scan inside the previous window: the window itself


def test_size_cap(check):
    # arithmetic only.  Lattice of 1 m cells, reach 14: two scans in row 20 give a window one block high; the far one sets the width.
    res, rt, anchor = 1.0, 12.0, (0.0, 0.0)
    assert rule.reach(rt, res) == 14
    cases = []
    for total in (CAP, CAP - 64 * rule.BLOCK):         # (padded) cells of the window: 2^31 - 4096, and one block of columns less
        width = total // rule.BLOCK
        cases.append((0, width))
    for width in (CAP, CAP - rule.BLOCK):              # a width of 2^31 - 4096 cells itself, and one block less
        cases.append((-(2 ** 30 - 2048), width))
    for x0, width in cases:
        assert width % rule.BLOCK == 0 and x0 % rule.BLOCK == 0
        xy = [(x0 + 14.0, 20.0), (x0 + width - 78.0, 20.0)]
        want = tuple(int(v) for v in rule.window(None, np.array(xy), anchor, res, rt))
        assert want == (x0, 0, width, rule.BLOCK)
        assert _window(check, None, xy, anchor, res, rt) == want
        assert int(check([f"cap {width} {rule.BLOCK}"])[0]) == int((width + 7) * rule.BLOCK > CAP)
    assert [int(v) for v in check([f"cap {CAP // 64} 64", f"cap {CAP // 64 - 64} 64", f"cap {2 ** 32} {2 ** 32}", "cap 0 0"])] == [1, 0, 1, 0]


# ---- classification and slots: a scripted history over scan ids 0 .. 7 against a dictionary model
RES, RT, ANCHOR = 0.05, 12.0, (0.0, 0.0)
P = {i: (0.5 * i, 0.25 * i, 0.01 * i) for i in range(8)}


def _moved(p):
    return (p[0] + RES, p[1], p[2])                    # by one cell


HISTORY = [                                            # (poses by id, must_rebuild)
    ({0: P[0], 2: P[2], 5: P[5]}, False),                                  # add, with gaps in the ids
    ({0: P[0], 2: _moved(P[2]), 5: P[5]}, False),                          # a move by one cell; the others bitwise equal
    ({0: P[0], 2: _moved(P[2]), 5: P[5]}, False),                          # nothing changed
    ({0: P[0], 5: P[5]}, False),                                           # a removal
    ({0: P[0], 5: P[5], 6: P[6]}, False),                                  # the freed slot is reused now
    ({5: P[5], 6: P[6], 7: P[7]}, False),                                  # a removal and an add in the same update
    ({5: P[5], 6: P[6], 7: P[7], 3: P[3], 4: P[4]}, False),                # ids that fill gaps: one freed slot, one new
    ({5: _moved(P[5]), 6: P[6], 7: P[7], 3: P[3], 4: P[4]}, True),         # a rebuild: slots restart at 0
    ({6: P[6], 7: P[7], 4: P[4], 1: P[1]}, False),                         # two leave, one comes
    ({6: P[6], 7: _moved(P[7]), 4: P[4], 1: P[1], 2: P[2]}, False),        # a move and an add after it
]


def _fields(line):
    """the key=value fields of print_update; values may hold blanks (rectangles)"""
    keys = ("rebuild", "needed", "window", "touched", "counted", "added", "moved", "gone", "live")
    out = {}
    for k, key in enumerate(keys):
        start = line.index(key + "=") + len(key) + 1
        end = line.index(" " + keys[k + 1] + "=") if k + 1 < len(keys) else len(line)
        out[key] = line[start:end]
    pairs = lambda s: {int(a): int(b) for a, b in (t.split(":") for t in s.split(",") if t)}      # noqa: E731
    ids = lambda s: [int(t) for t in s.split(",") if t]                                           # noqa: E731
    return {"rebuild": int(out["rebuild"]), "needed": int(out["needed"]), "window": out["window"], "touched": out["touched"],
            "counted": tuple(ids(out["counted"])), "added": pairs(out["added"]), "moved": ids(out["moved"]), "gone": ids(out["gone"]),
            "live": pairs(out["live"])}


def test_classification_and_slots(check):
    lines = [f"lattice {hx(ANCHOR[0])} {hx(ANCHOR[1])} {hx(RES)} {hx(RT)}"]
    for poses, must in HISTORY:
        lines.append(f"update {int(must)} inf {len(poses)} " + " ".join(f"{i} {hx(p[0])} {hx(p[1])} {hx(p[2])}" for i, p in sorted(poses.items())))
    got = check(lines)
    assert got[0] == "ok"
    model, free, next_slot = {}, [], 0                 # id -> (pose, slot); the free list; the slots dealt so far
    freed_before, window = [], None
    for step, ((poses, must), line) in enumerate(zip(HISTORY, got[1:])):
        f = _fields(line)
        added = sorted(i for i in poses if i not in model)
        moved = sorted(i for i in poses if i in model and model[i][0] != poses[i])
        gone = sorted(i for i in model if i not in poses)
        assert f["counted"] == (len(added), len(moved)) and f["gone"] == gone and f["rebuild"] == int(must), (step, line)
        changed = [poses[i][:2] for i in added + moved]
        window = rule.window(window, np.array(changed).reshape(-1, 2), ANCHOR, RES, RT)
        assert f["window"] == "%d %d %d %d" % (window[0], window[1], window[0] + window[2], window[1] + window[3]), (step, line)
        if must:
            assert f["moved"] == [] and f["added"] == {i: k for k, i in enumerate(sorted(poses))}, (step, line)      # slots restart at 0
            model, free, next_slot = {}, [], 0
            added, gone = sorted(poses), []
        else:
            assert sorted(f["added"]) == added and f["moved"] == moved, (step, line)
        freed_now = [model[i][1] for i in gone]
        for i in added:                                # last in, first out, then a new slot
            slot = free.pop() if free else next_slot
            next_slot = max(next_slot, slot + 1)
            model[i] = (poses[i], slot)
            assert f["added"][i] == slot, (step, line)
            assert slot not in freed_now, "a slot freed in this update was dealt in it"
        if freed_before and added and not must:
            assert f["added"][added[0]] == freed_before[-1], "a slot freed in the update before is the first one reused"
        for i in moved:
            model[i] = (poses[i], model[i][1])
        for i in gone:
            free.append(model.pop(i)[1])
        freed_before = freed_now
        assert f["live"] == {i: s for i, (_, s) in model.items()}, (step, line)
        slots = list(f["live"].values())
        assert len(set(slots)) == len(slots), "two live scans share a slot"
        assert all(s < f["needed"] for s in f["added"].values()) and f["needed"] == next_slot, (step, line)
        # the touched rectangle: reach around every position, old and new, in window columns and rows ("none": nothing changed)
        if not (added or moved or gone):
            assert f["touched"] == "none"
    # the history did what it is meant to do
    steps = [_fields(line) for line in got[1:]]
    assert steps[4]["added"] == {6: 1} and steps[5]["added"] == {7: 3} and steps[5]["gone"] == [0]
    assert steps[6]["added"] == {3: 0, 4: 4} and steps[7]["live"] == {3: 0, 4: 1, 5: 2, 6: 3, 7: 4}


def test_touched_rectangle(check):
    reach, win = 10, (-64, -64, 128, 64)
    cases = {
        "middle": f"touched {reach} {win[0]} {win[1]} {win[2]} {win[3]} 1 30 0 0 0",
        "corner": f"touched {reach} {win[0]} {win[1]} {win[2]} {win[3]} 1 -60 -61 0 0",
        "moved": f"touched {reach} {win[0]} {win[1]} {win[2]} {win[3]} 0 1 20 -5 23 -4 0",
        "gone": f"touched {reach} {win[0]} {win[1]} {win[2]} {win[3]} 0 0 1 100 40",
        "nothing": f"touched {reach} {win[0]} {win[1]} {win[2]} {win[3]} 0 0 0",
        "outside": f"touched {reach} {win[0]} {win[1]} {win[2]} {win[3]} 1 500 500 0 0",
    }
    got = dict(zip(cases, check(list(cases.values()))))

    def box(*cells):                                   # the union of cell +- reach, clipped to the window, in its columns and rows
        x0, y0 = min(c[0] for c in cells) - reach, min(c[1] for c in cells) - reach
        x1, y1 = max(c[0] for c in cells) + reach + 1, max(c[1] for c in cells) + reach + 1
        x0, y0, x1, y1 = max(x0, win[0]), max(y0, win[1]), min(x1, win[2]), min(y1, win[3])
        return "%d %d %d %d" % (x0 - win[0], y0 - win[1], x1 - win[0], y1 - win[1])

    assert got["middle"] == box((30, 0)) == "84 54 105 75"                 # 2 reach + 1 = 21 on a side
    assert got["corner"] == box((-60, -61)) == "0 0 15 14"                 # clipped at the window's low corner
    assert got["moved"] == box((20, -5), (23, -4))                         # the union of the old and the new position
    assert got["gone"] == box((100, 40))
    assert got["nothing"] == "none" and got["outside"] == "none"


def test_tile_job(check):
    win = (-64, -64, 64, 64)
    edges = (-17, -16, -1, 0, 15, 16)
    cases = [(x0, y0, x1, y1) for x0 in edges for x1 in edges if x1 > x0 for (y0, y1) in ((x0, x1), (-16, 15))]
    got = check([f"tiles 0 {x0} {y0} {x1} {y1} {win[0]} {win[1]} {win[2]} {win[3]}" for x0, y0, x1, y1 in cases])
    for (x0, y0, x1, y1), line in zip(cases, got):
        want = (feed_rule.tile_of(x0), feed_rule.tile_of(y0), feed_rule.tile_of(x1 - 1) + 1, feed_rule.tile_of(y1 - 1) + 1)
        assert line == "%d %d %d %d" % tuple(int(v) for v in want), (x0, y0, x1, y1)
    whole = "%d %d %d %d" % tuple(int(feed_rule.tile_of(v)) for v in win)
    outside, straddling = (64, 0, 100, 10), (50, -100, 100, -60)
    got = check([f"tiles 1 0 0 0 0 {win[0]} {win[1]} {win[2]} {win[3]}",                       # pending_whole: the rectangle is not looked at
                 f"tiles 1 -3 -3 5 5 {win[0]} {win[1]} {win[2]} {win[3]}",
                 "tiles 0 %d %d %d %d %d %d %d %d" % (outside + win),                          # wholly outside: an empty job
                 "tiles 0 0 0 0 0 %d %d %d %d" % win,                                          # nothing pending
                 "tiles 0 %d %d %d %d %d %d %d %d" % (straddling + win)])                      # clipped to the window first
    assert got == [whole, whole, "none", "none", "3 -4 4 -3"]
