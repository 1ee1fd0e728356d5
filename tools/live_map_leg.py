"""Measures the live map (kh_live_map_update) against kh_mapper_build_map and writes profiles/live_map_leg.json.

    python tools/live_map_leg.py [--scans 250,1500] [--repeat 7]

For each session of the lap queue (--scans queue scans; 250 / 1500 give the 168- / 1002-scan sessions of profiles/session_leg.json),
on one GPU, in one process:

  (a) update after 10 new scans: wall time of kh_live_map_update (delta path) against wall time of kh_mapper_build_map after the
      same 10 scans, the order alternating round by round; the trace-kernel times of both by device events
  (b) first full pass: a new live map's first update against kh_mapper_build_map, alternating
  (c) every update of (a) that found moved scans (a loop closure happened): the share of their beams left alone
  (d) rebuild-fraction sweep: k scans moved by a few centimetres with kh_mapper_set_scan_pose (a MOVE walks a beam twice: the
      dearest kind of record), one live map forced to the delta path and one to the rebuild path updated alternately; the
      crossover is the smallest fraction k / alive at which the delta path's median wall time exceeds the rebuild path's

Medians over --repeat rounds after a warm-up round.  No ratio is asserted: the record says what was measured."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, synth  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402

RES = 0.05
FRACTIONS = (0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.75, 1.0)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def session(n_queue, repeat):
    world = synth.make_world(12345)
    extra = 40 * (repeat + 2)
    truth, odom = synth.trajectory_laps(n_queue + extra)
    rng = np.random.default_rng(4)
    m = Mapper(synth.Laser(), loop_search_maximum_distance=3.0)
    nxt = [0]

    def accept(k):
        got = 0
        while got < k:
            i = nxt[0]
            got += int(m.Process(synth.make_scan(world, truth[i], rng), odom[i], 0.1 * i)[0])
            nxt[0] += 1

    while nxt[0] < n_queue:
        accept(1)
    live = m.live_map(RES, rebuild_fraction=math.inf)
    live.update()
    m.build_map(RES).close()
    upd_ms, upd_trace, build_ms, build_trace, skipped = [], [], [], [], []

    def build():
        g = m.build_map(RES)
        ms = g.stats()["trace_ms"]
        g.close()
        return ms

    for rep in range(-1, repeat):
        accept(10)
        if rep % 2:
            b, bt = timed(build)
            u, last = timed(live.update)
        else:
            u, last = timed(live.update)
            b, bt = timed(build)
        if last["scans_moved"]:
            kept = last["beams_skipped"] + (last["beams_traced"] - 10 * 1081) / 2.0
            skipped.append({"scans_moved": last["scans_moved"], "beams_skipped": last["beams_skipped"], "beams_traced": last["beams_traced"],
                            "share_skipped_of_moved_traced_beams": float(last["beams_skipped"] / max(kept, 1.0))})
        if rep >= 0:
            upd_ms.append(u); upd_trace.append(last["trace_ms"]); build_ms.append(b); build_trace.append(bt)
    n_alive = len(m.alive())
    first_ms, first_build = [], []
    for rep in range(-1, repeat):
        def first():
            f = m.live_map(RES, live.info()["anchor"], math.inf)
            f.update()
            f.close()
        if rep % 2:
            a = timed(first)[0]
            b = timed(build)[0]
        else:
            b = timed(build)[0]
            a = timed(first)[0]
        if rep >= 0:
            first_ms.append(a); first_build.append(b)
    # (d) the sweep
    rebuilt = m.live_map(RES, live.info()["anchor"], 0.0)
    rebuilt.update()
    prng = np.random.default_rng(11)
    sweep, crossover = [], None
    for frac in FRACTIONS:
        k = max(1, int(round(frac * n_alive)))
        d_ms, r_ms, d_tr, r_tr = [], [], [], []
        for rep in range(-1, repeat):
            ids = prng.choice(m.alive(), size=k, replace=False)
            poses = m.poses()
            for i in ids:
                m.set_scan_pose(int(i), poses[int(i)] + np.array([prng.normal(0, 0.03), prng.normal(0, 0.03), prng.normal(0, 0.002)]))
            if rep % 2:
                r, rl = timed(rebuilt.update)
                d, dl = timed(live.update)
            else:
                d, dl = timed(live.update)
                r, rl = timed(rebuilt.update)
            assert dl["rebuilds"] == 0 and rl["rebuilds"] == 1 and dl["scans_moved"] == k
            if rep >= 0:
                d_ms.append(d); r_ms.append(r); d_tr.append(dl["trace_ms"]); r_tr.append(rl["trace_ms"])
        sweep.append({"fraction": k / n_alive, "scans_moved": k, "delta_wall_ms": spread(d_ms), "rebuild_wall_ms": spread(r_ms),
                      "delta_trace_ms": spread(d_tr), "rebuild_trace_ms": spread(r_tr)})
        if crossover is None and np.median(d_ms) > np.median(r_ms):
            crossover = k / n_alive
    record = {"queue_scans": n_queue, "scans_alive": n_alive, "window": [live.info()[k] for k in ("ox", "oy", "width", "height")],
              "log_bytes": live.stats()["log_bytes"],
              "a_update_after_10_wall_ms": spread(upd_ms), "a_update_after_10_trace_ms": spread(upd_trace),
              "a_build_map_after_10_wall_ms": spread(build_ms), "a_build_map_after_10_trace_ms": spread(build_trace),
              "a_build_over_update_wall": float(np.median(build_ms) / np.median(upd_ms)),
              "b_first_pass_wall_ms": spread(first_ms), "b_build_map_wall_ms": spread(first_build),
              "c_updates_behind_a_closure": skipped, "d_sweep": sweep, "d_crossover_fraction": crossover}
    rebuilt.close(); live.close(); m.close()
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", default="250,1500")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_map_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("live_map_leg needs a GPU: nothing here is measured without one")
    record = {"resolution": RES, "sessions": [session(int(n), args.repeat) for n in args.scans.split(",")]}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
