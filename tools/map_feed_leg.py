"""Measures the map feed (kh_map_feed_poll) against the route without it and writes profiles/map_feed_leg.json.

    python tools/map_feed_leg.py [--scans 1500] [--every 25]

The lap queue (--scans queue scans) runs through one mapper with a live map at 0.05 m, on one GPU, in one process.  Every --every
accepted scans a ROUND does kh_live_map_update and then, the order alternating round by round,

  (feed)  kh_map_feed_poll + kh_map_feed_tiles: wall time, the compare kernel's time by device events, tiles_scanned, n_tiles,
          bytes_downloaded;
  (read)  what a consumer does without a feed: kh_live_map_read(cells) of the whole window and the toNavMap rule over it as a
          256-entry numpy lookup: wall time of both, bytes downloaded.

Once per round, outside the timed parts, the consumer's map patched from the tiles is compared with the lookup's result.  No ratio
is asserted: the record says what was measured."""
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
TILE = capi.KH_MAP_TILE
LOOKUP = np.full(256, -1, dtype=np.int8)
LOOKUP[100], LOOKUP[255] = 100, 0


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run(n_queue, every):
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_queue)
    rng = np.random.default_rng(4)
    m = Mapper(synth.Laser(), loop_search_maximum_distance=3.0)
    live = m.live_map(RES, np.array([-30.0, -30.0]), math.inf)      # (lower left of the 60 m x 40 m world by more than the range threshold)
    feed = live.feed()
    consumer, window = None, (0, 0, 0, 0)
    rounds, since = [], 0

    def read_route():
        cells = live.cells()
        return LOOKUP[cells[:, :live.info()["width"]]]

    for i in range(n_queue):
        since += int(m.Process(synth.make_scan(world, truth[i], rng), odom[i], 0.1 * i)[0])
        if since < every and i != n_queue - 1:
            continue
        if since == 0:
            continue
        last = live.update()
        if len(rounds) % 2:
            r_ms, nav = timed(read_route)
            f_ms, (delta, xy, data) = timed(feed.poll)
        else:
            f_ms, (delta, xy, data) = timed(feed.poll)
            r_ms, nav = timed(read_route)
        # the consumer: grown with -1 to the feed's window, the tiles written over it; it must be what the other route read
        win = (delta["ox"], delta["oy"], delta["width"], delta["height"])
        grown = np.full((win[3], win[2]), -1, dtype=np.int8)
        if consumer is not None:
            grown[window[1] - win[1]:window[1] - win[1] + window[3], window[0] - win[0]:window[0] - win[0] + window[2]] = consumer
        for (tx, ty), tile in zip(xy, data):
            grown[TILE * ty - win[1]:TILE * ty - win[1] + TILE, TILE * tx - win[0]:TILE * tx - win[0] + TILE] = tile
        consumer, window = grown, win
        if not np.array_equal(consumer, nav):
            raise RuntimeError(f"round {len(rounds)}: the consumer's map differs from toNavMap of the live map's cells")
        rounds.append({"scans_added": since, "scans_moved": last["scans_moved"], "relayout": last["relayouts"], "window": list(win),
                       "cells_updated": last["cells_updated"], "poll_wall_ms": f_ms, "poll_kernel_ms": delta["kernel_ms"],
                       "tiles_scanned": delta["tiles_scanned"], "n_tiles": delta["n_tiles"], "bytes_downloaded": delta["bytes_downloaded"],
                       "read_and_lookup_wall_ms": r_ms, "read_bytes_downloaded": int(win[2]) * int(win[3])})
        since = 0
    steady = [r for r in rounds[1:] if not r["relayout"]] or rounds
    record = {"resolution": RES, "queue_scans": n_queue, "update_every_accepted_scans": every, "scans_alive": len(m.alive()),
              "final_window": list(window), "rounds": rounds,
              "summary_rounds_without_relayout": {
                  "rounds": len(steady),
                  "poll_wall_ms": spread([r["poll_wall_ms"] for r in steady]),
                  "poll_kernel_ms": spread([r["poll_kernel_ms"] for r in steady]),
                  "read_and_lookup_wall_ms": spread([r["read_and_lookup_wall_ms"] for r in steady]),
                  "bytes_downloaded": spread([r["bytes_downloaded"] for r in steady]),
                  "read_bytes_downloaded": spread([r["read_bytes_downloaded"] for r in steady]),
                  "n_tiles": spread([r["n_tiles"] for r in steady]), "tiles_scanned": spread([r["tiles_scanned"] for r in steady])},
              "feed_stats": feed.stats()}
    feed.close(); live.close(); m.close()
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--every", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_feed_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("map_feed_leg needs a GPU: nothing here is measured without one")
    record = run(args.scans, args.every)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps({k: v for k, v in record.items() if k != "rounds"}))


if __name__ == "__main__":
    main()
