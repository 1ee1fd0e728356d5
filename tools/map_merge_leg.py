"""Measures the map merge (kh_map_merge_*) and writes profiles/map_merge_leg.json.

    python tools/map_merge_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_match_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500).  It is merged with itself under the correction (0.73, -0.41, 0.3).  On one GPU, in one process, by device events:

  k_map_known_box over the moving window; k_map_merge in ns per output cell at footprints 1 and 2, with the window grown (the default)
  and not grown (the target's own window); the downloads of cells, codes and nav values (wall); and beside them k_map_diff of a change
  layer on the same map -- a kernel this leg does not change -- over the target's window: the per-cell pass the merge is to be compared
  with (one thread per cell, two counter loads, one byte load, two byte stores, against four cells per thread, a gather through a
  rotation per sample, two dword stores).

Medians of --rounds rounds after a warm-up round.  No threshold is attached."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, synth  # noqa: E402
from slam_toolbox_amd.map_changes import MapChanges  # noqa: E402
from slam_toolbox_amd.map_merge import MapMerge  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES = 0.05
CORRECTION = (0.73, -0.41, 0.3)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_merge_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_merge_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(r, p, LASER.min_angle, LASER.ang_res) for r, p in zip(ranges, truth[:n])], RES, LASER)
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "correction": list(CORRECTION)}

    for grow in (1, 0):
        for footprint in (1, 2):
            box_ms, merge_ms, call_ms, downloads, last = [], [], [], {"cells": [], "codes": [], "nav": []}, None
            for k in range(a.rounds + 1):
                m = MapMerge(grid, grid, CORRECTION, footprint=footprint, grow=grow)
                box_ms.append(m.stats["times_ms"][0]); merge_ms.append(m.stats["times_ms"][1]); call_ms.append(m.stats["times_ms"][2])
                for name in downloads:
                    downloads[name].append(wall_ms(getattr(m, name)))
                last = dict(m.stats)
                m.close()
            cells = last["width"] * last["height"]
            record[f"grow_{grow}_footprint_{footprint}"] = {
                "output_width": last["width"], "output_height": last["height"], "output_cells": cells,
                "counters": {c: last[c] for c in ("target_only", "moving_only", "agree_free", "agree_occupied", "conflict_moving_occupied",
                                                  "conflict_moving_free", "overlap")}, "agreement": last["agreement"],
                "k_map_known_box_ms": spread(box_ms[1:]), "k_map_merge_ms": spread(merge_ms[1:]),
                "k_map_merge_ns_per_output_cell": spread(1e6 * np.asarray(merge_ms[1:]) / cells), "create_call_ms": spread(call_ms[1:]),
                "download_ms": {name: spread(v[1:]) for name, v in downloads.items()}}
            print(grow, footprint, record[f"grow_{grow}_footprint_{footprint}"], flush=True)

    layer = MapChanges(grid)
    layer.observe(LASER, ranges[0], truth[0])
    diff_ms = [layer.diff(cap=0)["diff_kernel_ms"] for _ in range(a.rounds + 1)]
    record["k_map_diff_same_map"] = {"cells": grid.width * grid.height, "k_map_diff_ms": spread(diff_ms[1:]),
                                     "k_map_diff_ns_per_cell": spread(1e6 * np.asarray(diff_ms[1:]) / (grid.width * grid.height))}
    print("diff", record["k_map_diff_same_map"], flush=True)
    layer.close(); grid.close()
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
