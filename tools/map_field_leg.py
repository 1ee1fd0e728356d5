"""Measures the distance field of a map (kh_map_field_*) and writes profiles/map_field_leg.json.

    python tools/map_field_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_match_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500).  On one GPU, in one process:

  k_field_columns and k_field_rows by device events, in ns per cell, for the default field (2 m: 40 cells), a short one (0.55 m: 11
  cells) and the uncapped one, with obstacles = occupied and = not free; the whole create call (wall, with the snapshot copy and the
  allocations); the costs (call, wall: table upload, kernel, download), the clearance of 1 and of 4096 points (call, wall), the
  score of one scan at 1 and at 27 x 64 poses (call, wall) and a refinement of 64 starts (kernels by events summed, and the call).

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
from slam_toolbox_amd.map_field import MapField  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES = 0.05


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_field_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_field_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(r, p, LASER.min_angle, LASER.ang_res) for r, p in zip(ranges, truth[:n])], RES, LASER)
    cells = grid.width * grid.height
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "cells": cells}

    for obstacles in ("occupied", "not_free"):
        for max_distance in (2.0, 0.55, 0.0):
            columns, rows, call, last = [], [], [], None
            for _ in range(a.rounds + 1):
                f = MapField(grid, max_distance=max_distance, obstacles=obstacles)
                columns.append(f.stats["times_ms"][0]); rows.append(f.stats["times_ms"][1]); call.append(f.stats["times_ms"][2])
                last = dict(f.stats)
                f.close()
            key = f"{obstacles}_max_distance_{max_distance}"
            record[key] = {"radius_cells": last["radius_cells"], "n_obstacles": last["n_obstacles"], "n_far": last["n_far"], "max_d2": last["max_d2"],
                           "k_field_columns_ms": spread(columns[1:]), "k_field_rows_ms": spread(rows[1:]),
                           "k_field_columns_ns_per_cell": spread(1e6 * np.asarray(columns[1:]) / cells),
                           "k_field_rows_ns_per_cell": spread(1e6 * np.asarray(rows[1:]) / cells), "create_call_ms": spread(call[1:])}
            print(key, record[key], flush=True)

    f = MapField(grid, max_distance=2.0)
    pose = np.asarray(truth[n // 2], dtype=np.float64)
    scan = ranges[n // 2]
    xy = rng.uniform(-1.0, 1.0, size=(4096, 2)) * 5.0 + pose[:2]
    poses = pose + rng.uniform(-1.0, 1.0, size=(27 * 64, 3)) * [0.3, 0.3, 0.05]
    starts = poses[:64]
    calls = {"costs": lambda: f.costs(), "read_d2": lambda: f.d2, "clearance_1": lambda: f.clearance(xy[:1]), "clearance_4096": lambda: f.clearance(xy),
             "score_1_pose": lambda: f.score(scan, poses[:1], LASER), "score_1728_poses": lambda: f.score(scan, poses, LASER)}
    record["readers_call_ms"] = {name: spread([wall_ms(fn) for _ in range(a.rounds + 1)][1:]) for name, fn in calls.items()}
    print("readers", record["readers_call_ms"], flush=True)
    for truncate in (0, 6):
        kernel, call, rounds = [], [], None
        for _ in range(a.rounds + 1):
            out, times = f.refine(scan, starts, LASER, truncate_cells=truncate)
            kernel.append(times[0]); call.append(times[1])
            rounds = [r.rounds for r in out]
        record[f"refine_64_starts_truncate_{truncate}"] = {
            "kernels_ms": spread(kernel[1:]), "call_ms": spread(call[1:]), "launches": 1 + max(rounds), "rounds": spread(rounds),
            "median_end_offset_m": float(np.median([np.hypot(*(r.pose[:2] - pose[:2])) for r in out])),
            "median_start_offset_m": float(np.median(np.hypot(*(starts[:, :2] - pose[:2]).T)))}
        print("refine", truncate, record[f"refine_64_starts_truncate_{truncate}"], flush=True)
    f.close(); grid.close()
    with open(a.out, "w") as out_file:
        json.dump(record, out_file, indent=1)
        out_file.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
