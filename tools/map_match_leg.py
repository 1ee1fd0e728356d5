"""Measures the map-sourced rasterisation (kh_matcher_add_map / kh_matcher_match_map_batch) against the
scan-sourced one and writes profiles/map_match_leg.json.

    python tools/map_match_leg.py [--scans 250,1500] [--rounds 10]

For each map -- the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m -- and each of the sequential and the
loop preset, on one GPU, in one process, with one handle:

  (a) k_map_collect (count, scan, fill) per rasterisation from the map, by device events (kh_matcher_profile_map)
  (b) the whole rasterisation, by device events (kh_matcher_profile): from the map, from the 10-scan running chain in front of the
      query, and from a 50-scan chain of the same place -- the routes a caller has today
  (c) a whole kh_matcher_match_map_batch of 1 and of 64 queries: HOST wall time of the call with profiling on (key
      host_wall_ms_profiling_on; not device time: the call returns synchronised, its kernels run on several streams, so no pair of
      events brackets it, and profiling adds an event wait behind the rasteriser); the rasteriser's share of it by device events

Medians of --rounds rounds after a warm-up round.  No threshold is attached: whether a map is cheaper than a chain is what the
record is for."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, synth  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan, MapperParams, ScanMatcher  # noqa: E402

LASER = synth.Laser()
PARAMS = dict(coarse_search_angle_offset=0.349, coarse_angle_resolution=0.0349, fine_search_angle_offset=0.00349,
              use_response_expansion=True, distance_variance_penalty=0.5, minimum_distance_penalty=0.5,
              angle_variance_penalty=1.0, minimum_angle_penalty=0.9)
PRESETS = {"sequential": (0.5, 0.01, 0.1, 20.0), "loop": (8.0, 0.05, 0.03, 20.0)}      # config/mapper_params_offline.yaml
BATCH = 64


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def measure(hm, rounds, call):
    """per round: (raster ms by events, collect ms by events, host wall ms with profiling on) of call()"""
    out = []
    for k in range(rounds + 1):
        hm.profile(True); hm.profile_map()
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        out.append((hm.profile(True)["raster_ms"], hm.profile_map()["collect_ms"], wall))
    hm.profile(False)
    r = np.array(out[1:])
    return {"raster_ms": spread(r[:, 0]), "collect_ms": spread(r[:, 1]), "host_wall_ms_profiling_on": spread(r[:, 2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", default="250,1500")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_match_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_match_leg needs a GPU")
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    counts = [int(s) for s in a.scans.split(",")]
    truth, _ = synth.trajectory_laps(max(counts) + BATCH)
    record = {"resolution": 0.05, "rounds": a.rounds, "maps": []}
    scans = []
    for n in counts:
        while len(scans) < n + BATCH:
            i = len(scans)
            scans.append(LocalizedRangeScan(synth.make_scan(world, truth[i], rng), truth[i], LASER.min_angle, LASER.ang_res))
        grid = OccupancyGrid.CreateFromScans(scans[:n], 0.05, LASER)
        entry = {"n_scans": n, "width": grid.width, "height": grid.height, "occupied_cells": int((grid.cells() == 100).sum()), "presets": {}}
        # the queries: the scans behind the map's last, handed over a little off their poses
        queries = [LocalizedRangeScan(s.ranges, s.sensor_pose + np.array([0.04, -0.03, 0.02]), LASER.min_angle, LASER.ang_res)
                   for s in scans[n:n + BATCH]]
        q = queries[0]
        chain10 = scans[n - 10:n]
        near = np.argsort([np.hypot(*(s.sensor_pose[:2] - q.sensor_pose[:2])) for s in scans[:n]])[:50]
        chain50 = [scans[i] for i in sorted(near)]
        for name, create in PRESETS.items():
            hm = ScanMatcher.Create(MapperParams(**PARAMS), *create, max_batch=BATCH)
            p = {"add_map": measure(hm, a.rounds, lambda: hm.AddMap(q, grid)),
                 "add_scans_chain10": measure(hm, a.rounds, lambda: hm.AddScans(q, chain10)),
                 "add_scans_chain50": measure(hm, a.rounds, lambda: hm.AddScans(q, chain50)),
                 "match_map_batch_1": measure(hm, a.rounds, lambda: hm.MatchScanMapBatch(queries[:1], grid)),
                 "match_map_batch_64": measure(hm, a.rounds, lambda: hm.MatchScanMapBatch(queries, grid))}
            resp = hm.MatchScanMapBatch(queries, grid)[0]
            p["responses_batch_64"] = spread(resp)
            for k in ("add_scans_chain10", "add_scans_chain50"):
                del p[k]["collect_ms"]
            entry["presets"][name] = p
            print(name, n, {k: v["raster_ms"]["median"] for k, v in p.items() if "raster_ms" in v}, flush=True)
            hm.close()
        record["maps"].append(entry)
        grid.close()
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
