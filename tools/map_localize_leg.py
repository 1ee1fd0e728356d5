"""Measures the map localizer (kh_map_localizer_*, kh_map_fit) and writes profiles/map_localize_leg.json.

    python tools/map_localize_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_match_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500).  On one GPU, in one process:

  (a) a whole-map relocalization of the scan behind the map's last at the defaults (seed spacing loop_search_space_dimension / 4,
      the default headings), split into the seed kernel and the fit kernel (device events), the coarse and the fine batches (wall)
      and the rest of the call (host: seeds' download and compaction, ranking, suppression)
  (b) k_map_fit per beam and pose (device events; the poses are the hypotheses of a relocalization with every gate open and no
      suppression) against k_occ_fit_merged per beam and candidate (kh_merge_fit_stats) for the same scan as a one-scan submap
      fitted, under as many candidates, against a mapper that processed the map's scans
  (c) one kh_map_localizer_process step per scan over the 64 scans behind the map (wall), against kh_mapper_process_localization
      per scan over the same scans behind the same scans' mapper

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
from slam_toolbox_amd.map_localizer import MapLocalizer  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402
from slam_toolbox_amd.merge import MapMerger  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES, TRACK = 0.05, 64
OPEN = dict(minimum_response_coarse=-1.0, maximum_variance_coarse=1e30, minimum_response_fine=-1.0, merge_distance=0.0)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_localize_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_localize_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, odom = synth.trajectory_laps(n + TRACK)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n + TRACK)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(ranges[i], truth[i], LASER.min_angle, LASER.ang_res) for i in range(n)], RES, LASER)
    cells = grid.cells()[:, :grid.width]
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height,
              "occupied_cells": int((cells == 100).sum()), "free_cells": int((cells == 255).sum()), "n_beams": LASER.n_beams}
    loc = MapLocalizer(None, LASER, max_batch=64).set_map(grid)
    query = ranges[n]

    # (a) the whole map at the defaults
    rows = []
    for k in range(a.rounds + 1):
        hyps, s = loc.relocalize(query)
        rows.append(s)
    rows = rows[1:]
    split = {k: spread([r[k] for r in rows]) for k in ("seed_kernel_ms", "coarse_ms", "fine_ms", "fit_kernel_ms", "total_ms")}
    split["host_ms"] = spread([r["total_ms"] - r["seed_kernel_ms"] - r["coarse_ms"] - r["fine_ms"] - r["fit_kernel_ms"] for r in rows])
    best = hyps[0] if hyps else None
    record["a_whole_map"] = dict(split, counts={k: rows[-1][k] for k in rows[-1] if k.startswith("n_")},
                                 best_error_m=None if best is None else float(np.hypot(*(best.robot_pose[:2] - truth[n, :2]))),
                                 best_fine_response=None if best is None else best.fine_response,
                                 best_fit_score=None if best is None else best.fit["score"])
    print("a", {k: v["median"] for k, v in split.items()}, record["a_whole_map"]["counts"], flush=True)

    # (b) the fit kernel per beam and pose, against the merger's per beam and candidate
    region = dict(center_xy=tuple(truth[n, :2]), radius=6.0, top_k=0, **OPEN)
    per_beam, poses = [], 0
    for k in range(a.rounds + 1):
        hyps, s = loc.relocalize(query, cap=4096, **region)
        poses = s["n_accepted"]
        per_beam.append(1e6 * s["fit_kernel_ms"] / (poses * LASER.n_beams))
    reference, moving = Mapper(LASER), Mapper(LASER)
    for i in range(n):
        reference.Process(ranges[i], odom[i], 0.1 * i)
    moving.Process(query, odom[n], 0.0)
    mg = MapMerger(RES)
    ids = [mg.add_submap(reference), mg.add_submap(moving)]
    cands = np.zeros((poses, 3))
    cands[1:, :2] = rng.uniform(-0.5, 0.5, size=(poses - 1, 2))
    cands[1:, 2] = rng.uniform(-0.1, 0.1, size=poses - 1)
    merged = []
    for k in range(a.rounds + 1):
        mg.fit(ids[1], cands)
        st = mg.fit_stats()
        merged.append(1e3 * st["kernel_us"] / st["beam_candidates"])
    record["b_fit"] = {"poses": poses, "k_map_fit_ns_per_beam_per_pose": spread(per_beam[1:]),
                       "k_occ_fit_merged_ns_per_beam_per_candidate": spread(merged[1:]),
                       "ratio": float(np.median(per_beam[1:]) / np.median(merged[1:]))}
    print("b", record["b_fit"], flush=True)
    mg.close(); moving.close()

    # (c) tracking: one step per scan, against ProcessLocalization behind the same scans
    step_ms, responses, errors = [], [], []
    for k in range(a.rounds + 1):
        loc.set_pose(truth[n - 1], odom[n - 1])
        ms = []
        for i in range(n, n + TRACK):
            t0 = time.perf_counter()
            step = loc.process(ranges[i], odom[i])
            ms.append((time.perf_counter() - t0) * 1e3)
            if k == a.rounds:
                responses.append(step.response)
                errors.append(float(np.hypot(*(step.robot_pose[:2] - truth[i, :2]))))
        step_ms.append(float(np.median(ms)))
    ms = []
    for i in range(n, n + TRACK):
        t0 = time.perf_counter()
        ok = reference.ProcessLocalization(ranges[i], odom[i], 0.1 * i)[0]
        dt = (time.perf_counter() - t0) * 1e3
        if ok:
            ms.append(dt)
    record["c_tracking"] = {"steps": TRACK, "process_ms_per_step": spread(step_ms[1:]), "response": spread(responses), "error_m": spread(errors),
                            "stats": loc.stats(), "mapper_process_localization_ms_per_scan": spread(ms)}
    print("c", {k: record["c_tracking"][k] for k in ("process_ms_per_step", "mapper_process_localization_ms_per_scan", "error_m")}, flush=True)
    reference.close(); loc.close(); grid.close()
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
