"""Measures the region analysis of a map (kh_map_regions_*) and writes profiles/map_regions_leg.json.

    python tools/map_regions_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_field_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500), its field the default one (2 m: 40 cells).  On one GPU, in one process, for clearances of 0, 4 and 8 cells under both
connectivities:

  the six stages of an analysis by device events -- k_region_tiles; k_region_seams (one launch per set); k_region_flatten (one per
  set); the compaction (per set k_region_roots twice, the unit scan, k_region_ids); k_region_records; k_region_anchor -- and their
  sum; the whole create call and a recompute (wall); a lookup of 1 and of 4096 points and the read of an id grid (call, wall);
  beside them the field's own whole-window update on the same window (by its events and its call) and, where scipy is installed,
  scipy.ndimage.label of the two masks on the host.

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
from slam_toolbox_amd.map_regions import MapRegions  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES = 0.05
STAGES = ("k_region_tiles", "k_region_seams_x2", "k_region_flatten_x2", "compaction_x2", "k_region_records", "k_region_anchor")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_regions_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_regions_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(r, p, LASER.min_angle, LASER.ang_res) for r, p in zip(ranges, truth[:n])], RES, LASER)
    cells = grid.width * grid.height
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "cells": cells, "stages": list(STAGES)}
    field = MapField(grid, max_distance=2.0)

    for connectivity in (8, 4):
        for rc in (0, 4, 8):
            kw = dict(min_clearance=max(0.0, rc - 0.5) * RES, connectivity=connectivity)
            stages, create, recompute, last = [], [], [], None
            for _ in range(a.rounds + 1):
                t = time.perf_counter()
                r = MapRegions(field, **kw)
                create.append(1e3 * (time.perf_counter() - t))
                recompute.append(wall_ms(lambda: r.recompute(field)))
                stages.append(r.stats["times_ms"][:6])
                last = dict(r.stats)
                r.close()
            stages = np.asarray(stages[1:])
            key = f"N{connectivity}_clearance_{rc}_cells"
            record[key] = {k: last[k] for k in ("clearance_cells", "n_traversable", "n_frontier_cells", "n_total", "n_kept", "truncated")}
            record[key].update({name + "_ms": spread(stages[:, k]) for k, name in enumerate(STAGES)})
            record[key].update(kernels_sum_ms=spread(stages.sum(axis=1)), kernels_sum_ns_per_cell=spread(1e6 * stages.sum(axis=1) / cells),
                               create_call_ms=spread(create[1:]), recompute_call_ms=spread(recompute[1:]))
            print(key, record[key], flush=True)

    r = MapRegions(field)
    pose = np.asarray(truth[n // 2], dtype=np.float64)
    xy = rng.uniform(-1.0, 1.0, size=(4096, 2)) * 5.0 + pose[:2]
    calls = {"lookup_1": lambda: r.lookup(xy[:1]), "lookup_4096": lambda: r.lookup(xy), "read_region_ids": lambda: r.region_ids, "get_regions": lambda: r.regions}
    record["readers_call_ms"] = {name: spread([wall_ms(fn) for _ in range(a.rounds + 1)][1:]) for name, fn in calls.items()}
    print("readers", record["readers_call_ms"], flush=True)
    region_ids, frontier_ids, whole = r.region_ids, r.frontier_ids, not r.stats["truncated"][0]
    r.close()

    updates = [field.update(grid) for _ in range(a.rounds + 1)][1:]       # the whole window compared; nothing changed
    rebuilt = []
    for _ in range(a.rounds + 1):
        f = MapField(grid, max_distance=2.0)
        rebuilt.append(f.update(grid))                         # a field's first update recomputes the whole window
        f.close()
    record["field_update_same_window"] = {
        "compare_only_kernel_ms": spread([u["times_ms"][0] for u in updates]), "compare_only_call_ms": spread([u["times_ms"][3] for u in updates]),
        "rebuild_kernels_ms": spread([u["times_ms"][1] + u["times_ms"][2] for u in rebuilt[1:]]), "rebuild_call_ms": spread([u["times_ms"][3] for u in rebuilt[1:]])}
    print("field update", record["field_update_same_window"], flush=True)
    try:
        from scipy import ndimage
        eight = np.ones((3, 3))
        record["scipy_ndimage_label_host_ms"] = {
            "traversable_N8": spread([wall_ms(lambda: ndimage.label(region_ids != capi.KH_REGION_NONE, structure=eight)) for _ in range(a.rounds)]),
            "frontier_N8": spread([wall_ms(lambda: ndimage.label(frontier_ids != capi.KH_REGION_NONE, structure=eight)) for _ in range(a.rounds)])}
        if whole:
            labels = ndimage.label(region_ids != capi.KH_REGION_NONE, structure=eight)[0]
            assert np.array_equal(np.where(labels > 0, labels - 1, capi.KH_REGION_NONE).astype(np.uint32), region_ids), "scipy's numbering minus one"
    except ImportError:
        record["scipy_ndimage_label_host_ms"] = "scipy is not installed"
    print("scipy", record["scipy_ndimage_label_host_ms"], flush=True)
    field.close(); grid.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out_file:
        json.dump(record, out_file, indent=1)
        out_file.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
