"""Measures the footprint analysis of a map (kh_map_footprint_*) and writes profiles/map_footprint_leg.json.

    python tools/map_footprint_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_travel_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500), its distance field to 2 m; the footprint the 1.0 m x 0.6 m rectangle (reach 13 cells).  On one GPU, in one process:

  (a) k_footprint_poses (device events) over 4096 poses drawn from the map's free cells at random headings, per pose and per covered
      cell, and the check call (wall) -- against kh_map_field_clearance of the same 4096 points
      (call, wall: k_field_lookup's time by events is not exposed, so the two CALLS are what compares), the floor any per-pose reader
      of the field pays;
  (b) k_footprint_layer (device events) at H = 8, 16 and 32, max_status 0, and the layer call with and without the masks (wall) --
      against kh_map_field_costs over the same window (call, wall), a one-read-per-cell pass;
  (c) the create call, a recompute, and check_path over the 64 paths of the travel leg (wall, all 64 together);
  (d) for context only, tests/map_footprint_rule.py's check on the host over the first --rule-poses poses.

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
from slam_toolbox_amd.map_footprint import MapFootprint  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES = 0.05
RECTANGLE = [(0.5, 0.3), (-0.5, 0.3), (-0.5, -0.3), (0.5, -0.3)]


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
    ap.add_argument("--rule-poses", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_footprint_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_footprint_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(r, p, LASER.min_angle, LASER.ang_res) for r, p in zip(ranges, truth[:n])], RES, LASER)
    field = MapField(grid, max_distance=2.0)
    fp = MapFootprint(field, RECTANGLE)
    cells = grid.cells()[:, :grid.width]
    scale, anchor = float(grid.view().scale), (float(grid.offset[0]), float(grid.offset[1]))
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "footprint": RECTANGLE, "reach": fp.stats["reach"],
              "tile": [64, 16]}

    # (a) 4096 poses on free cells
    jj, ii = np.nonzero(cells == 255)
    pick = np.random.default_rng(7).choice(len(ii), 4096, replace=False)
    poses = np.stack([anchor[0] + ii[pick] / scale, anchor[1] + jj[pick] / scale, np.random.default_rng(8).uniform(-np.pi, np.pi, 4096)], axis=1)
    kernel, call, lookup_call, records = [], [], [], None
    for _ in range(a.rounds + 1):
        records = fp.check(poses)
        kernel.append(fp.stats["times_ms"][0])
        call.append(wall_ms(lambda: fp.check(poses)))
        lookup_call.append(wall_ms(lambda: field.clearance(poses[:, :2])))
    covered = int(records["n_cells"].astype(np.int64).sum())
    kernel_ms = np.array(kernel[1:])
    record["a_poses"] = {"n_poses": 4096, "covered_cells": covered, "covered_cells_per_pose": spread(records["n_cells"]),
                         "status_counts": np.bincount(records["status"], minlength=5).tolist(),
                         "k_footprint_poses_ms": spread(kernel_ms), "ns_per_pose": float(1e6 * np.median(kernel_ms) / 4096),
                         "ns_per_covered_cell": float(1e6 * np.median(kernel_ms) / covered),
                         "check_call_ms": spread(call[1:]), "clearance_4096_call_ms": spread(lookup_call[1:]),
                         "ratio_check_call_to_clearance_call": float(np.median(call[1:]) / np.median(lookup_call[1:]))}
    print("a_poses", record["a_poses"], flush=True)

    # (b) the layer
    record["b_layer"] = {}
    costs_call = [wall_ms(lambda: field.costs()) for _ in range(a.rounds + 1)]
    for h in (8, 16, 32):
        kernel_ms, with_masks, summary_only, summary = [], [], [], None
        for _ in range(a.rounds + 1):
            with_masks.append(wall_ms(lambda: fp.layer(h, 0)))
            kernel_ms.append(fp.stats["times_ms"][1])
            t = time.perf_counter()
            _, summary = fp.layer(h, 0, masks=False)
            summary_only.append(1e3 * (time.perf_counter() - t))
        record["b_layer"][f"H_{h}"] = {"k_footprint_layer_ms": spread(kernel_ms[1:]), "ns_per_cell_and_heading": float(1e6 * np.median(kernel_ms[1:]) / (grid.width * grid.height * h)),
                                       "layer_call_ms": spread(with_masks[1:]), "layer_call_summary_only_ms": spread(summary_only[1:]),
                                       "stencil_rows": fp.stats["layer_rows"], "n_any": summary["n_any"], "n_all": summary["n_all"],
                                       "n_fit": [int(v) for v in summary["n_fit"]]}
    record["b_layer"]["costs_call_ms"] = spread(costs_call[1:])
    print("b_layer", record["b_layer"], flush=True)

    # (c) the handle's calls and the travel leg's 64 paths
    create, recompute = [], []
    for _ in range(a.rounds + 1):
        t = time.perf_counter()
        other = MapFootprint(field, RECTANGLE)
        create.append(1e3 * (time.perf_counter() - t))
        recompute.append(wall_ms(lambda: other.recompute(field)))
        other.close()
    travel = field.travel(goal_snap_cells=4)
    xy = np.asarray(truth[:n], dtype=np.float64)[:, :2]
    travel.solve(xy[:1])
    paths = travel.paths(xy[::max(1, n // 64)][:64], 4, 8192)
    travel.close()
    first = []

    def all_paths():
        first.clear()
        for p in paths:
            first.append(fp.check_path(p.xy)[1] if len(p.xy) else -1)
    path_ms = [wall_ms(all_paths) for _ in range(a.rounds + 1)]
    record["c_calls"] = {"create_call_ms": spread(create[1:]), "recompute_call_ms": spread(recompute[1:]), "check_path_64_paths_ms": spread(path_ms[1:]),
                         "path_poses": int(sum(len(p.xy) for p in paths)), "paths_blocked": int(sum(1 for k in first if k >= 0))}
    print("c_calls", record["c_calls"], flush=True)

    # (d) the rule on the host, for context
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import map_footprint_rule as rule
        view = dict(cells=grid.cells(), width=grid.width, height=grid.height, ox=0, oy=0, anchor=anchor, scale=scale)
        few = poses[:a.rule_poses]
        d2 = field.d2
        t = time.perf_counter()
        want = rule.check(view, d2, RECTANGLE, few)
        rule_ms = 1e3 * (time.perf_counter() - t)
        record["d_rule_host"] = {"n_poses": int(len(few)), "check_ms": rule_ms, "equals_device": bool(want.tobytes() == fp.check(few).tobytes())}
    except Exception as e:                                     # the oracle is a test dependency: the leg stands without it
        record["d_rule_host"] = f"not run: {type(e).__name__}: {e}"
    print("d_rule_host", record["d_rule_host"], flush=True)
    fp.close(); field.close(); grid.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out_file:
        json.dump(record, out_file, indent=1)
        out_file.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
