"""Measures the travel costs of a map (kh_map_travel_*) and writes profiles/map_travel_leg.json.

    python tools/map_travel_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_field_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500), its field the default one (2 m: 40 cells).  On one GPU, in one process:

  a solve from one goal and from 16 goals (poses of the trajectory, snapped by 4 cells) at clearances of 0 and 4 cells: rounds, tile
  runs, launches, the weights, goals and relaxation kernels by device events, the solve and the create call (wall);
  the rounds_per_check sweep (1, 2, 4, 8, 16, 32) of the one-goal solve at clearance 0: the call's wall time is what the default is
  chosen by;
  64 paths from poses of the trajectory and a lookup of 4096 points (call, wall);
  for context, where scipy is installed, scipy.sparse.csgraph.dijkstra on the host over the same graph with the graph already built
  (its values are compared with the device's), and the region analysis' recompute on the same field.

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
from slam_toolbox_amd.map_travel import MapTravel  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES = 0.05
STEPS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
SOLVE_KEYS = ("n_traversable", "n_reached", "max_value", "rounds", "launches", "tile_runs")


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


def host_graph(q, connectivity=8):
    """the graph of the rule from the weights (cut_corners 0), as scipy wants it: an edge v -> u of weight L q(u) per allowed step u -> v"""
    from scipy import sparse
    h, w = q.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = q > 0
    at = lambda di, dj: pad[1 + dj:1 + dj + h, 1 + di:1 + di + w]  # noqa: E731
    rows, cols, data = [], [], []
    for n, (di, dj) in enumerate(STEPS[:connectivity]):
        ok = at(0, 0) & at(di, dj)
        if n >= 4:
            ok = ok & at(di, 0) & at(0, dj)
        jj, ii = np.nonzero(ok)
        rows.append((jj + dj) * w + ii + di); cols.append(jj * w + ii)
        data.append((5 if n < 4 else 7) * q[jj, ii].astype(np.float64))
    return sparse.csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(h * w, h * w))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_travel_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_travel_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(r, p, LASER.min_angle, LASER.ang_res) for r, p in zip(ranges, truth[:n])], RES, LASER)
    cells = grid.width * grid.height
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "cells": cells, "tile": [64, 16]}
    field = MapField(grid, max_distance=2.0)
    poses = np.asarray(truth[:n], dtype=np.float64)[:, :2]
    goals = {1: poses[:1], 16: poses[::max(1, n // 16)][:16]}

    for rc in (0, 4):
        for n_goals, xy in goals.items():
            kw = dict(min_clearance=max(0.0, rc - 0.5) * RES, goal_snap_cells=4)
            create, solve, times, last, status = [], [], [], None, None
            for _ in range(a.rounds + 1):
                t = time.perf_counter()
                tr = MapTravel(field, **kw)
                create.append(1e3 * (time.perf_counter() - t))
                t = time.perf_counter()
                status = tr.solve(xy)
                solve.append(1e3 * (time.perf_counter() - t))
                times.append(tr.stats["times_ms"][:3])
                last = dict(tr.stats)
                tr.close()
            times = np.asarray(times[1:])
            key = f"clearance_{rc}_cells_{n_goals}_goals"
            record[key] = {k: last[k] for k in SOLVE_KEYS}
            record[key].update(goals_ok=int((status == capi.KH_TRAVEL_GOAL_OK).sum()), k_travel_weights_ms=spread(times[:, 0]), k_travel_goals_ms=spread(times[:, 1]),
                               k_travel_relax_ms=spread(times[:, 2]), relax_us_per_launch=spread(1e3 * times[:, 2] / max(1, last["launches"])),
                               create_call_ms=spread(create[1:]), solve_call_ms=spread(solve[1:]))
            print(key, record[key], flush=True)

    tr = MapTravel(field, goal_snap_cells=4)
    sweep = {}
    for k in (1, 2, 4, 8, 16, 32):
        tr.set_rounds_per_check(k)
        calls, relax = [], []
        for _ in range(a.rounds + 1):
            calls.append(wall_ms(lambda: tr.solve(goals[1])))
            relax.append(tr.stats["times_ms"][2])
        sweep[str(k)] = {"solve_call_ms": spread(calls[1:]), "k_travel_relax_ms": spread(relax[1:]), "launches": tr.stats["launches"], "rounds": tr.stats["rounds"]}
    record["rounds_per_check_sweep"] = sweep
    print("sweep", sweep, flush=True)
    tr.set_rounds_per_check(0)
    tr.solve(goals[1])
    starts = poses[::max(1, n // 64)][:64]
    xy = rng.uniform(-1.0, 1.0, size=(4096, 2)) * 5.0 + poses[n // 2]
    lengths = [len(p.cells) for p in tr.paths(starts, 4, 8192)]
    calls = {"paths_64": lambda: tr.paths(starts, 4, 8192), "paths_64_heads_only": lambda: capi.lib().kh_map_travel_paths(
        tr._h, 64, np.ascontiguousarray(starts).ctypes.data, 4, 8192, (capi.KhTravelPath * 64)(), None), "lookup_1": lambda: tr.lookup(xy[:1]),
        "lookup_4096": lambda: tr.lookup(xy), "lookup_4096_snap_4": lambda: tr.lookup(xy, 4), "read_values": lambda: tr.values}
    record["readers_call_ms"] = {name: spread([wall_ms(fn) for _ in range(a.rounds + 1)][1:]) for name, fn in calls.items()}
    record["paths_64_cells"] = {"longest": int(max(lengths)), "total": int(sum(lengths))}
    print("readers", record["readers_call_ms"], record["paths_64_cells"], flush=True)
    values, weights = tr.values, tr.weights
    goal_cell, st = tr.lookup(goals[1], 4)[2][0], dict(tr.stats)
    tr.close()

    regions = MapRegions(field)
    record["regions_recompute_call_ms"] = spread([wall_ms(lambda: regions.recompute(field)) for _ in range(a.rounds + 1)][1:])
    regions.close()
    print("regions", record["regions_recompute_call_ms"], flush=True)
    try:
        from scipy.sparse.csgraph import dijkstra
        graph = host_graph(weights)
        source = int(goal_cell[1] - st["oy"]) * grid.width + int(goal_cell[0] - st["ox"])
        record["scipy_dijkstra_host_ms"] = spread([wall_ms(lambda: dijkstra(graph, directed=True, indices=[source], min_only=True)) for _ in range(max(2, a.rounds // 3))])
        dist = dijkstra(graph, directed=True, indices=[source], min_only=True)
        host = np.where(np.isinf(dist), capi.KH_TRAVEL_FAR, dist).astype(np.uint32).reshape(values.shape)
        assert values[source // grid.width, source % grid.width] == 0 and np.array_equal(host, values), "scipy's distances are the device's values"
        record["scipy_dijkstra_equals_device"] = True
    except ImportError:
        record["scipy_dijkstra_host_ms"] = "scipy is not installed"
    print("scipy", record["scipy_dijkstra_host_ms"], flush=True)
    field.close(); grid.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out_file:
        json.dump(record, out_file, indent=1)
        out_file.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
