"""Measures a distance field that follows its map (kh_map_field_update, kh_live_map_field_sync) and writes
profiles/live_field_leg.json.

    python tools/live_field_leg.py [--scans 1500] [--rounds 10]

On one GPU, in one process, two parts.

  kernels   on tools/map_field_leg.py's map (the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m, 521 x 802
            cells for 1500), field of 2 m (40 cells): a field from kh_map_field_create (k_field_columns and k_field_rows by events,
            the call by wall time), then its first update, which rebuilds by k_field_columns_band and k_field_rows_region over the whole
            window -- at the library's band height and at two others; k_field_changed over the whole unchanged window; the recount
  live      the lap queue through a mapper with a live map at 0.05 m and a field of 2 m that follows it: a sync after ONE new scan
            and after 25 new scans, each against kh_map_field_create on the same view (the only route before a field could follow),
            the syncs that came behind a loop closure (the live update found moved scans) summed up once more on their own, and the costs of the boxes a
            sync reports (costs_rect) against kh_map_field_costs of the window

Medians of --rounds rounds after a warm-up round; kernels by device events.  No threshold is attached: the record says what ran."""
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
from slam_toolbox_amd.mapper import Mapper  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES, DISTANCE = 0.05, 2.0


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)} if v.size else {"n": 0}


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t), out


def summary(rows):
    keys = sorted({k for r in rows for k in r} - {"rebuilt", "relayout"})
    return {"rounds": len(rows), "rebuilt_rounds": sum(r["rebuilt"] for r in rows), "rounds_with_moved_scans": sum(r["scans_moved"] > 0 for r in rows),
            **{k: spread([r[k] for r in rows if k in r]) for k in keys}}


def kernels_part(n, rounds):
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    scans = [LocalizedRangeScan(synth.make_scan(world, truth[i], rng), truth[i], LASER.min_angle, LASER.ang_res) for i in range(n)]
    grid = OccupancyGrid.CreateFromScans(scans, RES, LASER)
    record = {"width": grid.width, "height": grid.height, "cells": grid.width * grid.height, "radius_cells": 40}
    for band in (0, 16, 160):                                  # 0: the library's choice, max(R, 8) = 40
        t = {k: [] for k in ("k_field_columns_ms", "k_field_rows_ms", "create_call_ms", "k_field_columns_band_ms", "k_field_rows_region_ms", "rebuild_call_ms",
                             "k_field_changed_ms", "unchanged_update_call_ms", "recount_call_ms")}
        for _ in range(rounds + 1):
            f = MapField(grid, max_distance=DISTANCE)
            for k, v in zip(("k_field_columns_ms", "k_field_rows_ms", "create_call_ms"), f.stats["times_ms"]):
                t[k].append(v)
            f.set_band_rows(band)
            u = f.update(grid, stats=False)
            assert u["rebuilt"] == 1
            t["k_field_columns_band_ms"].append(u["times_ms"][1]); t["k_field_rows_region_ms"].append(u["times_ms"][2]); t["rebuild_call_ms"].append(u["times_ms"][3])
            t["recount_call_ms"].append(timed(f._read_stats)[0])
            u = f.update(grid, stats=False)
            assert u["rebuilt"] == 0 and u["cells_recomputed"] == 0 and u["cells_compared"] == record["cells"]
            t["k_field_changed_ms"].append(u["times_ms"][0]); t["unchanged_update_call_ms"].append(u["times_ms"][3])
            f.close()
        bands = (grid.height + (band or 40) - 1) // (band or 40)
        record[f"band_rows_{band or 'library_40'}"] = dict({k: spread(v[1:]) for k, v in t.items()}, bands=bands, waves=bands * ((grid.width + 255) // 256))
        print(band, record[f"band_rows_{band or 'library_40'}"], flush=True)
    grid.close()
    return record


def live_part(n_queue, rounds):
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_queue + 40 * (rounds + 2))
    rng = np.random.default_rng(4)
    m = Mapper(LASER, loop_search_maximum_distance=3.0)
    nxt = [0]

    def accept(k):
        got = 0
        while got < k:
            i = nxt[0]
            got += int(m.Process(synth.make_scan(world, truth[i], rng), odom[i], 0.1 * i)[0])
            nxt[0] += 1

    while nxt[0] < n_queue:
        accept(1)
    live = m.live_map(RES)
    live.update()
    field = live.field(max_distance=DISTANCE)
    record = {"scans_in_map": len(m.alive())}
    behind_closure = []                                        # the rounds of either kind whose live update found moved scans
    for name, k in (("one_new_scan", 1), ("25_new_scans", 25)):
        rows = []
        for rep in range(-1, rounds):
            accept(k)
            last = live.update()
            sync_ms, u = timed(lambda: field.sync(stats=False))
            create_ms, fresh = timed(lambda: MapField(live, max_distance=DISTANCE))
            info = live.info()
            window = info["width"] * info["height"]
            boxes = [b for b in (u["cells_box"], u["values_box"]) if b[2] > 0]
            row = {"sync_call_ms": sync_ms, "create_call_ms": create_ms, "create_kernels_ms": fresh.stats["times_ms"][0] + fresh.stats["times_ms"][1],
                   "sync_kernels_ms": sum(u["times_ms"][:3]), "k_field_changed_ms": u["times_ms"][0], "k_field_columns_band_ms": u["times_ms"][1],
                   "k_field_rows_region_ms": u["times_ms"][2], "window_cells": window, "cells_given_by_live_update": last["cells_updated"],
                   "cells_compared": u["cells_compared"], "cells_recomputed": u["cells_recomputed"], "rebuilt": u["rebuilt"], "relayout": u["relayout"],
                   "scans_moved": last["scans_moved"]}
            if boxes:
                x0, y0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
                x1, y1 = max(b[0] + b[2] for b in boxes), max(b[1] + b[3] for b in boxes)
                row["costs_rect_cells"] = (x1 - x0) * (y1 - y0)
                row["costs_rect_call_ms"] = min(timed(lambda: field.costs_rect(x0, y0, x1 - x0, y1 - y0))[0] for _ in range(3))
                row["costs_call_ms"] = min(timed(field.costs)[0] for _ in range(3))
            assert np.array_equal(field.d2, fresh.d2), "the followed field differs from a fresh one"
            fresh.close()
            if rep < 0:
                continue
            rows.append(row)
            if last["scans_moved"]:
                behind_closure.append(row)
        record[name] = summary(rows)
        print(name, record[name], flush=True)
    record["behind_a_loop_closure"] = summary(behind_closure)
    print("behind a closure", record["behind_a_loop_closure"], flush=True)
    info = live.info()
    record.update(width=info["width"], height=info["height"], scans_in_map_at_the_end=len(m.alive()))
    field.close(); live.close(); m.close()
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_field_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("live_field_leg needs a GPU")
    record = {"resolution": RES, "max_distance": DISTANCE, "rounds": a.rounds, "n_scans": a.scans, "kernels": kernels_part(a.scans, a.rounds),
              "live": live_part(a.scans, a.rounds)}
    with open(a.out, "w") as out_file:
        json.dump(record, out_file, indent=1)
        out_file.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
