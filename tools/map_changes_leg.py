"""Measures the map change layer (kh_map_changes_*) and writes profiles/map_changes_leg.json.

    python tools/map_changes_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_match_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500).  On one GPU, in one process:

  (a) k_map_observe per beam (device events): the 64 scans behind the map at their true poses in ONE call, and one scan per call;
      against k_map_fit per beam and pose on the same map -- the hypotheses of a relocalization of the first of those scans with
      every gate open and no suppression (what tools/map_localize_leg.py measures), and one pose per launch (the tracking steps' fits)
  (b) a diff after those 64 scans: k_map_diff, the compaction (count, prefix, fill) and the downloads (counts, total, list), by
      device events, and the call's wall time
  (c) one kh_map_localizer_process step per scan over the same 64 scans (wall), without a layer and with one

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
from slam_toolbox_amd.map_localizer import MapLocalizer  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_changes_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_changes_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, odom = synth.trajectory_laps(n + TRACK)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n + TRACK)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(ranges[i], truth[i], LASER.min_angle, LASER.ang_res) for i in range(n)], RES, LASER)
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "n_beams": LASER.n_beams,
              "scans_observed": TRACK}
    layer = MapChanges(grid)
    loc = MapLocalizer(None, LASER, max_batch=64).set_map(grid)
    behind, poses = np.array(ranges[n:n + TRACK]), truth[n:n + TRACK]
    beams = TRACK * LASER.n_beams

    # (a) the observe kernel per beam, against the fit kernel per beam and pose
    batch, single, diffs, wall = [], [], [], []
    for k in range(a.rounds + 1):
        layer.clear()
        layer.observe(LASER, behind, poses)
        t0 = time.perf_counter()
        d = layer.diff()
        wall.append((time.perf_counter() - t0) * 1e3)
        batch.append(1e6 * d["observe_kernel_ms"] / beams)
        diffs.append(d)
        layer.clear()
        for i in range(TRACK):
            layer.observe(LASER, behind[i], poses[i])
        single.append(1e6 * layer.diff(cap=0)["observe_kernel_ms"] / beams)
    fit_batch, n_poses = [], 0
    region = dict(center_xy=tuple(truth[n, :2]), radius=6.0, top_k=0, **OPEN)
    for k in range(a.rounds + 1):
        _, s = loc.relocalize(ranges[n], cap=4096, **region)
        n_poses = s["n_accepted"]
        fit_batch.append(1e6 * s["fit_kernel_ms"] / (n_poses * LASER.n_beams))
    labels = layer.observe(LASER, behind, poses)
    record["a_observe"] = {"k_map_observe_ns_per_beam_64_scans_per_call": spread(batch[1:]),
                           "k_map_observe_ns_per_beam_1_scan_per_call": spread(single[1:]),
                           "k_map_fit_ns_per_beam_per_pose": spread(fit_batch[1:]), "k_map_fit_poses_per_launch": n_poses,
                           "ratio_64_scans_to_fit": float(np.median(batch[1:]) / np.median(fit_batch[1:])),
                           "labels": np.bincount(labels[:, :, 0].ravel(), minlength=6).tolist()}
    print("a", record["a_observe"], flush=True)

    # (b) the diff after 64 scans
    diffs = diffs[1:]
    record["b_diff"] = dict({k: spread([d[k] for d in diffs]) for k in ("diff_kernel_ms", "list_kernel_ms", "download_ms")},
                            call_wall_ms=spread(wall[1:]), counts=diffs[-1]["counts"].tolist(), n_changed=int(diffs[-1]["n_changed"]))
    print("b", record["b_diff"], flush=True)

    # (c) a tracking step without and with a layer
    def track(changes):
        step_ms, fit_ns = [], []
        for k in range(a.rounds + 1):
            loc.set_pose(truth[n - 1], odom[n - 1])
            if changes is not None:
                changes.clear()
            before, ms = loc.stats(), []
            for i in range(n, n + TRACK):
                t0 = time.perf_counter()
                loc.process(ranges[i], odom[i], changes=changes)
                ms.append((time.perf_counter() - t0) * 1e3)
            after = loc.stats()
            step_ms.append(float(np.median(ms)))
            fit_ns.append(1e6 * (after["fit_kernel_ms"] - before["fit_kernel_ms"]) / ((after["poses_fitted"] - before["poses_fitted"]) * LASER.n_beams))
        return step_ms[1:], fit_ns[1:]
    plain, fit_single = track(None)
    observed, _ = track(layer)
    record["c_tracking"] = {"steps": TRACK, "process_ms_per_step": spread(plain), "process_ms_per_step_with_layer": spread(observed),
                            "scans_observed_by_the_layer": int(layer.diff(cap=0)["scans_observed"])}
    record["a_observe"]["k_map_fit_ns_per_beam_1_pose_per_launch"] = spread(fit_single)
    record["a_observe"]["ratio_1_scan_to_fit_1_pose"] = float(np.median(single[1:]) / np.median(fit_single))
    print("c", record["c_tracking"], record["a_observe"]["k_map_fit_ns_per_beam_1_pose_per_launch"], flush=True)
    layer.close(); loc.close(); grid.close()
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
