"""Measures the ray cast and the map alignment (kh_map_raycast, kh_map_align) and writes
profiles/map_raycast_leg.json.

    python tools/map_raycast_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_match_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500).  On one GPU, in one process:

  (a) k_map_raycast per beam and pose (device events) against k_map_fit on the SAME poses: the fine means of a relocalization of the
      scan behind the map with every gate open and no suppression -- the fit kernel ran on them inside that call -- cast with no
      budget and with the alignment's budget of 20.  Both are read-only walks of a beam's line; the cast leaves at its first decision.
      And one pose per launch: what MapLocalizer.expected costs beside a tracking step's fit.
  (b) the split of an alignment: the same scans mapped once more with every pose carried by a rigid G, placed in the first map --
      seeds + cast, relocalizations, fits and the call (wall), and how far the first-ranked candidate lies from inverse(G).

Medians of --rounds rounds after a warm-up round.  No threshold is attached."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, synth  # noqa: E402
from slam_toolbox_amd.map_localizer import MapLocalizer, map_raycast  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES = 0.05
G = (0.73, -0.41, 0.3)
OPEN = dict(minimum_response_coarse=-1.0, maximum_variance_coarse=1e30, minimum_response_fine=-1.0, merge_distance=0.0)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def carried(pose, g=G):
    c, s = math.cos(g[2]), math.sin(g[2])
    return np.array([(c * pose[0] - s * pose[1]) + g[0], (s * pose[0] + c * pose[1]) + g[1], pose[2] + g[2]])


def grid_of(ranges, poses):
    return OccupancyGrid.CreateFromScans([LocalizedRangeScan(r, p, LASER.min_angle, LASER.ang_res) for r, p in zip(ranges, poses)], RES, LASER)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_raycast_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_raycast_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n + 1)]
    grid = grid_of(ranges[:n], truth[:n])
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "n_beams": LASER.n_beams}
    loc = MapLocalizer(None, LASER, max_batch=64).set_map(grid)

    # (a) the cast against the fit, per beam and pose, on the same poses
    region = dict(center_xy=tuple(truth[n, :2]), radius=6.0, top_k=0, **OPEN)
    fit_ns, cast_ns, cast20_ns, one_ns, one_fit_ns, poses, codes = [], [], [], [], [], None, None
    for k in range(a.rounds + 1):
        hyps, s = loc.relocalize(ranges[n], cap=4096, **region)
        poses = np.array([h.fine_mean for h in hyps])
        per = 1e6 / (len(poses) * LASER.n_beams)
        fit_ns.append(s["fit_kernel_ms"] * per)
        cast = map_raycast(grid, LASER, poses, -1)
        cast_ns.append(cast.kernel_ms * per)
        cast20_ns.append(map_raycast(grid, LASER, poses, 20).kernel_ms * per)
        codes = np.bincount(cast.codes.ravel(), minlength=3).tolist()
        one_ns.append(1e6 * np.median([loc.expected(p).kernel_ms for p in poses[:32]]) / LASER.n_beams)
        loc.set_pose(truth[n - 1])
        before = loc.stats()
        loc.process(ranges[n], truth[n - 1])
        one_fit_ns.append(1e6 * (loc.stats()["fit_kernel_ms"] - before["fit_kernel_ms"]) / LASER.n_beams)
    record["a_cast"] = {"poses_per_launch": int(len(poses)), "beams_by_code_free_hit_unknown": codes,
                        "k_map_raycast_ns_per_beam_per_pose": spread(cast_ns[1:]), "k_map_raycast_ns_per_beam_per_pose_budget_20": spread(cast20_ns[1:]),
                        "k_map_fit_ns_per_beam_per_pose": spread(fit_ns[1:]),
                        "ratio_cast_to_fit": float(np.median(cast_ns[1:]) / np.median(fit_ns[1:])),
                        "k_map_raycast_ns_per_beam_1_pose_per_launch": spread(one_ns[1:]),
                        "k_map_fit_ns_per_beam_1_pose_per_launch": spread(one_fit_ns[1:])}
    print("a", record["a_cast"], flush=True)

    # (b) the split of an alignment
    moving = grid_of(ranges[:n], [carried(p) for p in truth[:n]])
    times, got = [], None
    for k in range(a.rounds + 1):
        got, t = loc.align(moving)
        times.append(t)
    times = np.array(times[1:])
    best = got[0]
    ci, si = math.cos(-G[2]), math.sin(-G[2])
    inverse = np.array([-(ci * G[0] - si * G[1]), -(si * G[0] + ci * G[1]), -G[2]])
    centre = carried(np.array([grid.offset[0] + 0.5 * grid.width * RES, grid.offset[1] + 0.5 * grid.height * RES, 0.0]))
    off = carried(centre, best.correction)[:2] - carried(centre, inverse)[:2]
    record["b_align"] = {"moving_width": moving.width, "moving_height": moving.height, "n_candidates": len(got), "defaults": "3 probes, top_k 4, budget 20",
                         "seeds_and_cast_ms": spread(times[:, 0]), "relocalizations_ms": spread(times[:, 1]), "fits_ms": spread(times[:, 2]),
                         "call_ms": spread(times[:, 3]), "best_index": int(best.index), "best_score": float(best.fit["score"]),
                         "best_from_the_truth_m": float(math.hypot(off[0], off[1])), "best_from_the_truth_rad": float(abs(best.correction[2] - inverse[2]))}
    print("b", record["b_align"], flush=True)
    moving.close(); loc.close(); grid.close()
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
