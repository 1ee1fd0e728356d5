"""Measures the visibility analysis of a map (kh_map_visibility_*) and writes profiles/map_visibility_leg.json.

    python tools/map_visibility_leg.py [--scans 1500] [--rounds 10]

The map is tools/map_raycast_leg.py's: the occupancy grid of --scans synthetic scans of the lap trajectory at 0.05 m (521 x 802 cells
for 1500), the laser the synthetic one (1081 beams, reach 402 cells: a bitmap of 79 KB).  On one GPU, in one process:

  (a) k_vis_gain per beam and pose (device events) over the poses of map_raycast_leg -- the fine means of a relocalization of the
      held-out scan -- against k_map_raycast on the SAME poses at the same budget: the walk is the same, the difference is the LDS ORs
      and the count pass; with the read-before-OR skip and without; one pose per launch;
  (b) a commit of those poses and of one pose (kernel by events, call by wall time);
  (c) a select of k = 8 from the map's frontier anchors at 4 headings: the call (wall), its kernels (events), and the same launches
      timed apart -- a gain over the candidates, a commit of one pose; best is what is left of a round;
  (d) for context only, tests/map_visibility_rule.py's select on the host over the first --rule-candidates candidates.

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
from slam_toolbox_amd.map_localizer import MapLocalizer, map_raycast  # noqa: E402
from slam_toolbox_amd.map_visibility import MapVisibility  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402
from slam_toolbox_amd.scan_matcher import LocalizedRangeScan  # noqa: E402

LASER = synth.Laser()
RES = 0.05
OPEN = dict(minimum_response_coarse=-1.0, maximum_variance_coarse=1e30, minimum_response_fine=-1.0, merge_distance=0.0)
BUDGET = 20


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
    ap.add_argument("--rule-candidates", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_visibility_leg.json"))
    a = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise SystemExit("map_visibility_leg needs a GPU")
    n = a.scans
    world, rng = synth.make_world(12345), np.random.default_rng(4)
    truth, _ = synth.trajectory_laps(n + 1)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(n + 1)]
    grid = OccupancyGrid.CreateFromScans([LocalizedRangeScan(r, p, LASER.min_angle, LASER.ang_res) for r, p in zip(ranges[:n], truth[:n])], RES, LASER)
    loc = MapLocalizer(None, LASER, max_batch=64).set_map(grid)
    hyps, _ = loc.relocalize(ranges[n], cap=4096, center_xy=tuple(truth[n, :2]), radius=6.0, top_k=0, **OPEN)
    poses = np.array([h.fine_mean for h in hyps])
    vis = loc.visibility(max_unknown=BUDGET)
    record = {"resolution": RES, "rounds": a.rounds, "n_scans": n, "width": grid.width, "height": grid.height, "n_beams": LASER.n_beams, "max_unknown": BUDGET,
              "reach": vis.stats["reach"], "bitmap_bytes": vis.stats["bitmap_bytes"], "n_poses": int(len(poses))}
    per = 1e6 / (len(poses) * LASER.n_beams)

    # (a) the gain against the cast
    gain_ns, every_or_ns, cast_ns, one_ns, gain_call, seen = [], [], [], [], [], None
    for _ in range(a.rounds + 1):
        vis.set_skip(True)
        gain_call.append(wall_ms(lambda: vis.gain(poses)))
        gain_ns.append(vis.kernel_ms * per)
        seen = vis.gain(poses)
        vis.set_skip(False)
        vis.gain(poses)
        every_or_ns.append(vis.kernel_ms * per)
        vis.set_skip(True)
        cast_ns.append(map_raycast(grid, LASER, poses, BUDGET).kernel_ms * per)
        one = []
        for p in poses[:32]:
            vis.gain(p)
            one.append(vis.kernel_ms)
        one_ns.append(1e6 * np.median(one) / LASER.n_beams)
    cells = seen["seen_free"].astype(np.int64) + seen["seen_occupied"] + seen["seen_unknown"]
    record["a_gain"] = {"k_vis_gain_ns_per_beam_per_pose": spread(gain_ns[1:]), "k_vis_gain_every_or_ns_per_beam_per_pose": spread(every_or_ns[1:]),
                        "k_map_raycast_ns_per_beam_per_pose": spread(cast_ns[1:]), "ratio_gain_to_cast": float(np.median(gain_ns[1:]) / np.median(cast_ns[1:])),
                        "ratio_every_or_to_skip": float(np.median(every_or_ns[1:]) / np.median(gain_ns[1:])),
                        "k_vis_gain_ns_per_beam_1_pose_per_launch": spread(one_ns[1:]), "gain_call_ms": spread(gain_call[1:]),
                        "seen_cells_per_pose": spread(cells), "seen_unknown_per_pose": spread(seen["seen_unknown"])}
    print("a_gain", record["a_gain"], flush=True)

    # (b) commits
    many_ms, many_call, one_ms, one_call = [], [], [], []
    for _ in range(a.rounds + 1):
        vis.clear()
        many_call.append(wall_ms(lambda: vis.commit(poses)))
        many_ms.append(vis.stats["kernel_ms"])
        vis.clear()
        one_call.append(wall_ms(lambda: vis.commit(poses[:1])))
        one_ms.append(vis.stats["kernel_ms"])
    record["b_commit"] = {"all_poses_kernel_ms": spread(many_ms[1:]), "all_poses_call_ms": spread(many_call[1:]), "one_pose_kernel_ms": spread(one_ms[1:]),
                          "one_pose_call_ms": spread(one_call[1:])}
    print("b_commit", record["b_commit"], flush=True)

    # (c) a select of 8 from the frontier anchors
    field = MapField(grid, max_distance=2.0)
    regions = field.regions(min_clearance=0.2)
    candidates = MapVisibility.candidates(regions, n_headings=4)
    frontiers = regions.frontiers
    regions.close(); field.close()
    k = min(8, len(candidates))
    call, kernels, gain_ms, commit_ms, picks, gains = [], [], [], [], None, None
    for _ in range(a.rounds + 1):
        vis.clear()
        vis.gain(candidates)
        gain_ms.append(vis.kernel_ms)
        vis.commit(candidates[:1])
        commit_ms.append(vis.stats["kernel_ms"])
        vis.clear()
        t = time.perf_counter()
        picks, gains = vis.select(candidates, k)
        call.append(1e3 * (time.perf_counter() - t))
        kernels.append(vis.stats["kernel_ms"])
    record["c_select"] = {"n_frontiers": len(frontiers), "n_candidates": int(len(candidates)), "k": k, "picks": picks.tolist(), "pick_gains": gains.tolist(),
                          "call_ms": spread(call[1:]), "kernels_ms": spread(kernels[1:]), "one_gain_launch_ms": spread(gain_ms[1:]),
                          "one_commit_launch_ms": spread(commit_ms[1:]),
                          "best_and_gaps_ms_per_round": float((np.median(kernels[1:]) - k * (np.median(gain_ms[1:]) + np.median(commit_ms[1:]))) / max(1, k))}
    print("c_select", record["c_select"], flush=True)

    # (d) the rule on the host, for context
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import map_visibility_rule as rule
        from oracle import karto
        karto.lib()
        few = candidates[:a.rule_candidates]
        cells = grid.cells()
        view = dict(cells=cells, width=grid.width, height=grid.height, ox=0, oy=0, anchor=(float(grid.offset[0]), float(grid.offset[1])), scale=float(grid.view().scale))
        host = rule.Visibility(view, LASER, max_unknown=BUDGET)
        t = time.perf_counter()
        want = host.select(few, min(k, len(few)))
        rule_ms = 1e3 * (time.perf_counter() - t)
        vis.clear()
        got = vis.select(few, min(k, len(few)))
        record["d_rule_host"] = {"n_candidates": int(len(few)), "k": min(k, len(few)), "select_ms": rule_ms,
                                 "equals_device": bool(got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist())}
    except Exception as e:                                     # the oracle is a test dependency: the leg stands without it
        record["d_rule_host"] = f"not run: {type(e).__name__}: {e}"
    print("d_rule_host", record["d_rule_host"], flush=True)
    vis.close(); loc.close(); grid.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out_file:
        json.dump(record, out_file, indent=1)
        out_file.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
