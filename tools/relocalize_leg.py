"""Measures global relocalization (kh_mapper_relocalize) on loaded sessions and writes profiles/relocalize_leg.json.

Per session size (about 250, 1500 and 10 000 scans of the warehouse trajectory, saved and loaded again): wall time of
Mapper.relocalize at the default parameters for a scan taken at a pose of the trajectory that is not in the map, turned away from
the trajectory's heading; the library's own split of the call -- seed and base kernels (HIP events), the enumeration as a whole
(kernels, downloads, the store's upload), the query scans built on the host (kh_scan_points per hypothesis), the match batches --
and next to it n_hypotheses / 34 k pairs/s, what the loop-closure batch figure of the README predicts.  The timed loop runs after
--warmup calls; medians of --repeats calls.

The maps are placed, not matched (use_scan_matching 0, the trajectory's true poses): what is measured is the relocalization, and
a 10 000-scan map takes minutes to build through the matcher.

    python tools/relocalize_leg.py [--sizes 250 1500 10000] [--repeats 7] [--warmup 2]"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import synth  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402

PAIRS_PER_SECOND = 34.0e3              # README: 256-chain loop-closure batch in 7.5 ms


def med(v):
    return float(np.median(np.asarray(v)))


def leg(n_scans, repeats, warmup, tmp):
    world = synth.make_world(12345)
    truth, _ = synth.trajectory(n_scans + 1)
    rng = np.random.default_rng(4)
    held = n_scans // 2
    m = Mapper(synth.Laser(), use_scan_matching=0, minimum_travel_distance=0.0, minimum_travel_heading=0.0, minimum_time_interval=0.0)
    for i in range(n_scans + 1):
        if i != held:
            m.Process(synth.make_scan(world, truth[i], rng), truth[i], 0.1 * i)
    path = os.path.join(tmp, f"relocalize_{n_scans}.khms")
    m.save(path)
    m.close()
    m = Mapper.load(path)
    true_pose = truth[held] + (0.0, 0.0, 0.9)
    query = synth.make_scan(world, true_pose, rng)
    out = {"scans_in_map": int(len(m.alive()))}
    wall, parts = [], []
    first = None
    for r in range(warmup + repeats):
        t0 = time.perf_counter()
        hyps, summary = m.relocalize(query)
        dt = (time.perf_counter() - t0) * 1e3
        if first is None:
            first = dt
        if r >= warmup:
            wall.append(dt)
            parts.append(summary)
    m.close()
    s = parts[-1]
    out.update({k: s[k] for k in ("n_seeds", "n_headings", "n_hypotheses", "n_passed", "n_accepted")})
    out["first_call_wall_ms"] = first                      # scans become resident on the device, buffers are allocated
    out["wall_ms"] = med(wall)
    split = {k: med([p[k] for p in parts]) for k in ("kernel_ms", "candidates_ms", "scans_ms", "batch_ms", "total_ms")}
    out["split_ms"] = {"cover_and_gather_kernels": split["kernel_ms"], "enumeration_wall": split["candidates_ms"],
                       "host_scan_building": split["scans_ms"], "match_batches": split["batch_ms"], "call_total": split["total_ms"]}
    out["expected_ms_from_34k_pairs_per_s"] = s["n_hypotheses"] / PAIRS_PER_SECOND * 1e3
    out["wall_over_expected"] = out["wall_ms"] / out["expected_ms_from_34k_pairs_per_s"] if s["n_hypotheses"] else None
    shares = {k: out["split_ms"][k] for k in ("enumeration_wall", "host_scan_building", "match_batches")}
    out["dominant_part"] = max(shares, key=shares.get)
    if hyps:
        best = hyps[0]
        out["best"] = {"seed_scan": best.seed_scan, "fine_response": best.fine_response,
                       "distance_to_true_pose_m": math.hypot(best.robot_pose[0] - true_pose[0], best.robot_pose[1] - true_pose[1])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[250, 1500, 10000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relocalize_leg.json"))
    a = ap.parse_args()
    result = {"tool": "tools/relocalize_leg.py", "repeats": a.repeats, "warmup": a.warmup, "pairs_per_second_of_the_batch": PAIRS_PER_SECOND, "legs": []}
    with tempfile.TemporaryDirectory() as tmp:
        for n in a.sizes:
            result["legs"].append(leg(n, a.repeats, a.warmup, tmp))
            print(json.dumps(result["legs"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
