"""Measures the merger's fit and automatic alignment (kh_merge_fit, kh_merge_align) and writes profiles/merge_fit_leg.json.

    python tools/merge_fit_leg.py [--scans 500] [--repeat 20] [--align-repeat 3]

The two sessions of tools/merge_leg.py (two circuits of the synth world, saved and loaded again); the second one is the moving
submap, the first one the reference:

  (a) kernel time per beam per candidate of the fit (k_occ_fit_merged) for 1, 8 and 64 candidates -- the identity and small
      motions about it, so every candidate's walks cross the reference grid -- HIP events (kh_merge_fit_stats)
  (b) kernel time per beam of k_occ_trace_merged over the SAME scans (a merger that holds the moving session alone): the same
      gate, rounding and walk, with two atomics per visit where the fit has one byte load.  Its grid is the moving session's
      own, which holds every visit; (a)'s grid is the reference session's, which drops the visits outside it -- so a_over_b
      compares walks clipped by different grids, and is a ratio of costs per beam, not per visit
  (c) wall time of one kh_merge_fit call per candidate count (reference grid, tables, kernel, download)
  (d) kh_merge_align at its defaults (4 probes, 4 hypotheses each, the whole target map): the relocalizations, the fit's reference
      grid, the fit kernel, the whole call

(a), (b) and (c) alternate inside one loop after a warm-up; medians over --repeat rounds.  No threshold is applied."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from merge_leg import RES, session, spread  # noqa: E402
from slam_toolbox_amd import capi  # noqa: E402
from slam_toolbox_amd.merge import MapMerger  # noqa: E402

COUNTS = (1, 8, 64)


def candidates(n):
    """the identity, then motions of up to 0.5 m and 0.1 rad about it"""
    rng = np.random.default_rng(5)
    c = np.zeros((n, 3))
    c[1:, :2] = rng.uniform(-0.5, 0.5, size=(n - 1, 2))
    c[1:, 2] = rng.uniform(-0.1, 0.1, size=n - 1)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=500)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--align-repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_fit_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("merge_fit_leg needs a GPU: nothing here is measured without one")
    with tempfile.TemporaryDirectory(prefix="merge_fit_leg_") as tmp:          # (a loaded mapper holds no reference to its file)
        mappers = [session(args.scans, (0, 1), 12345, tmp), session(args.scans, (1, 2), 777, tmp)]
    mg, alone = MapMerger(RES), MapMerger(RES)
    ids = [mg.add_submap(m) for m in mappers]
    alone.add_submap(mappers[1])
    fit_ns = {n: [] for n in COUNTS}
    fit_wall_ms = {n: [] for n in COUNTS}
    trace_ns = []
    for rep in range(-3, args.repeat):                     # three warm-up rounds: code objects, first uploads, allocator
        row = {}
        for n in COUNTS:
            t0 = time.perf_counter()
            out = mg.fit(ids[1], candidates(n))
            wall = (time.perf_counter() - t0) * 1e3
            st = mg.fit_stats()
            assert out[0]["known"] > 0 and st["beam_candidates"] > 0
            row[n] = (1e3 * st["kernel_us"] / st["beam_candidates"], wall)
        g = alone.merge()
        b = 1e6 * g.stats()["trace_ms"] / g.stats()["beams"]
        g.close()
        if rep >= 0:
            for n in COUNTS:
                fit_ns[n].append(row[n][0]); fit_wall_ms[n].append(row[n][1])
            trace_ns.append(b)
    splits = []
    for rep in range(-1, args.align_repeat):
        cands, times = mg.align(ids[1], ids[0])
        if rep >= 0:
            splits.append(times)
    info = mg.submap_info(ids[1])
    record = {"queue_scans_per_session": args.scans, "moving_scans": info["n_scans"], "moving_beams": info["n_scans"] * info["n_beams"],
              "reference_scans": mg.submap_info(ids[0])["n_scans"],
              "a_fit_ns_per_beam_per_candidate": {str(n): spread(fit_ns[n]) for n in COUNTS},
              "b_merged_trace_ns_per_beam": spread(trace_ns),
              "a_over_b": {str(n): float(np.median(fit_ns[n]) / np.median(trace_ns)) for n in COUNTS},
              "c_fit_call_wall_ms": {str(n): spread(fit_wall_ms[n]) for n in COUNTS},
              "d_align": {k: spread([s[k] for s in splits]) for k in ("relocalize_ms", "reference_grid_ms", "fit_kernel_ms", "total_ms")} if splits else None,
              "d_align_candidates": int(splits[-1]["n_candidates"]) if splits else None}
    mg.close(); alone.close()
    for m in mappers:
        m.close()
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
