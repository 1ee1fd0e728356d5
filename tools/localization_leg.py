"""Measures localization mode (kh_mapper_process_localization) against mapping mode (kh_mapper_process) and the near-by query
kernels, and writes profiles/localization_leg.json.

    python tools/localization_leg.py                  # the mapper legs + the query timings (wall and HIP events)
    python tools/localization_leg.py --kernel-trace   # additionally a run of its own under rocprofv3 --kernel-trace --stats
    python tools/localization_leg.py --queries-only   # (what the traced child runs)

Mapper legs, on the 500-scan and the 3000-scan lap queue: the first half goes through kh_mapper_process (the map); the second
half once through kh_mapper_process (mapping, the baseline: that path is unchanged) and once through ProcessLocalization on an
identically built map.  Per accepted scan: wall time; for the localization run the number of scans alive over time.
KH_MAPPER_TIMING=1 in the environment makes the mapper print its own host pieces (sync_graph, remove_node, ...) on destroy."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import synth  # noqa: E402
from slam_toolbox_amd.loop_search import MapperGraphSearch  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402


def queue(n_scans):
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_scans)
    rng = np.random.default_rng(4)
    ranges = np.ascontiguousarray(np.stack([synth.make_scan(world, truth[i], rng) for i in range(n_scans)]))
    return ranges, np.ascontiguousarray(odom)


def summary(ms):
    ms = np.asarray(ms)
    return {"scans": int(ms.size), "median_ms": float(np.median(ms)), "mean_ms": float(ms.mean()), "p95_ms": float(np.percentile(ms, 95)),
            "max_ms": float(ms.max())}


def mapper_leg(n_scans):
    ranges, odom = queue(n_scans)
    switch = n_scans // 2
    out = {"queue_scans": n_scans, "switch_at_queue_scan": switch}
    for mode in ("mapping", "localization"):
        m = Mapper(synth.Laser(), loop_search_maximum_distance=3.0)
        for i in range(switch):
            m.Process(ranges[i], odom[i], 0.1 * i)
        step = m.ProcessLocalization if mode == "localization" else m.Process
        before = m.stats()
        ms, alive = [], []
        for i in range(switch, n_scans):
            t0 = time.perf_counter()
            ok = step(ranges[i], odom[i], 0.1 * i)[0]
            dt = (time.perf_counter() - t0) * 1e3
            if ok:
                ms.append(dt)
                alive.append(len(m.alive()))
        st = m.stats()
        out[mode] = dict(summary(ms), alive_first=alive[0], alive_last=alive[-1], alive_max=max(alive),
                         alive_every_50th=alive[::50], nodes_removed=st["nodes_removed"] - before["nodes_removed"],
                         loop_closures=st["loop_closures"] - before["loop_closures"],
                         match_ms=st["match_ms"] - before["match_ms"], solver_ms=st["solver_ms"] - before["solver_ms"])
        m.close()                                      # (prints the host pieces when KH_MAPPER_TIMING is set)
    return out


def query_leg(repeat=50):
    rng = np.random.default_rng(3)
    rows = []
    for n in (10000, 50000):
        pts = rng.uniform(-60.0, 60.0, size=(n, 2))
        g = MapperGraphSearch()
        g.SetGraph(pts, np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
        g.SetPoses(pts)
        for nq in (1, 256):
            q = rng.uniform(-60.0, 60.0, size=(nq, 2))
            g.FindNearByScan(q)
            wall, dev = [], []
            for _ in range(repeat):
                t0 = time.perf_counter()
                g.FindNearByScan(q)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(g.last_near_by_kernel_ms())
            rows.append({"vertices": n, "queries": nq, "wall_median_ms": float(np.median(wall)), "event_median_ms": float(np.median(dev))})
        t0 = time.perf_counter()
        for _ in range(repeat):
            hits = g.FindNearByVertices(q[0], 25.0)
        rows.append({"vertices": n, "radius_hits": int(hits.size), "wall_mean_ms": (time.perf_counter() - t0) * 1e3 / repeat,
                     "event_ms": g.last_near_by_kernel_ms()})
        g.close()
    return rows


def kernel_trace():
    """the query leg once more, in a child of its own under rocprofv3 --kernel-trace --stats; the near-by rows of its kernel stats"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="localization_leg_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "near_by", "--", sys.executable,
           os.path.abspath(__file__), "--queries-only"]
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    rows = []
    for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "near_by" in r.get("Name", "")]
    shutil.rmtree(tmp, ignore_errors=True)
    return {"returncode": run.returncode, "kernel_stats": rows} if rows else {"returncode": run.returncode, "output_tail": run.stdout[-2000:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--queries-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localization_leg.json"))
    args = ap.parse_args()
    if args.queries_only:
        print(json.dumps(query_leg()))
        return
    record = {"mapper": [mapper_leg(500), mapper_leg(3000)], "near_by_queries": query_leg()}
    if args.kernel_trace:
        record["near_by_kernel_trace"] = kernel_trace()
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
