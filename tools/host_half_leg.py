"""Measures the host half of the headline step (256 config-2 CorrelateScans through kh_matcher_correlate_batch) and writes
profiles/host_half_leg.json.

    python tools/host_half_leg.py --tag parent                      # wall and process CPU-seconds per step
    python tools/host_half_leg.py --tag parent --stage-split        # additionally a child with KH_MATCH_TIMING=1: the library's own
                                                                    # prepare / enqueue / wait / finalise split per chunk size
    python tools/host_half_leg.py --tag parent --trace DIR          # additionally the drain-plus-fill gap from a kernel trace that
                                                                    # `rocprofv3 --kernel-trace --output-format csv -d DIR` left

KH_LIBRARY picks another build of the library (tools/build_variant.sh).  Records of several tags are kept side by side in the file.
The step is bench.py's: the same 256 pairs, the same search, one handle.  process_time() counts every thread of the process, so the
worker pool's spinning is in the figure."""
import argparse
import csv
import glob
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 256
CORR = ((0.15, 0.15), (0.005, 0.005), math.radians(20.0), math.radians(0.5))


def make_step():
    from concurrent.futures import ThreadPoolExecutor
    from common import C2_PARAMS, PRESETS, Scenario
    from slam_toolbox_amd.scan_matcher import MapperParams, ScanMatcher, _scan_array

    def one(b):
        sc = Scenario(seed=b, start=(37 * b) % 380, perturb=(0.04 * math.sin(b), -0.03 * math.cos(b), 0.01 * (b % 5 - 2)), n_base=10)
        q, base = sc.hip_scans()
        return q, sc.query_pose, base
    with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        made = list(pool.map(one, range(B)))
    queries = [q for q, _, _ in made]
    centers = np.asarray([c for _, c, _ in made])
    h = ScanMatcher.Create(MapperParams(**C2_PARAMS), *PRESETS["C2"]["create"], device=0, max_batch=B)
    for b in range(B):
        h.AddScans(queries[b], made[b][2], slot=b)
    arr = (_scan_array(queries), B)

    def step(_keep=made):                              # (the scan array points into the scans' own arrays: they live as long as the step)
        return h.CorrelateScanBatch(None, centers, *CORR, True, False, scan_array=arr)
    return h, step


def run_steps(steps, warmup, windows=5):
    h, step = make_step()
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.5:
        step()
    for _ in range(warmup):
        step()
    wall, cpu = [], []
    for _ in range(windows):
        w0, c0 = time.perf_counter(), time.process_time()
        for _ in range(steps):
            resp, _, _, status = step()
        wall.append((time.perf_counter() - w0) / steps * 1e3)
        cpu.append((time.process_time() - c0) / steps)
    assert (status == 0).all() and (resp > 0.1).all(), "matches failed"
    h.close()
    return {"steps_per_window": steps, "windows": windows, "ms_per_step_windows": wall, "ms_per_step_median": float(np.median(wall)),
            "cpu_seconds_per_step_windows": cpu, "cpu_seconds_per_step_median": float(np.median(cpu)),
            "cpus_busy_median": float(np.median(np.asarray(cpu) / (np.asarray(wall) * 1e-3))),
            "cpus_allowed": len(os.sched_getaffinity(0))}


def stage_split(steps, warmup):
    """a child of its own with KH_MATCH_TIMING=1: the library prints its split every 64 chunks; the lines are averaged per chunk size"""
    env = dict(os.environ, KH_MATCH_TIMING="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps-only", "--steps", str(steps), "--warmup", str(warmup)],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    pat = re.compile(r"\[kh match\] per call: prepare ([\d.]+) ms, enqueue ([\d.]+) ms, wait ([\d.]+) ms, finalize ([\d.]+) ms \(n = (\d+), stage (\d+) B/job\)")
    rows = [tuple(float(v) for v in m.groups()) for m in pat.finditer(run.stderr)]
    if run.returncode != 0 or not rows:
        return {"returncode": run.returncode, "stderr_tail": run.stderr[-2000:]}
    a = np.asarray(rows)
    # (a line is the mean over the 64 chunks in front of it, of all sizes: the split is per chunk, not per chunk size)
    return {"lines": len(rows), "per_chunk_ms": {"prepare": float(a[:, 0].mean()), "enqueue": float(a[:, 1].mean()), "wait": float(a[:, 2].mean()),
                                                 "finalize": float(a[:, 3].mean())}, "stage_bytes_per_job": int(a[-1, 5])}


def trace_gap(directory, chunks_per_step=5):
    """drain plus fill: from the end of the last k_ties of a step to the start of the first k_offsets_lds of the next"""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                kind = "ties" if "k_ties" in name else "offsets" if "k_offsets_lds" in name else "score" if "k_score_lds" in name else None
                if kind:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
    rows.sort()
    ties = [r for r in rows if r[2] == "ties"]
    offsets = [r for r in rows if r[2] == "offsets"]
    if len(ties) < 2 * chunks_per_step or len(ties) != len(offsets):
        return {"error": "trace holds %d k_ties and %d k_offsets_lds launches" % (len(ties), len(offsets))}
    gaps, spans = [], []
    for s in range(len(ties) // chunks_per_step - 1):
        last_tie = ties[chunks_per_step * (s + 1) - 1]
        next_first = offsets[chunks_per_step * (s + 1)]
        gaps.append((next_first[0] - last_tie[1]) * 1e-3)
        spans.append((last_tie[1] - offsets[chunks_per_step * s][0]) * 1e-3)
    dur = {k: float(np.mean([(e - s) * 1e-3 for s, e, kk in rows if kk == k])) for k in ("offsets", "score", "ties")}
    return {"steps": len(gaps), "gap_us_median": float(np.median(gaps)), "gap_us_min": float(np.min(gaps)), "gap_us_max": float(np.max(gaps)),
            "first_offsets_to_last_ties_us_median": float(np.median(spans)), "mean_kernel_us": dur}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stage-split", action="store_true")
    ap.add_argument("--trace", default="", metavar="DIR")
    ap.add_argument("--steps-only", action="store_true", help="run the steps and print nothing (what the children and the traced run use)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_half_leg.json"))
    args = ap.parse_args()
    if args.steps_only:
        run_steps(args.steps, args.warmup, windows=1)
        return
    record = {"library": os.environ.get("KH_LIBRARY", "in-tree")}
    record.update(run_steps(args.steps, args.warmup))
    if args.stage_split:
        record["stage_split"] = stage_split(64, args.warmup)
    if args.trace:
        record["trace"] = trace_gap(args.trace)
    records = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            records = json.load(f)
    records[args.tag] = record
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
    print(json.dumps({args.tag: record}))


if __name__ == "__main__":
    main()
