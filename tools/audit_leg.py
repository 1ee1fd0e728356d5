"""Measures the constraint audit (kh_spa_audit_constraints) and writes profiles/audit_leg.json.

    python tools/audit_leg.py [--repeat 10]

On the 10 000-node / 30 000-edge graph of the benchmark, solved first, medians over --repeat rounds after a warm-up:

  (a) the covariance pass the audit rides on (kh_spa_compute_covariances of the same handle: wall time and the summary's total)
  (b) the audit on that resident pass: its two launches -- the audit's own linearisation of all edges and k_edge_audit -- between
      HIP events (kh_spa_set_debug bit 1), and the wall time of the call (launches, the download of 40 bytes per constraint, the
      records)
  (c) one rejection round as kh_mapper_reject_outliers runs it: Compute() + the pass + the audit + the download, after a pose was
      nudged so that the solve has work to do

No threshold is applied."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, synth  # noqa: E402
from slam_toolbox_amd.scan_solver import HipSpaSolver  # noqa: E402

NODES, EDGES = 10000, 30000


def med(v):
    return float(np.median(v))


def measure(repeat):
    g = synth.make_pose_graph(NODES, EDGES, seed=12345)
    sol = HipSpaSolver()
    sol.set_debug(phase_timing=True)
    sol.load(g["init"], g["edges"], g["z"], g["cov"])
    sol.Compute()
    rows = {k: [] for k in ("pass_wall_ms", "pass_total_ms", "audit_kernel_ms", "audit_wall_ms", "round_wall_ms", "round_solve_ms",
                            "round_pass_ms", "round_audit_kernel_ms")}
    rec = None
    for rep in range(-3, repeat):                        # three warm-up rounds: code objects, first allocations
        t0 = time.perf_counter()
        summ = sol.ComputeCovariances()
        pass_wall = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        rec = sol.AuditConstraints()
        audit_wall = (time.perf_counter() - t0) * 1e3
        a = sol.audit_summary
        assert a["cov"]["total_ms"] == 0.0               # (it rode on the pass above)
        sol.ModifyNode(1, [g["init"][1][0], g["init"][1][1], 0.0])       # (a pose changed: the next Compute has work to do)
        t0 = time.perf_counter()
        sol.Compute()
        solve = (time.perf_counter() - t0) * 1e3
        sol.AuditConstraints()
        round_wall = (time.perf_counter() - t0) * 1e3
        r = sol.audit_summary
        if rep >= 0:
            rows["pass_wall_ms"].append(pass_wall); rows["pass_total_ms"].append(summ["total_ms"])
            rows["audit_kernel_ms"].append(a["kernel_ms"]); rows["audit_wall_ms"].append(audit_wall)
            rows["round_wall_ms"].append(round_wall); rows["round_solve_ms"].append(solve)
            rows["round_pass_ms"].append(r["cov"]["total_ms"]); rows["round_audit_kernel_ms"].append(r["kernel_ms"])
    out = {k: med(v) for k, v in rows.items()}
    out.update(nodes=NODES, edges=EDGES, n_constraints=int(len(rec)), n_verifiable=int(rec["verifiable"].sum()),
               largest_chi2_loo=float(rec["chi2_loo"].max()),
               bytes_gathered_per_edge=8 * (21 + 27) + 4 * 4,
               audit_kernel_over_pass=out["audit_kernel_ms"] / max(out["pass_total_ms"], 1e-9))
    sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audit_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("audit_leg needs a GPU: nothing here is measured without one")
    result = dict(repeat=args.repeat, graph=measure(args.repeat))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
