"""Measures the covariance columns (kh_spa_compute_covariance_columns, kh_spa_get_relative_covariances) and writes
profiles/covariance_columns_leg.json.

    python tools/covariance_columns_leg.py [--repeat 20]

On the 10 000-node / 30 000-edge graph of the benchmark, solved first, one handle throughout:

  (a) the pass with 1, 16 and 64 query nodes (spread evenly over the free nodes): wall time of the call, the forward and the backward
      sweep alone (HIP events, kh_spa_set_debug bit 1), the fronts the forward sweep visited, the flops of the sweeps and the rate they
      give, and the share of the two sweeps in the call
  (b) the covariance pass of the same handle with no queries (kh_spa_compute_covariances)
  (c) k_cov_relative over all nodes against the first query (kh_spa_get_relative_covariances, wall: upload of the poses, the kernel,
      download of nine doubles per node) and the first getter of a column (its download)

(a) and (b) alternate inside one loop after a warm-up; medians over --repeat rounds.  No threshold is applied."""
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
QUERY_COUNTS = (1, 16, 64)


def med(v):
    return float(np.median(v))


def measure(repeat):
    g = synth.make_pose_graph(NODES, EDGES, seed=12345)
    sol = HipSpaSolver()
    sol.set_debug(phase_timing=True)
    sol.load(g["init"], g["edges"], g["z"], g["cov"])
    sol.Compute()
    keys = ("wall_ms", "forward_ms", "backward_ms", "total_ms", "relative_all_nodes_ms", "first_column_getter_ms")
    rows = {count: {k: [] for k in keys} for count in QUERY_COUNTS}
    plain = {"wall_ms": [], "total_ms": [], "inverse_ms": []}
    last = {}
    for rep in range(-3, repeat):                        # three warm-up rounds: code objects, first allocation of the buffers
        t0 = time.perf_counter()
        summ = sol.ComputeCovariances()
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= 0:
            plain["wall_ms"].append(wall)
            plain["total_ms"].append(summ["total_ms"])
            plain["inverse_ms"].append(summ["inverse_ms"])
        for count in QUERY_COUNTS:
            queries = [int(v) for v in np.linspace(1, NODES - 1, count).astype(np.int64)]
            t0 = time.perf_counter()
            summ = sol.ComputeCovarianceColumns(queries)
            wall = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            sol.CovarianceColumn(queries[0], [queries[0]])
            getter = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            sol.RelativeCovariances(queries[0])
            relative = (time.perf_counter() - t0) * 1e3
            last[count] = summ
            if rep >= 0:
                r = rows[count]
                r["wall_ms"].append(wall)
                for k in ("forward_ms", "backward_ms", "total_ms"):
                    r[k].append(summ[k])
                r["relative_all_nodes_ms"].append(relative)
                r["first_column_getter_ms"].append(getter)
    out = dict(nodes=NODES, edges=EDGES, n_free=last[1]["cov"]["n_free"], levels=last[1]["cov"]["levels"],
               no_queries={k: med(v) for k, v in plain.items()}, queries=[])
    for count in QUERY_COUNTS:
        r = {k: med(v) for k, v in rows[count].items()}
        sweeps = r["forward_ms"] + r["backward_ms"]
        r.update(n_queries=count, path_fronts=last[count]["path_fronts"], column_flops=last[count]["column_flops"],
                 column_gflops_per_s=last[count]["column_flops"] / max(sweeps, 1e-9) / 1e6,
                 sweeps_share_of_call=sweeps / max(r["total_ms"], 1e-9),
                 call_over_no_queries=r["total_ms"] / max(out["no_queries"]["total_ms"], 1e-9))
        out["queries"].append(r)
    sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_columns_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("covariance_columns_leg needs a GPU: nothing here is measured without one")
    result = dict(repeat=args.repeat, graph=measure(args.repeat))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
