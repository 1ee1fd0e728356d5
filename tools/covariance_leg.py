"""Measures the pose-graph covariance pass (kh_spa_compute_covariances) and writes profiles/covariance_leg.json.

    python tools/covariance_leg.py [--repeat 20]

On the 10 000-node / 30 000-edge graph of the benchmark and on a 1000 / 3000 graph, each solved first:

  (a) the pass: wall time of the call and the split of its summary -- linearisation, factorisation + downward pass + gather
      (wall), the downward pass and the collecting kernel alone (HIP events, kh_spa_set_debug bit 1), the flops of the downward
      pass and the rate they give
  (b) ONE factorisation of the same handle: the factor phase of a Compute() (kh_spa_summary.factor_gpu_ms / factorizations,
      HIP events), which the issue that asked for the pass expects it to cost about as much as
  (c) the first getter behind a pass (the download of the array and its pattern) and a getter after it

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

GRAPHS = ((10000, 30000), (1000, 3000))


def med(v):
    return float(np.median(v))


def measure(n, e, repeat):
    g = synth.make_pose_graph(n, e, seed=12345)
    sol = HipSpaSolver()
    sol.set_debug(phase_timing=True)
    sol.load(g["init"], g["edges"], g["z"], g["cov"])
    first = sol.Compute()
    rows = {k: [] for k in ("wall_ms", "linearize_ms", "factor_ms", "inverse_ms", "gather_ms", "total_ms", "one_factorization_gpu_ms",
                            "first_getter_ms", "next_getter_ms")}
    summ = None
    for rep in range(-3, repeat):                        # three warm-up rounds: code objects, first allocation of Z
        t0 = time.perf_counter()
        summ = sol.ComputeCovariances()
        wall = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        sol.Covariance(1)
        getter0 = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        sol.Covariance(2)
        getter1 = (time.perf_counter() - t0) * 1e3
        sol.ModifyNode(1, [g["init"][1][0], g["init"][1][1], 0.0])       # (a pose changed: the next Compute has work to do)
        c = sol.Compute()
        if rep >= 0:
            rows["wall_ms"].append(wall)
            for k in ("linearize_ms", "factor_ms", "inverse_ms", "gather_ms", "total_ms"):
                rows[k].append(summ[k])
            rows["one_factorization_gpu_ms"].append(c["factor_gpu_ms"] / max(1, c["factorizations"]))
            rows["first_getter_ms"].append(getter0)
            rows["next_getter_ms"].append(getter1)
    out = {k: med(v) for k, v in rows.items()}
    out.update(nodes=n, edges=e, n_free=summ["n_free"], levels=summ["levels"], inverse_flops=summ["inverse_flops"],
               factor_flops=first["factor_flops"],
               inverse_gflops_per_s=summ["inverse_flops"] / max(out["inverse_ms"], 1e-9) / 1e6,
               inverse_over_one_factorization=out["inverse_ms"] / max(out["one_factorization_gpu_ms"], 1e-9))
    sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("covariance_leg needs a GPU: nothing here is measured without one")
    result = dict(repeat=args.repeat, graphs=[measure(n, e, args.repeat) for n, e in GRAPHS])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
