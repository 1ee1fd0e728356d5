"""Measures marginalizing node removal (kh_spa_marginalize_nodes, KH_REMOVE_MARGINALIZE) and writes profiles/marginalize_leg.json.

    python tools/marginalize_leg.py [--repeat 5] [--scans 3000]

  (a) the batch case the kernel is shaped for: ONE call over every third node of a 30 000-node chain-with-closures graph
      (synth.make_pose_graph(30000, 36000)), 10 000 nodes: rounds, constraints added / fused, and the split of the call into
      pack (rounds + packing on the host), kernel (upload + launch + download) and apply (the edits of the graph); beside it
      kh_spa_remove_node over the same 10 000 nodes of the same graph.  Medians over --repeat fresh solvers after one warm-up.
  (b) the per-scan case: the lifelong circuit replay of --scans scans (replay.run) under plain and under marginalizing removal:
      scans/s, components of the graph that is left, map IoU against the map from the true poses, node-decay time per removed
      node.  Here every removing scan pays a launch and a download of its own: latency, not throughput.

No threshold is applied."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, replay, synth  # noqa: E402
from slam_toolbox_amd.scan_solver import HipSpaSolver  # noqa: E402


def med(v):
    return float(np.median(v))


def batch(repeat, n=30000, e=36000):
    g = synth.make_pose_graph(n, e, seed=12345)
    ids = np.arange(1, n, 3, dtype=np.int32)[:10000]
    rows = {k: [] for k in ("wall_ms", "pack_ms", "kernel_ms", "apply_ms", "total_ms", "plain_remove_wall_ms")}
    summ = None
    for rep in range(-1, repeat):
        sol = HipSpaSolver()
        sol.load(g["init"], g["edges"], g["z"], g["cov"])
        t0 = time.perf_counter()
        summ = sol.MarginalizeNodes(ids)
        wall = (time.perf_counter() - t0) * 1e3
        left = capi.lib().kh_spa_num_constraints(sol._h)
        sol.close()
        sol = HipSpaSolver()
        sol.load(g["init"], g["edges"], g["z"], g["cov"])
        t0 = time.perf_counter()
        for v in ids:
            sol.RemoveNode(int(v))
        plain = (time.perf_counter() - t0) * 1e3
        sol.close()
        print(f"[marginalize_leg] batch round {rep}: {summ['n_rounds']} rounds, call {wall:.1f} ms, plain removal {plain:.1f} ms", flush=True)
        if rep >= 0:
            rows["wall_ms"].append(wall)
            rows["plain_remove_wall_ms"].append(plain)
            for k in ("pack_ms", "kernel_ms", "apply_ms", "total_ms"):
                rows[k].append(summ[k])
    out = {k: med(v) for k, v in rows.items()}
    out.update(nodes=n, edges=int(len(g["edges"])), listed=int(ids.size), constraints_left=int(left),
               **{k: summ[k] for k in ("n_marginalized", "n_plain", "n_rounds", "n_added", "n_fused", "max_degree")})
    out["us_per_node"] = out["total_ms"] * 1e3 / ids.size
    return out


def lifelong(n_scans):
    out = {}
    for name, marg in (("plain", False), ("marginalize", True)):
        r = replay.run(n_scans, lifelong=True, marginalize=marg, queue=replay.LapQueue(n_scans), progress=500)
        st = r["stats"]
        out[name] = dict(scans_per_s=r["scans_per_s"], alive=r["alive"], graph_components=r["graph_components"],
                         graph_largest_components=r["graph_largest_components"], map_iou_vs_truth_poses=r["map_iou_vs_truth_poses"],
                         aligned_map_iou_vs_truth_poses=r["aligned"]["map_iou_vs_truth_poses"], pose_error_xy_rms_m=r["pose_error_xy_rms_m"],
                         loop_closures=st["loop_closures"], nodes_removed=st["nodes_removed"], marginalize_fallbacks=st["marginalize_fallbacks"],
                         lifelong_ms=st["lifelong_ms"], process_ms=st["process_ms"],
                         lifelong_ms_per_removed_node=st["lifelong_ms"] / max(1, st["nodes_removed"]))
    out["scans"] = n_scans
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--scans", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginalize_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("marginalize_leg needs a GPU: nothing here is measured without one")
    result = dict(repeat=args.repeat, batch=batch(args.repeat), lifelong=lifelong(args.scans))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
