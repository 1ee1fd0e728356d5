"""Measures the covariance gate of the loop search (kh_mapper_set_loop_gate) and writes
profiles/loop_gate_leg.json.

    python tools/loop_gate_leg.py [--sizes 250 1500 10000] [--tail 100] [--replay-scans 1500]

  (a) cost: a lap queue is replayed up to each graph size with the gate off (the parent behaviour); the mapper is saved there, and
      from that session the next --tail scans are processed with the gate off and with it on (defaults) at refresh_scans 1 / 10 /
      50: ms per scan (kh_mapper_stats.process_ms), column passes and their ms, the same box and the same queue for all four
  (b) kernel: k_loop_candidates gated against ungated on the graph store of each size, 64 queries per batch (HIP events,
      kh_graph_last_kernel_ms), medians
  (c) effect: the 4 % / 1 deg/m queue (LapQueue(drift_xy=0.02, drift_theta_deg=0.5)) replayed plain and gated: closures, chains
      the jump test rejected, pose error against the truth

No threshold is applied."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, replay  # noqa: E402
from slam_toolbox_amd.loop_search import MapperGraphSearch  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402

REFRESH = (1, 10, 50)


def med(v):
    return float(np.median(v))


def cost(sizes, tail):
    q = replay.LapQueue(max(sizes) + tail)
    ranges = [q.ranges(i) for i in range(q.n)]
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        m = Mapper(q.laser)
        done = 0
        for size in sorted(sizes):
            while done < size:
                m.Process(ranges[done], q.odom[done], 0.1 * done)
                done += 1
            path = os.path.join(tmp, f"at_{size}.khms")
            m.save(path)
            row = dict(scans=size, alive=int(len(m.alive())), variants=[])
            for refresh in (None,) + REFRESH:
                t = Mapper.load(path)
                if refresh is not None:
                    t.SetLoopGate(True, refresh_scans=refresh)
                before = t.stats()
                for i in range(size, size + tail):
                    t.Process(ranges[i], q.odom[i], 0.1 * i)
                st, gs = t.stats(), t.loop_gate_stats()
                n = max(1, st["scans_processed"] - before["scans_processed"])
                row["variants"].append(dict(gate="off" if refresh is None else "on", refresh_scans=refresh,
                                            ms_per_scan=(st["process_ms"] - before["process_ms"]) / n, scans=n,
                                            closures=st["loop_closures"] - before["loop_closures"], **gs))
                t.close()
            out.append(row)
        m.close()
    return out


def kernel(sizes, repeat):
    out = []
    rng = np.random.default_rng(5)
    for size in sizes:
        q = replay.LapQueue(size)
        xy = np.ascontiguousarray(q.truth[:, :2])
        ptr = np.zeros(size + 1, dtype=np.int32)
        ptr[1:] = np.cumsum([1] + [2] * (size - 2) + [1]) if size > 1 else 0
        idx = np.asarray([w for i in range(size) for w in ([i - 1] if i else []) + ([i + 1] if i + 1 < size else [])], dtype=np.int32)
        s = MapperGraphSearch()
        s.SetGraph(xy, ptr, idx)
        queries = np.linspace(0, size - 1, 64).astype(np.int32)
        L = np.tril(rng.uniform(-1, 1, size=(64, size, 3, 3)))
        gate = np.ascontiguousarray(L @ np.swapaxes(L, -1, -2))
        ms = {"ungated": [], "gated": []}
        for rep in range(-2, repeat):
            s.FindPossibleLoopClosures(queries, 3.0, 10)
            a = capi.lib().kh_graph_last_kernel_ms(s._h)
            s.find_loop_candidates(queries, 3.0, 10, gate=gate, chi2=5.991)
            b = capi.lib().kh_graph_last_kernel_ms(s._h)
            if rep >= 0:
                ms["ungated"].append(a)
                ms["gated"].append(b)
        s.close()
        out.append(dict(scans=size, queries=64, ungated_kernel_ms=med(ms["ungated"]), gated_kernel_ms=med(ms["gated"])))
    return out


def effect(n_scans):
    rows = []
    for gate in (None, {}):
        q = replay.LapQueue(n_scans, drift_xy=0.02, drift_theta_deg=0.5)
        r = replay.run(n_scans, lifelong=False, queue=q, loop_gate=gate)
        rows.append(dict(gate="off" if gate is None else "on (defaults)", closures=r["stats"]["loop_closures"],
                         loop_candidates=r["stats"]["loop_candidates"], pose_error_xy_rms_m=r["pose_error_xy_rms_m"],
                         pose_error_xy_max_m=r["pose_error_xy_max_m"], aligned_pose_error_xy_rms_m=r["aligned"]["pose_error_xy_rms_m"],
                         scans_per_s=r["scans_per_s"], loop_gate_stats=r.get("loop_gate_stats")))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[250, 1500, 10000])
    ap.add_argument("--tail", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--replay-scans", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_gate_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("loop_gate_leg needs a GPU: nothing here is measured without one")
    result = dict(sizes=args.sizes, tail=args.tail, cost=cost(args.sizes, args.tail), kernel=kernel(args.sizes, args.repeat),
                  effect=effect(args.replay_scans))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
