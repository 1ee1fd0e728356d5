"""Measures the session merge (kh_merge_build) and writes profiles/merge_leg.json.

    python tools/merge_leg.py [--scans 500] [--repeat 20]

Two sessions of the lap queue (two circuits of the synth world, saved with kh_mapper_save and loaded again), merged in one process:

  (a) kernel time per beam of the merged trace (k_occ_trace_merged) with identity corrections, HIP events (kh_occupancy_info)
  (b) kernel time per beam of k_occ_trace_resident over the same scans: kh_mapper_build_map of the two mappers, same source
  (c) wall time of a re-merge after set_transform (table upload, grid allocation, trace, Update, synchronise)
  (d) wall time of the host route: kh_mapper_get_scan of every scan, the correction in numpy, kh_occupancy_add_scans (40 bytes per
      beam over PCIe), Update

(a) and (b) alternate inside one loop after a warm-up; medians over --repeat rounds.  No threshold is applied to (c) and (d)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, synth  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402
from slam_toolbox_amd.merge import MapMerger  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402

RES = 0.05


def session(n_scans, aisles, seed, tmp):
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_scans, seed=seed, aisles=aisles)
    rng = np.random.default_rng(seed + 3)
    m = Mapper(synth.Laser(), loop_search_maximum_distance=3.0)
    for i in range(n_scans):
        m.Process(synth.make_scan(world, truth[i], rng), odom[i], 0.1 * i)
    path = os.path.join(tmp, f"laps_{aisles[0]}_{aisles[1]}.khms")
    m.save(path)
    m.close()
    return Mapper.load(path)


class HostScan:
    """what kh_occupancy_add_scans reads of a scan, held in numpy arrays"""

    def __init__(self, ranges, points, sensor_pose):
        self.ranges, self.points, self.sensor_pose = ranges, np.ascontiguousarray(points), sensor_pose

    def c(self):
        s = capi.KhScan()
        s.n = self.ranges.shape[0]
        s.ranges = self.ranges.ctypes.data_as(C.POINTER(C.c_double))
        s.points_xy = self.points.ctypes.data_as(C.POINTER(C.c_double))
        for k in range(3):
            s.sensor_pose[k] = self.sensor_pose[k]
        s.device_points_xy = None
        return s


def host_route(mappers, transforms):
    """the route that exists without the merger; returns the grid"""
    laser = synth.Laser()
    scans = []
    for m, (tx, ty, yaw) in zip(mappers, transforms):
        c, s = math.cos(yaw), math.sin(yaw)
        for i in m.alive():
            k, _ = m.scan(int(i))
            n = k.n
            ranges = np.ctypeslib.as_array(k.ranges, (n,))
            p = np.ctypeslib.as_array(k.points_xy, (2 * n,)).reshape(n, 2)
            with np.errstate(invalid="ignore"):
                q = np.stack([(c * p[:, 0] - s * p[:, 1]) + tx, (s * p[:, 0] + c * p[:, 1]) + ty], axis=1)
            sx, sy = k.sensor_pose[0], k.sensor_pose[1]
            scans.append(HostScan(ranges, q, ((c * sx - s * sy) + tx, (s * sx + c * sy) + ty, k.sensor_pose[2] + yaw)))
    arr = (capi.KhScan * len(scans))(*[s.c() for s in scans])
    w, h, off = C.c_int32(), C.c_int32(), np.zeros(2)
    capi.check(capi.lib().kh_occupancy_compute_dimensions(len(scans), arr, laser.min_range, laser.range_threshold, RES, C.byref(w), C.byref(h), off),
               "kh_occupancy_compute_dimensions")
    g = OccupancyGrid(w.value, h.value, off, RES)
    capi.check(capi.lib().kh_occupancy_add_scans(g._h, len(scans), arr, laser.range_threshold, laser.min_range, laser.max_range), "kh_occupancy_add_scans")
    g.Update(2, 0.1)
    return g


def spread(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=500)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_leg.json"))
    args = ap.parse_args()
    if capi.lib().kh_device_count() < 1:
        raise RuntimeError("merge_leg needs a GPU: nothing here is measured without one")
    with tempfile.TemporaryDirectory(prefix="merge_leg_") as tmp:
        mappers = [session(args.scans, (0, 1), 12345, tmp), session(args.scans, (1, 2), 777, tmp)]
    mg = MapMerger(RES)
    ids = [mg.add_submap(m) for m in mappers]
    placed = (3.0, -2.0, 0.7)
    merged_ns, resident_ns, remerge_ms, host_ms = [], [], [], []
    for rep in range(-3, args.repeat):                     # three warm-up rounds: code objects, first uploads, allocator
        mg.set_transform(ids[1], (0.0, 0.0, 0.0))
        g = mg.merge()
        a = 1e6 * g.stats()["trace_ms"] / g.stats()["beams"]
        g.close()
        ms, beams = 0.0, 0
        for m in mappers:
            g = m.build_map(RES)
            ms += g.stats()["trace_ms"]; beams += g.stats()["beams"]
            g.close()
        b = 1e6 * ms / beams
        t0 = time.perf_counter()
        mg.set_transform(ids[1], placed)
        g = mg.merge()
        c = (time.perf_counter() - t0) * 1e3
        st = mg.stats()
        assert st["point_uploads"] == 0 and st["range_uploads"] == 0
        g.close()
        t0 = time.perf_counter()
        g = host_route(mappers, [(0.0, 0.0, 0.0), placed])
        d = (time.perf_counter() - t0) * 1e3
        g.close()
        if rep >= 0:
            merged_ns.append(a); resident_ns.append(b); remerge_ms.append(c); host_ms.append(d)
    st = mg.stats()
    record = {"queue_scans_per_session": args.scans, "scans": st["scans_traced"], "beams": st["beams_traced"], "table_bytes": st["table_bytes"],
              "a_merged_trace_ns_per_beam": spread(merged_ns), "b_resident_trace_ns_per_beam": spread(resident_ns),
              "a_over_b": float(np.median(merged_ns) / np.median(resident_ns)),
              "c_remerge_wall_ms": spread(remerge_ms), "d_host_route_wall_ms": spread(host_ms),
              "d_over_c": float(np.median(host_ms) / np.median(remerge_ms))}
    mg.close()
    for m in mappers:
        m.close()
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
