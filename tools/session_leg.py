"""Measures mapping sessions and writes profiles/session_leg.json:

  * kh_mapper_build_map (trace from the resident scans) against the existing host-packed path (kh_occupancy_compute_dimensions +
    _create + _add_scans + _update over kh_mapper_get_scan) on the SAME session in the same process: first build and rebuild
    after 10 new scans, wall and kernel time (HIP events of the grid), medians of --repeats alternating runs.  The packed path is
    timed from a kh_scan array made beforehand: fetching the scans through ctypes is not charged to it.
  * kh_mapper_save / kh_mapper_load wall time and file size, load split into read + validate, Update of every scan, solver rebuild,
    graph store (kh_session_last_load_ms).
  * per accepted scan, localization behind a LOADED map against the same map built in-process (the legs of tools/localization_leg.py).

    python tools/session_leg.py [--sizes 500 3000] [--repeats 7]
(queue sizes: half of each queue is the map, so 500 / 3000 give the 250- / 1500-scan sessions)"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, session, synth  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402
from slam_toolbox_amd.occupancy_grid import OccupancyGrid  # noqa: E402

RESOLUTION = 0.05


def queue(n_scans):
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_scans)
    rng = np.random.default_rng(4)
    ranges = np.ascontiguousarray(np.stack([synth.make_scan(world, truth[i], rng) for i in range(n_scans)]))
    return ranges, np.ascontiguousarray(odom)


def med(v):
    return float(np.median(np.asarray(v)))


def packed_map(m, scans=None):
    """the existing path; returns (wall ms of the four C calls, kernel ms)"""
    L, laser = capi.lib(), synth.Laser()
    ids = m.alive()
    if scans is None:
        scans = (capi.KhScan * len(ids))(*[m.scan(int(i))[0] for i in ids])
    t0 = time.perf_counter()
    w, h, off = C.c_int32(), C.c_int32(), np.zeros(2)
    capi.check(L.kh_occupancy_compute_dimensions(len(ids), scans, laser.min_range, laser.range_threshold, RESOLUTION, C.byref(w), C.byref(h), off),
               "kh_occupancy_compute_dimensions")
    g = OccupancyGrid(w.value, h.value, off, RESOLUTION)
    capi.check(L.kh_occupancy_add_scans(g._h, len(ids), scans, laser.range_threshold, laser.min_range, laser.max_range), "kh_occupancy_add_scans")
    g.Update(2, 0.1)
    wall = (time.perf_counter() - t0) * 1e3
    kernel = g.stats()["trace_ms"]
    g.close()
    return wall, kernel


def resident_map(m):
    t0 = time.perf_counter()
    g = m.build_map(RESOLUTION)
    wall = (time.perf_counter() - t0) * 1e3
    kernel = g.stats()["trace_ms"]
    g.close()
    return wall, kernel


def leg(n_queue, repeats, tmp):
    ranges, odom = queue(n_queue)
    switch = n_queue // 2
    out = {"queue_scans": n_queue, "map_queue_scans": switch}
    path = os.path.join(tmp, f"session_{n_queue}.khms")
    m = Mapper(synth.Laser(), loop_search_maximum_distance=3.0)
    for i in range(switch):
        m.Process(ranges[i], odom[i], 0.1 * i)
    out["scans_alive"] = int(len(m.alive()))
    save_ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        m.save(path)
        save_ms.append((time.perf_counter() - t0) * 1e3)
    out["save_ms"], out["file_bytes"] = med(save_ms), os.path.getsize(path)
    m.close()
    # load, and the FIRST build of each path on a freshly loaded mapper (nothing resident yet), alternating
    load_ms, split, first_res, first_packed = [], [], [], []
    for r in range(repeats):
        t0 = time.perf_counter()
        m = Mapper.load(path)
        load_ms.append((time.perf_counter() - t0) * 1e3)
        parts = np.zeros(4)
        capi.lib().kh_session_last_load_ms(parts)
        split.append(parts)
        if r % 2 == 0:
            first_res.append(resident_map(m)); first_packed.append(packed_map(m))
        else:
            first_packed.append(packed_map(m)); first_res.append(resident_map(m))
        if r + 1 < repeats:
            m.close()
    split = np.median(np.stack(split), axis=0)
    out["load_ms"] = med(load_ms)
    out["load_split_ms"] = dict(zip(("read_validate", "create_and_update_scans", "solver_rebuild", "graph_store"), (float(v) for v in split)))
    out["first_build"] = {"resident_wall_ms": med([a for a, _ in first_res]), "resident_kernel_ms": med([b for _, b in first_res]),
                          "packed_wall_ms": med([a for a, _ in first_packed]), "packed_kernel_ms": med([b for _, b in first_packed])}
    # rebuild after 10 new scans, repeated: 10 more accepted scans, then both paths
    re_res, re_packed, i = [], [], switch
    for r in range(repeats):
        more = 0
        while more < 10 and i < n_queue:
            more += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
            i += 1
        if more < 10:
            break
        if r % 2 == 0:
            re_res.append(resident_map(m) + (m.map_stats()["point_uploads"],)); re_packed.append(packed_map(m))
        else:
            re_packed.append(packed_map(m)); re_res.append(resident_map(m) + (m.map_stats()["point_uploads"],))
    out["rebuild_after_10_scans"] = {"repeats": len(re_res), "resident_wall_ms": med([a for a, _, _ in re_res]),
                                     "resident_kernel_ms": med([b for _, b, _ in re_res]), "point_uploads_median": med([c for _, _, c in re_res]),
                                     "packed_wall_ms": med([a for a, _ in re_packed]), "packed_kernel_ms": med([b for _, b in re_packed])}
    for k in ("first_build", "rebuild_after_10_scans"):
        out[k]["wall_ratio_packed_over_resident"] = out[k]["packed_wall_ms"] / out[k]["resident_wall_ms"]
    m.close()
    # localization behind the loaded map against the map built in-process
    loc = {}
    for mode in ("in_process", "loaded"):
        if mode == "loaded":
            m = Mapper.load(path)
        else:
            m = Mapper(synth.Laser(), loop_search_maximum_distance=3.0)
            for i in range(switch):
                m.Process(ranges[i], odom[i], 0.1 * i)
        ms = []
        for i in range(switch, n_queue):
            t0 = time.perf_counter()
            ok = m.ProcessLocalization(ranges[i], odom[i], 0.1 * i)[0]
            dt = (time.perf_counter() - t0) * 1e3
            if ok:
                ms.append(dt)
        loc[mode] = {"scans": len(ms), "median_ms": med(ms), "mean_ms": float(np.mean(ms))}
        m.close()
    loc["median_ratio_loaded_over_in_process"] = loc["loaded"]["median_ms"] / loc["in_process"]["median_ms"]
    out["localization_per_accepted_scan"] = loc
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 3000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_leg.json"))
    a = ap.parse_args()
    result = {"tool": "tools/session_leg.py", "resolution": RESOLUTION, "repeats": a.repeats, "legs": []}
    with tempfile.TemporaryDirectory() as tmp:
        for n in a.sizes:
            result["legs"].append(leg(n, a.repeats, tmp))
            print(json.dumps(result["legs"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
