"""Generates tests/golden/occupancy_edges.npz from the reference build (oracle/_ref/libkarto_ref.so): the reference's own
karto::OccupancyGrid::CreateFromScans (Karto.h:5947-5962) on 12 scans whose range readings sit ON the gates of AddScan
(Karto.h:6167-6180): min_range and one ulp either side, range_threshold and one ulp below, range_threshold - 1e-6 and one ulp
either side, a reading between threshold and max_range, max_range and one ulp either side, NaN, +inf, -inf, 0 and a negative
reading (tests/occupancy_cases.py::gate_values), each at several beams of every scan.  The other readings follow a smooth wall
quantised to 1/64 m, which keeps the file small.  Same sparse layout as occupancy.npz.
Run in the dev container: python tests/golden/make_golden_occupancy_edges.py"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import occupancy_cases as oc  # noqa: E402
from oracle import ref  # noqa: E402
from slam_toolbox_amd import synth  # noqa: E402

N_SCANS, RESOLUTION = 12, 0.2


def gate_scans(laser):
    gates = oc.Gates(laser.min_range, laser.range_threshold, laser.max_range)
    values = [v[1] for v in oc.gate_values(gates)]
    beam = np.arange(laser.n_beams)
    ranges = np.zeros((N_SCANS, laser.n_beams))
    poses = np.zeros((N_SCANS, 3))
    for k in range(N_SCANS):
        ranges[k] = np.round((4.0 + 1.5 * np.sin(beam * 0.01 + k)) * 64.0) / 64.0
        for j, v in enumerate(values):
            for rep in range(3):
                ranges[k, (7 * k + 59 * j + 353 * rep) % laser.n_beams] = v
        poses[k] = (0.25 * k, -0.125 * k, 0.25 * k - 1.0)
    return ranges, poses


def main():
    laser = synth.Laser()
    ref.init_laser(laser)
    L = ref.lib()
    ranges, poses = gate_scans(laser)
    scans = [ref.RefScan(ranges[k], poses[k]) for k in range(N_SCANS)]
    handles = (C.c_void_p * len(scans))(*[s.h for s in scans])
    dims = (C.c_int * 3)()
    off = (C.c_double * 2)()
    L.ref_occupancy_from_scans.restype = C.c_int
    L.ref_occupancy_from_scans.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    size = L.ref_occupancy_from_scans(handles, len(scans), RESOLUTION, dims, off, None, None, None, 0)
    cells = np.zeros(size, dtype=np.uint8)
    passes = np.zeros(size, dtype=np.uint32)
    hits = np.zeros(size, dtype=np.uint32)
    L.ref_occupancy_from_scans(handles, len(scans), RESOLUTION, dims, off, cells.ctypes.data, passes.ctypes.data, hits.ctypes.data, size)
    nz = np.flatnonzero(passes)
    out = os.path.join(ROOT, "tests", "golden", "occupancy_edges.npz")
    np.savez_compressed(out, ranges=ranges, poses=poses, resolution=RESOLUTION, dims=np.asarray(list(dims), dtype=np.int32),
                        offset=np.asarray(list(off)), cells_idx=np.flatnonzero(cells).astype(np.int32),
                        cells_val=cells[np.flatnonzero(cells)], count_idx=nz.astype(np.int32), pass_val=passes[nz], hit_val=hits[nz])
    print(out, os.path.getsize(out), "bytes; grid", list(dims), "offset", list(off), "touched cells", nz.size, "occupied",
          int((cells == 100).sum()), "free", int((cells == 255).sum()))


if __name__ == "__main__":
    main()
