"""Maps whose clip to the region of interest holds more units than one trip of k_map_collect (csrc/matcher_kernels.hip), as plain numpy
data.  tests/test_map_match_rule_oracle.py checks with tests/map_match_rule.py alone that every case holds the units its name says;
tests/test_map_match_gpu.py hands the same cases to the library and compares the grid bytes.

The capped launches.  k_map_collect runs on min(ceil(n_units / 4), 1024) workgroups of four waves per job, a wave a unit of 64 cells of
a row of the clip: TRIP_UNITS = 4096 units per trip of its strided loop, the launch sized by the largest job of the batch.
k_map_collect_scan is one workgroup of SCAN_THREADS = 1024 threads per job, per = ceil(n_units / 1024) units a thread.  The maps of
tests/test_map_match_gpu.py before this table hold 576 units at the most (192 x 192 cells).  n_units is that of the clip (clip_axis,
csrc/matcher_host.cpp), which the library does not report: map_match_rule.units_lower_bound and units_upper_bound hold it from both
sides, and for a map that lies inside the region of interest the two are equal.

Launches of the matcher's hot path that are capped too and whose later trips the suite reached before (checked on the CPU in
tests/test_map_match_rule_oracle.py from the grids' sizes, without running anything): k_raster_tile and k_repitch* on at most 2048
tiles of 32 x 32 cells, k_repitch_full on at most 4096 rows -- the benchmark-shape cases of tests/test_baseline_shapes_gpu.py run the
sequential preset's grid of 4096 tiles and the loop preset's re-pitched copy of more than 8000 rows."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

SMALL = (0.3, 0.01, 0.03, 4.0)              # 13 x 13 smear kernel with 100 on its centre alone, region of interest 831 cells
FOOT = (0.3, 0.01, 0.0999, 4.0)             # the kernel holds 100 on the centre's four neighbours: the stamping order shows in the bytes
WIDE = (0.3, 0.01, 0.03, 12.0)              # region of interest 2431 cells: 4862 rows of a 0.005 m map
TRIP_UNITS, SCAN_THREADS = 4096, 1024
TO_CELL = {-1: 0, 100: 100, 0: 255}
MapCase = namedtuple("MapCase", "name create pose nav offset res above")
BatchCase = namedtuple("BatchCase", "name create nav offset res poses units")


def cells_of(nav):
    out = np.zeros(nav.shape, dtype=np.uint8)
    for k, v in TO_CELL.items():
        out[nav == k] = v
    return out


def framed_nav(rng, h, w, p_occ=0.12):
    """random nav values, p_occ of them occupied, inside a frame of occupied cells: the first and last column and row"""
    nav = rng.choice(np.array([-1, 100, 0], dtype=np.int8), size=(h, w), p=[(1 - p_occ) / 2, p_occ, (1 - p_occ) / 2])
    nav[:, 0] = nav[:, w - 1] = 100
    nav[0, :] = nav[h - 1, :] = 100
    return nav


def centred(pose, h, w, res):
    """the offset that puts the map's middle on the pose, off the grid's lattice by a few millimetres"""
    return (pose[0] - 0.5 * w * res + 0.0037, pose[1] - 0.5 * h * res - 0.0041)


def trip_cases():
    """800 columns are 13 units a row: 80, 160, 320 and 640 rows are 1040, 2080, 4160 and 8320 units"""
    out = []
    rng = np.random.default_rng(41)
    pose = np.array([1.0, 2.0, 0.1])
    for res in (0.01, 0.005):
        for h, above in ((80, 1024), (160, 2048), (320, 4096), (640, 8192)):
            out.append(MapCase(f"800 x {h} at {res} m: above {above} units", SMALL, pose, framed_nav(rng, h, 800), centred(pose, h, 800, res), res, above))
    for h, above in ((320, 4096), (640, 8192)):
        out.append(MapCase(f"800 x {h} at 0.01 m, a kernel with 100 off-centre: above {above} units", FOOT, pose, framed_nav(rng, h, 800),
                           centred(pose, h, 800, 0.01), 0.01, above))
    out.append(MapCase("40 x 4400 at 0.005 m, one unit a row: above 4096 units", WIDE, pose, framed_nav(rng, 4400, 40), centred(pose, 4400, 40, 0.005),
                       0.005, 4096))
    return out


def batch_case():
    """one map of 800 x 640 cells at 0.01 m and three poses: the region of interest around the map, over the map's first cell alone (the
    region's last cell lies a third of a cell beyond that cell's centre), and 300 m away"""
    rng = np.random.default_rng(43)
    res, h, w = 0.01, 640, 800
    pose = np.array([1.0, 2.0, 0.1])
    offset = centred(pose, h, w, res)
    reach = 0.5 * (831 - 1) * res                                # the region of interest's last cell centre, from the pose
    corner = np.array([offset[0] - reach + 0.3 * res, offset[1] - reach + 0.3 * res, -0.2])
    far = np.array([pose[0] + 300.0, pose[1] + 100.0, 0.5])
    return BatchCase("one map, clips of 8320, 3 and 0 units", SMALL, framed_nav(rng, h, w), offset, res, [pose, corner, far], [8320, 3, 0])
