"""TEST INFRASTRUCTURE: matcher geometries off the four (resolution, smear) pairs of the presets -- every smear-kernel size at which
kh_matcher_create takes another decision, and grid pitches down to one raster tile.

A table of named geometries (GEOMETRIES), the formulas of kh_matcher_create restated (derive()), a closed room of range readings
sized to each grid (scene()), the routes a geometry is walked on (RASTER, SCORING, the batch) with the restated rule of which way a
call must go (route()), and the address arithmetic of the scoring kernels restated over the CPU oracle's lookup table and lattice
(score_reads()).  tests/test_geometry_cases_oracle.py proves on the CPU that every geometry sits where its name says and pins the
oracle to the reference there; tests/test_geometry_gpu.py walks the table on the device.  Nothing here calls the library.

What is decided once, at create, and which geometry pins it (DESIGN.md section 3b has the same list):

* kernel_size = 2 * round_half_away(2 * smear / res) + 1.  k_raster_tile (LDS atomics, 64 / k^2 points per wave pass) stamps 3, 5
  and 7; k_raster_tile_reg and kseq_tile (tile in registers) 9 .. 41; kseq_stage is a launch of its own only below 8.
* n_foot, the off-centre kernel cells equal to 100: 4 at smear / res = 10 and 0 otherwise; it switches on the order-dependent rule
  (k_cell_first, k_cell_links, k_active_set, the first-point state of kseq_bin).
* bshift = 3 iff kernel_size <= 25 and side <= 64 and max_batch >= 8, else 5.
* ws, height and side give pad_rows, grid_pad, the copies' pitches, the raster tiles and the block map.

Reads of the narrow grids (ws <= 144), from the kernels' address arithmetic -- score_reads() computes the intervals per case and the
oracle-side test asserts them inside [-grid_pad, data_size + grid_pad):

* k_offsets / k_score, kseq_score (entries on the fast lists): a window that starts at byte `start` = base0 + idx of the grid is read
  from the dword boundary in front of it, rows (ny - 1) * sy_ws apart.  k_score's lanes stop behind the tile's last pose
  (lane_on): the last byte is start + (nx - 1) * sx + (ny - 1) * sy_ws + 3.  kseq_score has no such mask: every lane loads, the
  last byte is start - s + 63 + (ny - 1) * sy_ws -- up to 63 bytes behind the window on a lattice of four poses.  An entry is fast
  when start >= -pad and start + span < data_size + pad, pad = max(0, pad_rows * ws - 512), and grid_pad = align_up(pad_rows * ws,
  256) + 512 >= pad + 512: 3 bytes in front and 63 behind stay inside whatever ws is.  What a narrow pitch changes is WHICH rows the
  bytes behind the window belong to (the next rows: zeros or stamps), and those lanes' sums are dropped (x < PX, xi < nx).
* slow entries (k_score, kseq_score) and kseq_fine test every index against [0, data_size) before the load.
* K2' / K3' (lds_score): lds_cases.region_bounds over lds_cases.chunks, as tests/test_lds_cases_oracle.py has it.
* tile write-back (k_raster_tile, k_raster_tile_reg, kseq_tile) and the tile-list clear (k_raster_clear, prep_clear) clip on
  x < ws and y < height; ws is a multiple of 8, a tile starts on a multiple of 64 and the widest store is 8 bytes on a multiple of 8:
  no store crosses ws.  clear_tail() names the geometries whose last 16-byte group does cross it (the branch of k_raster_clear).
* the re-pitched and column-decimated copies are allocated by a search of nx * ny * na * P >= 1e8 only (ensure_slot_scratch): the
  largest search of this table is 33 x 33 x 21 x 181 = 4.1e6.  No geometry here has copies, CorrelateScan at two cells included
  (copies() restates the rule; the cases assert the result only).
"""
from __future__ import annotations

import math

import numpy as np

import lds_cases as lc
from common import OFFLINE_PARAMS, PRESETS
from seq_cases import ScanSpec, round_half_away
from slam_toolbox_amd import synth

TILE = 64                  # kRasterTile
BLOCK_SHIFT = 5            # kBlockShift
GRID_PAD = 512             # kGridPad
MAX_READINGS = 2048        # kSeqMaxReadings
TILE_SPAN = 61             # kTileSpan

N_BEAMS = 181
FOV = math.radians(270.0)
FAR_EVERY = 9              # every ninth query reading lies at 3 x the range threshold (from reading 4), every ninth behind its wall (from 1)
PARAMS = dict(PRESETS["K"]["params"])          # response expansion off


def laser():
    """the one laser of the table's scans (the reference build takes the layout from a registered device, not per scan)"""
    return synth.Laser(n_beams=N_BEAMS, min_angle=-0.5 * FOV, max_angle=0.5 * FOV, ang_res=FOV / (N_BEAMS - 1), min_range=0.0,
                       max_range=1000.0, range_threshold=1000.0)


# ---------------------------------------------------------------- kh_matcher_create, restated
def kernel_values(smear, res):
    """CalculateKernel (Mapper.h:1213-1266): the k x k byte kernel"""
    hk = int(round_half_away(2.0 * smear / res))
    k = 2 * hk + 1
    out = np.zeros((k, k), dtype=np.uint8)
    for i in range(-hk, hk + 1):
        for j in range(-hk, hk + 1):
            z = math.exp(-0.5 * math.pow(math.hypot(i * res, j * res) / smear, 2))
            out[j + hk, i + hk] = int(round_half_away(z * 100))
    return out


def accepted(res, smear):
    """the smear test of CalculateKernel on the grid's own resolution (1 / scale)"""
    r = 1.0 / (1.0 / res)
    return 0.5 * r <= smear <= 10 * r


def derive(create):
    """what kh_matcher_create derives from (search_size, resolution, smear, range_threshold)"""
    search, res, smear, rt = create
    side = int(round_half_away(search / res) + 1)
    margin = int(math.ceil(rt / res))
    roi = side + 2 * margin
    hk = int(round_half_away(2.0 * smear / res))
    width = roi + 2 * (hk + 1)
    ws = (width + 7) & ~7
    height = width
    kern = kernel_values(smear, 1.0 / (1.0 / res))
    k = 2 * hk + 1
    pad_rows = side + 8
    out = dict(kernel_size=k, n_foot=int((kern == 100).sum()) - 1, ws=ws, width=width, height=height, side=side, roi=roi, border=hk + 1,
               tiles=((ws + TILE - 1) // TILE) * ((height + TILE - 1) // TILE), data_size=ws * height, pad_rows=pad_rows,
               grid_pad=((pad_rows * ws + 255) // 256) * 256 + GRID_PAD, pad=max(0, pad_rows * ws - 512))
    for mb in (1, 8):
        out[f"bshift{mb}"] = 3 if (k <= 25 and side <= 64 and mb >= 8) else BLOCK_SHIFT
    return out


def clear_tail(d):
    """k_raster_clear: does the last 16-byte group of a tile row cross ws (the branch that stores 8 bytes at a time)"""
    return d["ws"] % 16 != 0


PROBE_KEYS = ("kernel_size", "n_foot", "ws", "height", "side", "tiles", "bshift1", "bshift8")


class Geometry:
    def __init__(self, name, create, stands_for, probe, offline=False, two_cells=False, last=False):
        self.name, self.create, self.stands_for, self.offline, self.two_cells, self.last = name, tuple(create), stands_for, offline, two_cells, last
        self.probe = dict(zip(PROBE_KEYS, probe))

    def params_sets(self):
        return (("K", PARAMS),) + ((("offline", dict(OFFLINE_PARAMS)),) if self.offline else ())

    def oracle_matcher(self, params=None):
        from oracle import karto
        return karto.Matcher(*self.create, PARAMS if params is None else params)

    def hip_matcher(self, params=None, max_batch=1):
        from slam_toolbox_amd.scan_matcher import MapperParams, ScanMatcher
        return ScanMatcher.Create(MapperParams(**(PARAMS if params is None else params)), *self.create, max_batch=max_batch)

    def __repr__(self):
        return self.name


P2 = 2.0 ** -5
#                       create (search, res, smear, range)      stands for                                      k  foot  ws  height side tiles b1 b8
GEOMETRIES = [
    Geometry("k5",           (0.3, 0.01, 0.011, 1.0), "k_raster_tile, two points per wave pass",                (5, 0, 240, 237, 31, 16, 5, 3)),
    Geometry("k7",           (0.3, 0.01, 0.016, 1.0), "k_raster_tile, one point per pass, lanes 49-63 idle",    (7, 0, 240, 239, 31, 16, 5, 3), offline=True),
    Geometry("k7 half away", (P2 * 10, P2, 1.25 * P2, 1.5), "2 smear / res == 2.5: half away from zero",        (7, 0, 120, 115, 11, 4, 5, 3)),
    Geometry("k9",           (0.3, 0.01, 0.021, 1.0), "first size on k_raster_tile_reg / kseq_tile; ws 3*64+56", (9, 0, 248, 241, 31, 16, 5, 3), two_cells=True),
    Geometry("k9 coarse",    (0.5, 0.05, 0.11, 3.0),  "k = 9 on a coarse grid, side 11 (a nav-style config)",   (9, 0, 144, 141, 11, 9, 5, 3)),
    Geometry("k7 side 21",   (0.4, 0.02, 0.031, 1.5), "k = 7, side 21, ws 184",                                 (7, 0, 184, 179, 21, 9, 5, 3)),
    Geometry("k21 narrow",   (0.3, 0.01, 0.051, 0.3), "under two raster tiles wide; search 31 of 91 ROI cells", (21, 0, 120, 113, 31, 4, 5, 3), two_cells=True),
    Geometry("k25",          (0.3, 0.01, 0.061, 1.0), "last kernel size with bshift 3",                         (25, 0, 264, 257, 31, 25, 5, 3)),
    Geometry("k27",          (0.3, 0.01, 0.066, 1.0), "first kernel size with bshift 5 on a batch handle",      (27, 0, 264, 259, 31, 25, 5, 5)),
    Geometry("side 64",      (0.63, 0.01, 0.03, 1.0), "last side with bshift 3",                                (13, 0, 280, 278, 64, 25, 5, 3)),
    Geometry("side 65",      (0.64, 0.01, 0.03, 1.0), "first side with bshift 5 on a batch handle",             (13, 0, 280, 279, 65, 25, 5, 5)),
    Geometry("k41 no foot",  (0.3, 0.01, 0.099, 1.0), "41 x 41 kernel, no 100 off-centre",                      (41, 0, 280, 273, 31, 25, 5, 5)),
    Geometry("k41 foot",     (0.3, 0.01, 0.1, 1.0),   "41 x 41 kernel with the order-dependent rule, same grid", (41, 4, 280, 273, 31, 25, 5, 5), offline=True),
    Geometry("k41 small",    (0.3, 0.01, 0.1, 0.1),   "footprints over a third of the grid, 2 x 2 raster tiles", (41, 4, 96, 93, 31, 4, 5, 5)),
    Geometry("pad 7",        (0.3, 0.01, 0.03, 0.46), "ws 144 against width 137: seven padding columns",        (13, 0, 144, 137, 31, 9, 5, 3)),
    Geometry("one tile",     (0.06, 0.01, 0.006, 0.2), "ONE raster tile; a grid row shorter than a 64-byte window row", (3, 0, 56, 51, 7, 1, 5, 3), last=True),
]
BY_NAME = {g.name: g for g in GEOMETRIES}
NARROW = 144               # ws up to here: the in-bounds argument of the module docstring is asserted per case
PAIRS = (("k25", "k27"), ("side 64", "side 65"), ("k41 no foot", "k41 foot"))

RASTER = ("table", "hash")
SCORING = ("fused", "general", "lds", "windowed", "dense")
FLAGS = ((True, True), (False, False))


def debug_bits(scoring):
    """kh_matcher_set_debug arguments of a scoring route"""
    return dict(fused={}, general=dict(no_fused_match=True), lds=dict(lds_score=True, no_fused_match=True),
                windowed=dict(windowed_score=True, no_fused_match=True), dense=dict(dense_score=True, no_fused_match=True))[scoring]


def route(scoring, raster, n_calls):
    """what seq_stats() must read after n_calls MatchScan calls: the fused path takes every call of a `table` input (181 readings, 4
    scans, 724 points, <= 25 tiles: inside every limit of plan_table_raster) and refuses the `hash` input with reason 3 (a base scan
    of more than kSeqMaxReadings readings); a handle with no_fused_match never asks"""
    st = dict(calls=0, fused_score=0, ineligible=0, ineligible_reason=0)
    if scoring == "fused":
        if raster == "table":
            st.update(calls=n_calls, fused_score=n_calls)
        else:
            st.update(ineligible=n_calls, ineligible_reason=3)
    return st


# ---------------------------------------------------------------- the scene: a closed room sized to the grid
def room(rt, shift=(0.0, 0.0)):
    """walls about 0.6 x the range threshold from the origin (not square: no pose ties with another), one pillar"""
    sx, sy = shift
    segs = synth._rect(sx - 0.6 * rt, sy - 0.52 * rt, sx + 0.56 * rt, sy + 0.6 * rt)
    segs += synth._rect(sx + 0.2 * rt, sy + 0.25 * rt, sx + 0.3 * rt, sy + 0.33 * rt)
    return np.asarray(segs, dtype=np.float64)


class Scene:
    """base scans a few cells apart, a query two or three cells and 0.02 rad off its true pose, with far and fringe readings"""

    def __init__(self, geo, shift_cells=0):
        _, res, _, rt = geo.create
        self.res, self.rt = res, rt
        shift = (shift_cells * res, -shift_cells * res)
        world = room(rt, shift)
        rng = np.random.default_rng(1000 + shift_cells)
        lz = laser()

        def scan(pose, at=None):
            r = synth.raycast(world, pose, lz) + rng.normal(0.0, 0.2 * res, size=N_BEAMS)
            return ScanSpec(r, pose if at is None else at, lz.min_angle, lz.ang_res)
        self.base = [scan((shift[0] + 3 * i * res, shift[1] - 2 * i * res, 0.4 * i - 0.5)) for i in range(4)]
        truth = (1.5 * res, -0.5 * res, 0.1)
        self.guess = (truth[0] + 2.5 * res, truth[1] - 2.0 * res, truth[2] + 0.02)
        q = scan((shift[0] + truth[0], shift[1] + truth[1], truth[2]), at=self.guess)
        r = q.ranges.copy()
        r[4::FAR_EVERY] = 3.0 * rt + 0.37 * res * np.arange(r[4::FAR_EVERY].size)
        # ... and every ninth lands behind its wall by the half kernel and 8 to 15 cells more: its window touches the outermost cells
        # of the walls' footprints only -- where a block-map bit that a stamp failed to set makes the window count as empty
        hk = derive(geo.create)["kernel_size"] // 2
        r[1::FAR_EVERY] += (hk + 8 + np.arange(r[1::FAR_EVERY].size) % 8) * res
        self.query = ScanSpec(r, self.guess, q.min_angle, q.ang_res)
        # the hash route: one more base scan, of 2049 readings that are NaN from reading 400 on (plan_table_raster: reason 3)
        long = np.full(MAX_READINGS + 1, np.nan)
        first = synth.raycast(world, (shift[0] - res, shift[1] + 2 * res, 0.9), synth.Laser(n_beams=400, min_angle=lz.min_angle, ang_res=FOV / 399))
        long[:400] = 0.8 * first + rng.normal(0.0, 0.2 * res, size=400)         # (a smaller room: stamps where the other scans leave none)
        self.long = ScanSpec(long, (shift[0] - res, shift[1] + 2 * res, 0.9), lz.min_angle, FOV / 399)

    def bases(self, raster):
        return self.base + ([self.long] if raster == "hash" else [])

    def query_at(self, i):
        """the query at the i-th of eight poses one cell apart"""
        pose = (self.guess[0] + (i - 3) * self.res, self.guess[1] + ((i % 3) - 1) * self.res, self.guess[2] + 0.003 * i)
        return ScanSpec(self.query.ranges, pose, self.query.min_angle, self.query.ang_res)


SHIFT_CELLS = 20           # the second scene of a slot: the room 20 cells further


# ---------------------------------------------------------------- the searches, as lds_cases sees them
class Search:
    """the arguments of one CorrelateScan in the shape lds_cases.classify() reads them"""

    def __init__(self, query, centre, ang_off, ang_res):
        self.query, self.centre, self.ang_off, self.ang_res = query, np.asarray(centre, dtype=np.float64), ang_off, ang_res


def coarse_args(geo, params):
    """MatchScan's coarse search (Mapper.cpp:577-592): offsets, resolutions"""
    d = derive(geo.create)
    res = 1.0 / (1.0 / geo.create[1])
    off = 0.5 * (float(d["side"]) - 1) * res
    return (off, off), (2 * res, 2 * res), params["coarse_search_angle_offset"], params["coarse_angle_resolution"]


def run_coarse(om, geo, scene, raster="table", params=PARAMS, penalize=True):
    """AddScans + the coarse CorrelateScan on the oracle; returns (result, Search)"""
    q = scene.query.oracle()
    om.add_scans(q, [b.oracle() for b in scene.bases(raster)])
    off, res, ang_off, ang_res = coarse_args(geo, params)
    out = om.correlate_scan(q, q.sensor_pose, off, res, ang_off, ang_res, penalize, False)
    return out, Search(scene.query, scene.query.pose, ang_off, ang_res)


def score_reads(cl, d, lanes_masked):
    """(lowest, highest) byte offset from the grid's first byte that the windowed scoring of the search reads for its FAST entries:
    k_score (lanes_masked: lanes behind the tile's last pose do not load) or kseq_score (every lane loads its dword of the 64-byte
    tile row).  One scoring tile: nx <= 31 two-cell poses."""
    lat = cl["lat"]
    assert lat["linear"] and (lat["nx"] - 1) * lat["sx"] + 1 <= TILE_SPAN
    start = lat["base0"] + cl["gx"] + cl["gy"] * lat["ws"]
    fast = cl["cls"] == lc.FAST
    if not fast.any():
        return 0, 0
    start = start[fast]
    s = start & 3
    rows = (lat["ny"] - 1) * lat["sy_ws"]
    lo = int((start - s).min())
    if lanes_masked:
        last_lane = (s + (lat["nx"] - 1) * lat["sx"]) // 4           # lane_on: 4 * lx <= s + (np_tile - 1) * SX
        hi = int((start - s + 4 * last_lane + 3 + rows).max())
    else:
        hi = int((start - s + 63 + rows).max())
    return lo, hi


def copies(lat, n_beams):
    """ensure_slot_scratch's rule for allocating re-pitched / column-decimated copies (lds_cases.copies_kind): 0 = none"""
    return lc.copies_kind(lat, n_beams)
