"""TEST INFRASTRUCTURE: edge cases of the LDS-staged scoring kernels k_offsets_lds (K2') and k_score_lds (K3') of csrc/matcher_kernels.hip.

A table of named cases (cases()), the rules of the path restated over the CPU oracle's lookup table and grid geometry -- classify():
the class K2' gives every (angle, beam) entry; chunks(): its greedy chunk builder; predict(): whether prepare_job sends the search down
the path and what kh_matcher_score_loads must then report.  tests/test_lds_cases_oracle.py proves on the CPU that every case sits on
the edge its probe names; tests/test_lds_edges_gpu.py walks the table on the device.  Nothing here calls the library.

What the table found out about the path while it was written (DESIGN.md section 4 has the same list):

* DEFECT, fixed with the table: prepare_job reports a two-cell search on a slot that holds column-decimated copies as an sx = 1 job
  (true for the windowed kernel, which then reads the copies), and the LDS launch took its instance from that number: k_score_lds<1>
  on a lattice that steps two cells -- row step, poses per row and the epilogue's pose mapping all wrong (group G).  K2' / K3' read the
  grid itself: they now get the lattice's own step (JobShape::lds_sx).  One-cell jobs never have `dec`: their instance is unchanged.
* The class of a window is (base0 + gx) & 3 whatever the chunk: the region's first column is xmin rounded DOWN to 16 bytes of the
  grid address, so rel & 3 does not depend on which beams share the chunk.  The x test of `fits` is monotone along the lanes for the
  same reason (the aligned start only moves left), which is what the builder's "run of ones, then zeros" relies on.
* "Slow" through the pad is unreachable from MatchScan: the allocation has side + 8 zero rows either side and a window is at most
  `side` rows high, so a window that starts beyond the pad is wholly off the array.  It is reached by a public CorrelateScan whose
  lattice is taller than the handle's search space (a fine search: the coarse one must fit the probability grid), group E.
* A region's rows stay inside the allocation: see region_bounds().
* A chunk never spans two runs of 64 beams, so P = 256 with no two neighbours compatible fills lds_desc_capacity exactly (64 per
  builder wave) and nothing can exceed it.
* The fallback sends the LAST angle of the pair that still has a window to the slow list, so a far beam costs angle a0 + 1 a slow
  entry and angle a0 none; in the last group of an odd angle count the second angle is dead and a far beam needs no fallback.
* K3's step_base (the running step number over the classes and chunks of an angle) only BALANCES the steps between the waves that
  share an angle's rows: wave `part` takes the steps of a class whose number is (part - step_base) modulo `parts`, and for any
  step_base the `parts` waves together take every step of the class exactly once (deal() restates it).  Dropping step_base from
  the formula therefore changes no sum -- that mutant is equivalent, no case can catch it (the GPU file's docstring has the run).
  What a case CAN catch in this bookkeeping is a dealing that is no bijection (two waves on one step, or a step nobody takes):
  the tails cases make the step number enter every class and chunk at every phase, so such a slip shows in the sums.
* With every reading invalid no chunk exists, K3' walks nothing and every pose ties at 0: beyond kTieCap poses the host's walk of the
  volume takes over, like on the windowed path.
"""
from __future__ import annotations

import math

import numpy as np

from common import PRESETS
from seq_cases import ScanSpec, ring_scan, room_base, room_scan, round_half_away

# ---------------------------------------------------------------- the path's constants, restated
TILE_BYTES = 64           # kTileBytes (kh_internal.hpp): bytes of a grid row a window row reads
TILE_SPAN = 61            # kTileSpan (kh_internal.hpp): of which hold poses whatever the alignment class
CLASSES = 4               # kClasses (kh_internal.hpp)
GROUP_ANGLES = 2          # kGroupAngles = KH_GROUP_ANGLES (kh_internal.hpp)
LDS_PITCH = 192           # kLdsPitch = KH_LDS_PITCH (kh_internal.hpp)
LDS_ROWS = 196            # kLdsRows = KH_LDS_ROWS (kh_internal.hpp)
LDS_RANGES = 4            # kLdsRanges (kh_internal.hpp): builder waves of K2'
MAX_BEAMS = 2048          # prepare_job's lds_ok: c.P <= 2048 (k_offsets_lds: kMaxRounds = 8 rounds of 256)
MAX_ROWS = 64             # prepare_job's lds_ok: c.ny <= 64
GRID_PAD = 512            # kGridPad (kh_internal.hpp)
INVALID_SCAN = 2147483647  # kInvalidScan (kh_internal.hpp)
TIE_CAP = 2048            # kTieCap (kh_internal.hpp)


def lds_desc_capacity(n_points):
    """lds_desc_capacity (kh_internal.hpp): descriptors one builder wave may write"""
    return 64 * ((n_points + 255) // 256)


def lds_row_waves(ny):
    """lds_row_waves (kh_internal.hpp): how many of an angle's four waves share the lattice rows"""
    return 1 if ny <= 16 else 2 if ny <= 32 else 4


def pad_rows(side):
    """kh_matcher_create: m->pad_rows = m->side + 8"""
    return side + 8


INVALID, OFF, SLOW, FAST = 0, 1, 2, 3
KINDS = ("lattice", "angles", "beams", "invalid runs", "chunk per beam", "one chunk", "tails", "region x", "region y", "fallback",
         "array edges", "past the limit")


class Case:
    """one CorrelateScan: query, base scans, matcher geometry, search arguments; `dense`: the dense_score settings it runs with"""

    def __init__(self, name, kind, query, base, lattice, probe, na=1, ang_res=1e-6, create=None, fine=False, centre=None, dense=(True,),
                 pens=(True, False)):
        self.name, self.kind, self.query, self.base, self.probe = name, kind, query, base, dict(probe)
        self.create = tuple(G1 if create is None else create)
        self.params = dict(PRESETS["K"]["params"])
        nx, ny, s = lattice
        self.want = (nx, ny, s, na)
        cell = self.create[1]
        self.off = (0.5 * (nx - 1) * s * cell, 0.5 * (ny - 1) * s * cell)
        self.res = (s * cell, s * cell)
        self.ang_off, self.ang_res = 0.5 * (na - 1) * ang_res, ang_res
        # lattice poses a fifth of a cell off the cell centres, whatever the parity of the lattice: no pose on a rounding boundary
        shift = [0.002 + (0.5 * cell if (s == 1 and n % 2 == 0) else 0.0) for n in (nx, ny)]
        c = query.pose if centre is None else np.asarray(centre, dtype=np.float64)
        self.centre = np.array([c[0] + shift[0], c[1] + shift[1], c[2]])
        self.fine, self.dense, self.pens = fine, tuple(dense), tuple(pens)

    def geometry(self):
        return self.create

    def args(self):
        return self.centre, self.off, self.res, self.ang_off, self.ang_res

    def oracle_matcher(self):
        from oracle import karto
        return karto.Matcher(*self.create, self.params, threads=4)

    def hip_matcher(self, max_batch=1):
        from slam_toolbox_amd.scan_matcher import MapperParams, ScanMatcher
        return ScanMatcher.Create(MapperParams(**self.params), *self.create, max_batch=max_batch)

    def base_scans(self):
        return BASES[self.base]()


def run_oracle(om, case, pen):
    """the oracle's AddScans + CorrelateScan of the case: (response, mean, covariance)"""
    q = case.query.oracle()
    om.add_scans(q, [b.oracle() for b in case.base_scans()])
    centre, off, res, ang_off, ang_res = case.args()
    return om.correlate_scan(q, centre, off, res, ang_off, ang_res, pen, case.fine)


# ---------------------------------------------------------------- prepare_job and K2', restated over the oracle's last search
def lattice(om):
    """the lattice of the oracle's last CorrelateScan as prepare_job sees it: base indices, steps, `linear`"""
    g = om.grid_info()
    vol = om.volume()
    ny, nx, na = vol.shape[:3]
    ws = g["width_step"]
    bx = [round_half_away((vol[0, k, 0, 1] - g["offset_x"]) * g["scale"]) + g["roi_x"] for k in range(nx)]
    by = [(round_half_away((vol[k, 0, 0, 2] - g["offset_y"]) * g["scale"]) + g["roi_y"]) * ws for k in range(ny)]
    sx = bx[1] - bx[0] if nx > 1 else 1
    sy_ws = by[1] - by[0] if ny > 1 else ws
    linear = sx in (1, 2) and sy_ws > 0
    linear = linear and all(bx[k] - bx[k - 1] == sx for k in range(1, nx)) and all(by[k] - by[k - 1] == sy_ws for k in range(1, ny))
    if linear:
        bmax = bx[0] + by[0] + (ny - 1) * sy_ws
        linear = bx[0] + by[0] >= 0 and bmax < g["data_size"]
    if not linear:
        sx, sy_ws = 1, ws
    side = om.probs().shape[0]
    return dict(nx=nx, ny=ny, na=na, ws=ws, data_size=g["data_size"], base0=bx[0] + by[0], sx=sx, sy_ws=sy_ws, sy_cells=sy_ws // ws,
                linear=linear, pad=max(0, pad_rows(side) * ws - GRID_PAD), side=side, scale=g["scale"])


def lds_rule(lat, n_beams):
    """the conditions of prepare_job's lds_ok with the path forced (lds_always), by name"""
    sx = lat["sx"]
    return dict(linear=lat["linear"], nx=(lat["nx"] - 1) * sx + 1 <= TILE_SPAN, ny=lat["ny"] <= MAX_ROWS, P=n_beams <= MAX_BEAMS,
                rows=lat["sy_ws"] % lat["ws"] == 0 and lat["sy_ws"] // lat["ws"] == sx, pitch=lat["ws"] % 4 == 0, region=63 * sx + 1 <= LDS_ROWS)


def classify(om, case):
    """the class of every (angle, beam) entry as K2' decides it, with the window corner (gx, gy) in cells relative to the lattice's
    first pose.  dense_score: no block map, so no empty-window rule."""
    lat = lattice(om)
    table = om.lookup_table().astype(np.int64)
    na, n = table.shape
    ws = lat["ws"]
    bmin = lat["base0"]
    bmax = bmin + (lat["nx"] - 1) * lat["sx"] + (lat["ny"] - 1) * lat["sy_ws"]
    # the cell of every point: an estimate from the readings, made exact by the oracle's own index (idx = gx + gy * ws)
    ang = case.query.min_angle + np.arange(n) * case.query.ang_res
    r = np.where(np.isfinite(case.query.ranges), case.query.ranges, 0.0)
    lx, ly = r * np.cos(ang), r * np.sin(ang)
    cls = np.zeros((na, n), dtype=np.int8)
    gx = np.zeros((na, n), dtype=np.int64)
    gy = np.zeros((na, n), dtype=np.int64)
    for a in range(na):
        th = case.centre[2] - case.ang_off + a * case.ang_res
        ex = np.round((math.cos(th) * lx - math.sin(th) * ly) * lat["scale"]).astype(np.int64)
        ey = np.round((math.sin(th) * lx + math.cos(th) * ly) * lat["scale"]).astype(np.int64)
        idx = table[a]
        valid = idx != INVALID_SCAN
        y = np.floor_divide(idx - ex + ws // 2, ws)
        x = idx - y * ws
        assert (np.abs(x - ex)[valid] <= 1).all() and (np.abs(y - ey)[valid] <= 1).all(), "the oracle's index is not the point's cell"
        exact = np.abs(x) < (1 << 20)                      # (and gx + gy * ws == idx, which holds by construction: no int32 wrap in the table)
        assert (np.abs(x + y * ws)[valid] < (1 << 31) - 1).all()
        off = (idx + bmax < 0) | (idx + bmin >= lat["data_size"])
        inside = (idx + bmin >= -lat["pad"]) & (idx + bmax < lat["data_size"] + lat["pad"])
        cls[a] = np.where(~valid, INVALID, np.where(off, OFF, np.where(inside & exact, FAST, SLOW)))
        gx[a], gy[a] = x, y
    return dict(lat=lat, cls=cls, gx=gx, gy=gy, P=n, na=na)


def chunks(case, cl):
    """K2's greedy chunk builder: per angle pair, per builder wave, the chunk list; per angle, n_slow (the fallback's entries included)"""
    lat = cl["lat"]
    n, na, ws, base0 = cl["P"], cl["na"], lat["ws"], lat["base0"]
    row_waves = lds_row_waves(lat["ny"])
    read_rows = (16 * row_waves - 1) * lat["sy_cells"] + 1
    span_rows = (lat["ny"] - 1) * lat["sy_cells"] + 1
    n_slow = [int((cl["cls"][a] == SLOW).sum()) for a in range(na)]
    fallbacks = []
    groups = []
    for group in range((na + GROUP_ANGLES - 1) // GROUP_ANGLES):
        a0 = group * GROUP_ANGLES
        waves = [[] for _ in range(LDS_RANGES)]
        for run_lo in range(0, n, 64):                       # beam i: builder wave (i >> 6) & 3, round i >> 8
            wave = (run_lo >> 6) & 3
            n_run = min(64, n - run_lo)
            win = [[(int(cl["gx"][a0 + q, run_lo + k]), int(cl["gy"][a0 + q, run_lo + k]))
                    if a0 + q < na and cl["cls"][a0 + q, run_lo + k] == FAST else None for q in range(GROUP_ANGLES)] for k in range(n_run)]
            begin = 0
            while begin < n_run:
                while True:
                    xmin = ymin = None
                    xmax = ymax = None
                    state, end = None, n_run
                    for lane in range(begin, n_run):
                        for w in win[lane]:
                            if w is not None:
                                xmin = w[0] if xmin is None else min(xmin, w[0])
                                xmax = w[0] if xmax is None else max(xmax, w[0])
                                ymin = w[1] if ymin is None else min(ymin, w[1])
                                ymax = w[1] if ymax is None else max(ymax, w[1])
                        if xmin is not None:
                            al = (base0 + xmin) & 15
                            px0 = xmin - al
                            fits = xmax - px0 + TILE_BYTES <= LDS_PITCH and ymax - ymin + read_rows <= LDS_ROWS
                            if not fits:
                                end = lane
                                break
                            state = (px0, ymin, ymax, al, xmax)
                    if end > begin:
                        break
                    # beam `begin` alone does not fit: its windows at the two angles are too far apart
                    qd = 0
                    for q in range(1, GROUP_ANGLES):
                        if win[begin][q] is not None:
                            qd = q
                    assert win[begin][qd] is not None
                    win[begin][qd] = None
                    n_slow[a0 + qd] += 1
                    fallbacks.append((a0 + qd, run_lo + begin))
                if state is not None:
                    x0, y0, ymax_, al, xmax_ = state
                    cnt = [[0] * CLASSES for _ in range(GROUP_ANGLES)]
                    for lane in range(begin, end):
                        for q, w in enumerate(win[lane]):
                            if w is not None:
                                cnt[q][((w[1] - y0) * LDS_PITCH + (w[0] - x0)) & 3] += 1
                    waves[wave].append(dict(beam_begin=run_lo + begin, beams=end - begin, g0=y0 * ws + x0, rows=ymax_ - y0 + span_rows, cnt=cnt,
                                            windows=sum(map(sum, cnt)), al=al, x_extent=xmax_ - x0 + TILE_BYTES, y_extent=ymax_ - y0 + read_rows))
                begin = end
        groups.append(waves)
    return dict(groups=groups, n_slow=n_slow, fallbacks=fallbacks, row_waves=row_waves, read_rows=read_rows)


def deal(chunk_counts, parts, with_step_base=True):
    """K3's dealing of the steps of one angle among `parts` waves: {(chunk, class, step): [waves that take it]} for the class counts
    of the angle's chunks in order (score(): `first`, the loop over full steps, the tail step)"""
    taken = {}
    for part in range(parts):
        step_base = 0
        for ci, cnt4 in enumerate(chunk_counts):
            for c, cnt in enumerate(cnt4):
                first = (part - (step_base if with_step_base else 0)) & (parts - 1)
                step_base += (cnt + 3) >> 2
                k = 4 * first
                while k + 4 <= cnt:
                    taken.setdefault((ci, c, k // 4), []).append(part)
                    k += 4 * parts
                if k < cnt:
                    taken.setdefault((ci, c, k // 4), []).append(part)
    return taken


def region_bounds(cl, ch):
    """(lowest, highest) byte offset from the grid's first byte that K3's LDS-DMA of any chunk reads.

    A fast window has base0 + idx >= -pad and base0 + idx + (xs - 1) + (ys - 1) * ws < data_size + pad, pad = pad_rows * ws - 512
    (prepare_job: job.pad).  A region starts at the union's corner (ymin, xmin rounded down to 16 bytes): at most 128 + 15 bytes in
    front of the window in row ymin, so >= -pad - 143 > -(pad_rows * ws + 512) = the bytes in front of the grid at least
    (grid_pad = align_up(pad_rows * ws, 256) + 512).  Its last row is row ymax + ys - 1, read for 192 bytes from the aligned
    start: at most 191 bytes behind the last byte of the window in that row, so < data_size + pad + 191 < data_size + grid_pad.
    The tail DMA block re-reads the last 16-byte unit (clamped offsets)."""
    lat = cl["lat"]
    lo, hi = 0, 0
    for waves in ch["groups"]:
        for lst in waves:
            for d in lst:
                first = lat["base0"] + d["g0"]
                lo = min(lo, first)
                hi = max(hi, first + (d["rows"] - 1) * lat["ws"] + LDS_PITCH - 1)
    return lo, hi


def predict(case, cl, ch):
    """(does the forced search take the path, the value kh_matcher_score_loads reports for it if it does)"""
    lds = all(lds_rule(cl["lat"], cl["P"]).values())
    windows = sum(d["windows"] for waves in ch["groups"] for lst in waves for d in lst)
    return lds, 4 * ch["row_waves"] * windows


# ---------------------------------------------------------------- scans
G1 = (1.3, 0.01, 0.03, 12.0)          # 131 x 131 cells of search space: a two-cell lattice of 64 rows fits the probability grid
G2 = (0.3, 0.01, 0.03, 12.0)          # 31 cells of search space, 39 pad rows: a lattice of 64 rows is taller than the pad
CELL = 0.01


def _rings():
    """concentric rings every 0.1 m out to 5 m, and three at 10 m: something under every window the hand-built queries make"""
    return [ring_scan(0.3 + 0.1 * i) for i in range(48)] + [ring_scan(r, n=2048) for r in (9.9, 10.0, 10.1)]


def _edge():
    """the rings, and two at the range threshold: stamps in the array's first and last rows and columns"""
    return _rings() + [ring_scan(r, n=2048) for r in (11.9, 11.99)]


BASES = {"rings": _rings, "room": lambda: room_base(4, 181), "edge": _edge}


def line_scan(cells, heading=0.0, pose=(0.0, 0.0, 0.0)):
    """reading k lands cells[k] cells from the sensor along `heading` (NaN: an invalid reading): beams 1e-7 rad apart, so that the
    cross-axis cell is the sensor's own for every reading"""
    r = np.array([np.nan if (c is None or (isinstance(c, float) and math.isnan(c))) else (c + 0.2) * CELL for c in cells], dtype=np.float64)
    return ScanSpec(r, pose, heading, 1e-7)


def room(n, pose=(0.05, -0.15, 0.035)):
    q = room_scan((0.03, -0.12, 0.02), n, 7)
    return ScanSpec(q.ranges, pose, q.min_angle, q.ang_res)


def tails_query():
    """four runs of 64 readings, 22 usable each: per run the residues of the cell number mod 4 occur 5, 6, 7, 4 times, rotated by one
    from run to run -- whatever base0 is, every alignment class sees the remainders 1, 2, 3 and 0, and a run is 2 + 2 + 2 + 1 = 7
    steps: an odd count, so the running step number enters the next class, and the next chunk, at every phase"""
    cells = []
    for run in range(4):
        counts = [(5, 6, 7, 4)[(r + run) % 4] for r in range(4)]
        run_cells = [100.0 + 4 * m + r for r in range(4) for m in range(counts[r])]
        cells += run_cells + [None] * (64 - len(run_cells))
    return line_scan(cells)


def cases():
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    # ---- A. lattice: a room seen by 181 beams, three angles 0.02 rad apart
    q181 = room(181)
    for nx, ny in ((2, 64), (60, 1), (61, 16), (60, 17), (61, 31), (2, 32), (60, 33), (61, 63), (61, 64)):
        add(f"one-cell lattice {nx} x {ny}", "lattice", q181, "room", (nx, ny, 1), dict(lds=True, nx=nx, ny=ny, sx=1), na=3, ang_res=0.02)
    for nx, ny in ((30, 16), (31, 17), (30, 32), (31, 33), (31, 64)):
        add(f"two-cell lattice {nx} x {ny}", "lattice", q181, "room", (nx, ny, 2), dict(lds=True, nx=nx, ny=ny, sx=2), na=3, ang_res=0.02)
    # (the benchmark's config-2 shape, once: 61 x 61 poses, 81 angles, 1081 beams)
    add("config-2 shape", "lattice", room(1081), "room", (61, 61, 1), dict(lds=True, nx=61, ny=61, sx=1), na=81, ang_res=math.radians(0.5), pens=(True,))
    add("one-cell lattice 62 x 33", "past the limit", q181, "room", (62, 33, 1), dict(lds=False, only="nx"), na=3, ang_res=0.02)
    add("one-cell lattice 61 x 65", "past the limit", q181, "room", (61, 65, 1), dict(lds=False, only="ny"), na=3, ang_res=0.02)
    add("two-cell lattice 32 x 33", "past the limit", q181, "room", (32, 33, 2), dict(lds=False, only="nx"), na=3, ang_res=0.02)
    # ---- B. angles: an odd count leaves the last workgroup a dead second angle
    for na in (1, 2, 3, 9):
        add(f"{na} angles", "angles", q181, "room", (17, 31, 1), dict(lds=True, na=na, dead_angle=na % 2 == 1), na=na, ang_res=0.02)
    # ---- C. beams
    for n in (1, 63, 64, 65, 255, 256, 257, 1025, 2047, 2048):
        add(f"{n} beams", "beams", room(n), "room", (16, 17, 1), dict(lds=True, P=n), na=2, ang_res=0.02, pens=(True,))
    add("2049 beams", "past the limit", room(2049), "room", (16, 17, 1), dict(lds=False, only="P"), na=2, ang_res=0.02, pens=(True,))
    r512 = room(512)

    def with_nan(lo_hi):
        r = r512.ranges.copy()
        for lo, hi in lo_hi:
            r[lo:hi:2] = np.nan
            r[lo + 1:hi:2] = np.inf
        return ScanSpec(r, r512.pose, r512.min_angle, r512.ang_res)
    add("a run of 64 invalid", "invalid runs", with_nan([(64, 128)]), "room", (16, 17, 1), dict(lds=True, empty_runs=[64]), na=2, ang_res=0.02)
    add("a builder wave's share invalid", "invalid runs", with_nan([(128, 192), (384, 448)]), "room", (16, 17, 1),
        dict(lds=True, empty_wave=2), na=2, ang_res=0.02)
    add("every reading invalid", "invalid runs", with_nan([(0, 512)]), "room", (61, 33, 1), dict(lds=True, no_chunk=True, ties_over=TIE_CAP),
        na=2, ang_res=0.02)
    # ---- D1. every beam a chunk of its own: readings alternate between 1 m and 4 m
    for n in (256, 512):
        add(f"a chunk per beam, {n} beams", "chunk per beam", line_scan([100.0 + (k % 7) if k % 2 == 0 else 400.0 + (k % 5) for k in range(n)]), "rings",
            (9, 33, 1), dict(lds=True, capacity_full=True), na=2)
    # ---- D2. one chunk of 64 windows in one class: 16 full steps, no tail
    for nx, ny in ((61, 64), (9, 16), (9, 32)):
        add(f"64 windows on one cell, lattice {nx} x {ny}", "one chunk", line_scan([100.0] * 64), "rings", (nx, ny, 1),
            dict(lds=True, one_chunk=64), na=2)
    # ---- D3. tails, for parts = 4, 2 and kFull
    for ny, parts in ((16, 4), (32, 2), (40, 1)):
        add(f"tails of every class, {ny} rows", "tails", tails_query(), "rings", (9, ny, 1), dict(lds=True, parts=parts), na=2)
    add("tails of every class, two-cell lattice", "tails", tails_query(), "rings", (9, 16, 2), dict(lds=True, parts=4), na=3)
    # ---- D4. region limits: two beams, the union at the limit and one cell further.  (base0 + 100) & 15 of these searches is recorded
    # in X_AL: the first beam's cell is chosen for al = 0 and al = 15
    for al in (0, 15):
        x1 = 100 + ((al - X_AL) % 16)
        for more in (0, 1):
            add(f"x limit, al = {al}" + (", one further" if more else ""), "region x", line_scan([x1, x1 + 128 - al + more]), "rings", (9, 9, 1),
                dict(lds=True, al=al, n_chunks=1 + more, x_extent=LDS_PITCH if not more else None), pens=(True,))
    for ny, read_rows in ((16, 16), (32, 32), (64, 64)):
        for more in (0, 1):
            add(f"y limit, {ny} rows" + (", one further" if more else ""), "region y", line_scan([100.0, 100.0 + LDS_ROWS - read_rows + more], heading=0.5 * math.pi),
                "rings", (9, ny, 1), dict(lds=True, read_rows=read_rows, n_chunks=1 + more, y_extent=LDS_ROWS if not more else None), pens=(True,))
    # ---- D5. fallback: a beam at 10 m, angles 0.2 rad apart: its two windows lie 200 rows apart
    for at in (64, 30):
        cells = [100.0 + (k % 50) for k in range(128)]
        cells[at] = 1000.0
        add(f"far beam at {at}", "fallback", line_scan(cells), "rings", (9, 33, 1), dict(lds=True, n_slow=(0, 1), fallbacks=[(1, at)]), na=2, ang_res=0.2)
    add("far beam, three angles", "fallback", line_scan([100.0] * 10 + [1000.0] + [100.0] * 10), "rings", (9, 33, 1),
        dict(lds=True, n_slow=(0, 1, 0), fallbacks=[(1, 10)]), na=3, ang_res=0.2)
    # ---- E. array edges: a fine search of 64 rows on the handle whose pad is 39 rows, its lattice at the array's first rows; readings
    # that point down the rows (towards lower addresses) from 0 to 30 m
    for name, sign in (("front", -1.0), ("back", 1.0)):
        edge = line_scan([float(c) for c in E_CELLS], heading=sign * 0.5 * math.pi)
        add(f"windows off the array's {name}", "array edges", edge, "edge", (9, 64, 1), dict(lds=True, classes={OFF, SLOW, FAST}, outside=name), na=2,
            create=G2, fine=True, centre=(0.0, sign * E_CENTRE_Y, 0.0), dense=(True, False))
    # windows that run over a row end: readings along +x up to the array's last columns and beyond
    add("windows over a row end", "array edges", line_scan([float(c) for c in W_CELLS]), "edge", (61, 9, 1), dict(lds=True, wraps=True), na=2,
        create=G2, fine=True, dense=(True, False))
    return out


# found by sweeps over the restated builder on the CPU (tests/test_lds_cases_oracle.py checks what they give)
X_AL = 8                       # (base0 + 100) & 15 of the 9 x 9 one-cell search centred on a query at the origin (G1)
E_CENTRE_Y = 11.845            # the 64-row lattice starts in the array's first row of the region of interest (ends in its last)
E_CELLS = tuple(range(0, 80)) + (100, 500, 1000, 2000, 3000)
W_CELLS = tuple(range(1100, 1300, 3))


# ---------------------------------------------------------------- F. batches
BATCH_BEAMS = (64, 257, 1081)


def batch_jobs(n):
    """n searches for ONE CorrelateScanBatch (same lattice and angles, as a batch has them): queries of 64, 257 and 1081 beams mixed,
    each from a pose of its own"""
    return [Case(f"batch of {n}, job {i}", "batch", room(BATCH_BEAMS[i % 3], pose=(0.05 + 0.013 * i, -0.15 + 0.007 * i, 0.035 - 0.004 * i)), "room",
                 (31, 33, 1), dict(lds=True), na=3, ang_res=0.02, pens=(True,)) for i in range(n)]


# ---------------------------------------------------------------- G. column-decimated copies, then a small two-cell search
def pick_ry(ny):
    """pick_ry (matcher_host.cpp): rows per lane of the windowed kernel"""
    if ny <= 4:
        return 1
    best, best_cost = 8, 1 << 30
    for ry in (8, 7, 4):
        cost = ((ny + 4 * ry - 1) // (4 * ry)) * ry
        if cost < best_cost:
            best, best_cost = ry, cost
    return best


def copies_kind(lat, n_beams):
    """ensure_slot_scratch: the copies a slot WITHOUT any is given by this search (0 none, 1 re-pitched, 2 column-decimated)"""
    nx, ny = lat["nx"], lat["ny"]
    lt = ((nx + 30) // 31) * ((ny + 4 * pick_ry(ny) - 1) // (4 * pick_ry(ny)))
    if lt > 32:
        lt = 1
    work = float(nx) * ny * lat["na"] * n_beams
    step = lat["sx"] if lat["linear"] else 0
    full_res = nx > 1 and step == 1 and nx <= TILE_SPAN
    tiled = lt > 1 and step in (1, 2)
    if not ((full_res or tiled) and work >= 1e8):
        return 0
    return 2 if (step == 2 and lat["ws"] % 8 == 0) else 1


def dec_rule(lat, slot_copy_kind):
    """prepare_job: is the search scored from the column-decimated copies by the windowed kernel (CorrJob::dec), one tile column"""
    return slot_copy_kind == 2 and lat["linear"] and lat["sx"] == 2 and lat["sy_ws"] % lat["ws"] == 0 and lat["nx"] <= TILE_SPAN


def lds_by_default(lat, n_beams, n_launch):
    """prepare_job's lds_wanted with no debug bit set"""
    return float(lat["nx"]) * lat["ny"] * lat["na"] * n_beams >= 1e8 and float(n_launch) * lat["na"] >= 1024.0


DEFAULT_BATCH = 8


def decimated_cases():
    """(large, small, [jobs of the default-route batch]): see tests/test_lds_edges_gpu.py::test_small_two_cell_search_on_a_slot_with_decimated_copies"""
    large = Case("two-cell search that allocates the copies", "decimated", room(1081), "room", (66, 66, 2), dict(copies=2), na=23, ang_res=0.03, pens=(False,))
    small = Case("small two-cell search, path forced", "decimated", room(181), "room", (31, 33, 2), dict(lds=True, dec=True), na=3, ang_res=0.02)
    jobs = [Case(f"two-cell search of a default-route batch, job {i}", "decimated", room(400, pose=(0.05 + 0.013 * (i % 2), -0.15, 0.035)), "room", (31, 64, 2),
                 dict(lds=True, dec=True, copies=2, default=True), na=129, ang_res=0.005, pens=(False,)) for i in range(DEFAULT_BATCH)]
    return large, small, jobs
