"""TEST INFRASTRUCTURE: edge cases of the fused path of ONE MatchScan (csrc/matcher_seq.cpp + the kseq_* kernels of csrc/matcher_seq.hip).

A table of named cases (cases()), the restated rules that say which way a call must go (refusal(), predict()), and the CPU oracle's
MatchScan taken apart pass by pass (stages()) so that tie counts, lattice sizes and the fine pass's average can be read from its
volumes.  tests/test_seq_cases_oracle.py proves on the CPU that every case sits on the edge its probe names;
tests/test_seq_edges_gpu.py walks the table on the device.  Nothing here calls the library.

What the table found out about the path while it was written (DESIGN.md section 3a has the same list):

* MatchScan never runs FindValidPoints on the QUERY (Mapper.cpp:534-639): every reading is a point of the lookup table, NaN / inf
  readings become INVALID_SCAN entries, readings beyond the range threshold are ordinary points that fall on empty cells.  kseq_score
  and kseq_fine cut the READINGS into slices of 64, so the slice edges are hit by queries of 1, 63, 64, 65 and 129 readings
  ("slice readings") -- and, separately, by longer queries with that many usable readings in between invalid ones ("slice valid").
* A base scan counts against kSeqMaxScans when it has a points array and n > 0: an all-NaN scan counts, an empty one does not.
* FindValidPoints keeps a reading only once a later reading lies more than 0.1 m from the run's first: a scan of ONE reading keeps
  nothing.  The one-candidate case is a scan of two readings 0.5 m apart, of which the first is kept.
* Coarse tie counts: the wall scene gives nx (16 on the K lattice) times the tied rows and angles -- a few dozen.  Counts at kTieCap
  are reached with a query that sees nothing (every pose ties at response 0): 16 x 16 x 8 = 2048 exactly; 2049 = 3 x 683 is
  nx * nx * na only for a lattice of ONE position with 2049 angles, which is no search: the nearest count above the cap is
  5 x 5 x 82 = 2050, and 16 x 16 x 9 = 2304 is the 2048 lattice with one more angle.
* The fine pass's tie average cannot leave the 3 x 3 lattice: see fine_average_on_lattice().
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from common import OFFLINE_PARAMS, PRESETS
from slam_toolbox_amd import synth

# ---------------------------------------------------------------- the limits, restated (matcher_seq.hpp, kh_internal.hpp, plan_table_raster)
MAX_READINGS = 2048       # kSeqMaxReadings
MAX_SCANS = 128           # kSeqMaxScans
MAX_POINTS = 131072       # kSeqMaxPoints
MAX_TILES = 16384         # kSeqMaxTiles
MAX_FINE = 1024           # kSeqMaxFine: poses of the fine volume (9 per angle: 113 angles)
TIE_CAP = 2048            # kTieCap
SLICE = 64                # kSeqSlice
BIN_REGS = 8192           # kseq_bin: 1024 threads x kBinRegs candidates in registers
CLEAR_WAVES = 2048        # prep_clear: 128 workgroups x 16 waves
TILE = 64                 # kRasterTile
LDS_RULE = 150 * 1024
TOLERANCE = 1e-6          # KT_TOLERANCE

KINDS = ("readings", "scans", "points", "lds", "tiles", "reason 1", "slice readings", "slice valid", "candidates", "clear", "coarse ties",
         "tie cap", "fine lattice", "fine ties", "expansion")

Lz = namedtuple("Lz", "min_angle ang_res")


class ScanSpec:
    """range readings + sensor pose + angular layout; n = 0: an empty scan"""

    def __init__(self, ranges, pose, min_angle, ang_res):
        self.ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        self.pose = np.asarray(pose, dtype=np.float64)
        self.min_angle, self.ang_res = float(min_angle), float(ang_res)
        self.n = self.ranges.shape[0]

    def oracle(self):
        from oracle import karto
        return karto.Scan(self.ranges, self.pose, Lz(self.min_angle, self.ang_res))

    def hip(self):
        from slam_toolbox_amd.scan_matcher import LocalizedRangeScan
        return LocalizedRangeScan(self.ranges, self.pose, self.min_angle, self.ang_res)


class Case:
    def __init__(self, name, kind, query, base, probe, preset="K", create=None, params=None, pairs=((True, True), (False, True), (True, False)),
                 debug=False):
        self.name, self.kind, self.query, self.base, self.probe, self.debug = name, kind, query, list(base), dict(probe), debug
        self.create = tuple(PRESETS[preset]["create"] if create is None else create)
        self.params = dict(PRESETS[preset]["params"] if params is None else params)
        self.pairs = tuple(pairs)

    def geometry(self):
        return self.create, tuple(sorted(self.params.items()))

    def oracle_matcher(self):
        from oracle import karto
        return karto.Matcher(*self.create, self.params)

    def hip_matcher(self):
        from slam_toolbox_amd.scan_matcher import MapperParams, ScanMatcher
        return ScanMatcher.Create(MapperParams(**self.params), *self.create)

    def n_scans(self):
        return sum(1 for b in self.base if b.n > 0)

    def n_points(self):
        return sum(b.n for b in self.base)


def round_half_away(v):
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


# ---------------------------------------------------------------- geometry of a matcher, from what the oracle matcher reports
def geometry(om):
    """grid, tiles, block map and 100-footprint of a matcher (kh_matcher_create, restated over the oracle's grid_info and kernel)"""
    g = om.grid_info()
    kernel = om.kernel()
    side = om.probs().shape[0]
    ws, height = g["width_step"], g["data_size"] // g["width_step"]
    bshift = 5                                    # kBlockShift (8 x 8 blocks only on handles made for batches of >= 8)
    return dict(ws=ws, height=height, tiles=((ws + TILE - 1) // TILE) * ((height + TILE - 1) // TILE), n_foot=int((kernel == 100).sum()) - 1,
                bm_words=((((ws >> bshift) + 1) + 31) // 32 + 1) * ((height >> bshift) + 2), kernel_size=g["kernel_size"], side=side,
                nx=(side - 1) // 2 + 1, roi_w=g["roi_w"], roi_x=g["roi_x"], roi_y=g["roi_y"], scale=g["scale"])


def seq_bin_lds_bytes(n_points, n_foot, tiles, bm_words):
    state = ((n_points + 15) & ~15) if n_foot > 0 else 0
    return state + 4 * tiles + 4 * max(bm_words, 0) + 16


def lds_plan(n_points, geo):
    """(bytes, bm_global, fits) of kseq_bin for a job, as plan_table_raster decides"""
    b = seq_bin_lds_bytes(n_points, geo["n_foot"], geo["tiles"], geo["bm_words"])
    bm_global = b > LDS_RULE
    if bm_global:
        b = seq_bin_lds_bytes(n_points, geo["n_foot"], geo["tiles"], 0)
    return b, bm_global, b <= LDS_RULE


def refusal(case, geo):
    """the reason seq_match refuses the call with (0: it takes it), in seq_match's order"""
    if case.debug:
        return 1
    if case.query.n <= 0 or case.query.n > MAX_READINGS:
        return 2
    scans = [b for b in case.base if b.n > 0]
    if not scans:
        return 4
    if max(b.n for b in scans) > MAX_READINGS:
        return 3
    if len(scans) > MAX_SCANS or case.n_points() > MAX_POINTS or geo["tiles"] > MAX_TILES:
        return 5
    if not lds_plan(case.n_points(), geo)[2]:
        return 6
    return 0


def fine_angles(params):
    """angles of the fine pass: fine_search (half the coarse resolution either side, fine_search_angle_offset apart) through init_ctx"""
    ang_off = 0.5 * params["coarse_angle_resolution"]
    return int(round_half_away(ang_off * 2.0 / params["fine_search_angle_offset"]) + 1)


def coarse_angles(params):
    return int(round_half_away(params["coarse_search_angle_offset"] * 2.0 / params["coarse_angle_resolution"]) + 1)


# ---------------------------------------------------------------- the oracle's MatchScan, pass by pass
def _ties(vol):
    r = vol[..., 0]
    best = r.max()
    d = r - best
    return best, np.where(d < 0.0, d >= -TOLERANCE, d <= TOLERANCE)


def fine_average_on_lattice(om, vol, mask):
    """Is the cell of the fine pass's tie average one of the lattice's cells (finalize_job: otherwise the column of sums is rescored)?

    It always is when the lattice's cells are neighbours: the mean of points of a 3 x 3 block of adjacent cells lies in their hull and
    rounds to a cell of the block.  The fine lattice is centre + {-res, 0, +res}; its cells are neighbours unless the centre sits on
    a cell boundary, and the centre is a coarse lattice pose or a mean of coarse lattice poses two cells apart.  On the device's fine
    pass the centre is ONE coarse pose -- a cell centre: finalize_job's kNeedGeneric for an off-lattice average cannot be reached
    there, and no case of the table gets the general path to it either (the CPU file asserts what each case does)."""
    g = om.grid_info()

    def cell(x, y):
        return (round_half_away((x - g["offset_x"]) * g["scale"]), round_half_away((y - g["offset_y"]) * g["scale"]))
    lattice = {cell(x, y) for x, y in vol[..., 0, 1:3].reshape(-1, 2)}
    n = int(mask.sum())
    ax, ay = 0.0, 0.0
    for x, y in vol[mask][:, 1:3]:          # (y, x, a) order: the reference's
        ax += x
        ay += y
    return cell(ax / n, ay / n) in lattice


def stages(om, case, penalize, refine):
    """ko_match_scan in Python over the oracle's own CorrelateScan: result, grid, last lookup table and what the route depends on"""
    q = case.query.oracle()
    base = [b.oracle() for b in case.base]
    p = case.params
    om.add_scans(q, base)
    out = dict(grid=om.grid())
    res = 1.0 / om.grid_info()["scale"]
    side = om.probs().shape[0]
    cso, csr = 0.5 * (float(side) - 1) * res, 2 * res
    ang_off = p["coarse_search_angle_offset"]
    r, mean, cov = om.correlate_scan(q, q.sensor_pose, (cso, cso), (csr, csr), ang_off, p["coarse_angle_resolution"], penalize, False)
    vol = om.volume()
    _, mask = _ties(vol)
    out.update(coarse_response=r, coarse_ties=int(mask.sum()), coarse_shape=vol.shape[:3], expansions=0)
    if p["use_response_expansion"] and abs(r) <= TOLERANCE:
        for _ in range(3):
            ang_off += 20 * 0.01745329251994329577
            r, mean, cov = om.correlate_scan(q, q.sensor_pose, (cso, cso), (csr, csr), ang_off, p["coarse_angle_resolution"], penalize, False)
            out["expansions"] += 1
            if abs(r) > TOLERANCE:
                break
    if refine:
        r, mean, cov = om.correlate_scan(q, mean.copy(), (csr * 0.5, csr * 0.5), (res, res), 0.5 * p["coarse_angle_resolution"],
                                         p["fine_search_angle_offset"], penalize, True, cov_in=cov)
        vol = om.volume()
        _, mask = _ties(vol)
        out.update(fine_shape=vol.shape[:3], fine_ties=int(mask.sum()), fine_tie_cells=len({(y, x) for y, x, _ in zip(*np.nonzero(mask))}),
                   fine_on_lattice=fine_average_on_lattice(om, vol, mask))
    out.update(result=(r, mean, cov), lookup=om.lookup_table())
    return out


STAT_KEYS = ("calls", "fine_on_device", "fine_fallbacks", "fine_mismatches", "coarse_fallbacks", "fused_score", "ineligible", "ineligible_reason")


def predict(stats, case, geo, st, refine):
    """adds to `stats` what ONE kh_matcher_match of `case` must add to seq_stats(): seq_match's branches over the oracle's volumes"""
    reason = refusal(case, geo)
    if reason:
        stats["ineligible"] += 1
        stats["ineligible_reason"] = reason
        return stats
    stats["calls"] += 1
    stats["fused_score"] += 1                     # the coarse lattice steps two cells inside the grid: linear, kseq_score takes it
    if st["coarse_ties"] > TIE_CAP:
        stats["coarse_fallbacks"] += 1            # the tie list does not hold them: the general path redoes the pass
        return stats
    if not refine:
        return stats
    if case.params["use_response_expansion"] and abs(st["coarse_response"]) <= TOLERANCE:
        return stats                              # the general path's business, no counter
    device_fine = st["fine_shape"][0] == 3 and st["fine_shape"][1] == 3 and st["fine_shape"][2] * 9 <= MAX_FINE
    if not device_fine or st["coarse_ties"] != 1:
        stats["fine_fallbacks"] += 1
    elif not st["fine_on_lattice"]:
        stats["fine_fallbacks"] += 1
    else:
        stats["fine_on_device"] += 1
    return stats


def zero_stats():
    return {k: 0 for k in STAT_KEYS}


# ---------------------------------------------------------------- scenes
_ROOM = np.asarray(synth._rect(-3.0, -2.0, 3.0, 2.0) + synth._rect(1.0, 0.8, 1.4, 1.2) + synth._rect(-2.0, -1.2, -1.6, -0.7)
                   + synth._rect(-0.9, 1.1, -0.6, 1.6), dtype=np.float64)


def room_scan(pose, n, seed, fov=math.radians(270.0), noise=0.004):
    """n beams over `fov` in a 6 m x 4 m room with three pillars, a little noise on the ranges (ties are for the cases that want them)"""
    ang_res = fov / max(n - 1, 1)
    laser = synth.Laser(n_beams=n, min_angle=-0.5 * fov, max_angle=0.5 * fov, ang_res=ang_res)
    r = synth.raycast(_ROOM, pose, laser)
    r = r + np.random.default_rng(seed).normal(0.0, noise, size=r.shape)
    return ScanSpec(r, pose, laser.min_angle, ang_res)


def room_base(n_scans, n, seed=100):
    """base scans along a short drive through the room"""
    return [room_scan((-0.6 + 0.1 * (i % 12), -0.2 + 0.02 * (i % 7), 0.05 * ((i % 5) - 2)), n, seed + i) for i in range(n_scans)]


ROOM_QUERY_POSE = (0.03, -0.12, 0.02)
ROOM_QUERY_GUESS = (0.05, -0.15, 0.035)


def room_query(n, seed=7, fov=math.radians(270.0)):
    q = room_scan(ROOM_QUERY_POSE, n, seed, fov)
    return ScanSpec(q.ranges, ROOM_QUERY_GUESS, q.min_angle, q.ang_res)


def wall_scan(x, n, half_width, d=1.0, side=1.0, y=0.0):
    """sensor at (x, y) heading 0, a straight wall parallel to x at y + side * d seen from end to end by n beams"""
    a0 = math.atan2(d, half_width)
    ang = a0 + np.arange(n) * ((math.pi - 2 * a0) / (n - 1))
    ranges = d / np.sin(ang)
    if side < 0:
        return ScanSpec(ranges[::-1].copy(), (x, y, 0.0), -(math.pi - a0), (math.pi - 2 * a0) / (n - 1))
    return ScanSpec(ranges, (x, y, 0.0), a0, (math.pi - 2 * a0) / (n - 1))


def wall_base():
    """two dense scans of the wall y = 1 from x = -0.5 and +0.5: every 1 cm cell of the row from x = -3 to 3 gets a reading"""
    return [wall_scan(-0.5, 2048, 2.5), wall_scan(0.5, 2048, 2.5)]


def wall_query(guess=(0.0, 0.03, 0.0), n=65, side=1.0):
    """65 beams, 60 degrees wide, that see only the wall, 1 m away; the pose guess is off by `guess`"""
    q = wall_scan(0.0, n, math.tan(math.radians(30.0)), side=side)
    return ScanSpec(q.ranges, guess, q.min_angle, q.ang_res)


def arc_scan(radius, n=2048, pose=(0.0, 0.0, 0.0), fov=math.radians(270.0)):
    """every beam at the same range: n points on an arc"""
    return ScanSpec(np.full(n, float(radius)), pose, -0.5 * fov, fov / (n - 1))


def ring_scan(radius, n=512):
    return ScanSpec(np.full(n, float(radius)), (0.0, 0.0, 0.0), -math.pi, 2 * math.pi / n)


def sprinkle(ranges, keep, seed):
    """all but `keep` of the readings made NaN / inf, interleaved with the kept ones and trailing (the last eighth is all invalid)"""
    r = np.array(ranges, dtype=np.float64)
    n = r.shape[0]
    rng = np.random.default_rng(seed)
    body = n - n // 8
    kept = np.sort(rng.choice(body, size=keep, replace=False))
    bad = np.ones(n, dtype=bool)
    bad[kept] = False
    idx = np.nonzero(bad)[0]
    r[idx[0::2]] = np.nan
    r[idx[1::2]] = np.inf
    return r, kept


K_SMALL = dict(create=(0.1, 0.01, 0.03, 12.0), params=PRESETS["K"]["params"])      # 6 x 6 coarse poses: 36 x 21 = 756 poses in all
ALL = ((True, True), (False, True), (True, False))
ONE = ((True, True),)


def cases():
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    # ---- readings (reasons 2 and 3): the room, K
    base4 = room_base(4, 181)
    for n, reason in ((2048, 0), (2049, 2)):
        add(f"query of {n} readings", "readings", room_query(n), base4, dict(limit="query readings", n=n, reason=reason), pairs=ONE)
    for n, reason in ((2048, 0), (2049, 3)):
        add(f"base scan of {n} readings", "readings", room_query(181), base4[:2] + [room_scan((0.2, 0.1, -0.05), n, 55)] + base4[2:],
            dict(limit="base readings", n=n, reason=reason), pairs=ONE)
    # ---- scans (reason 5): short scans of 16 readings
    short = room_base(129, 16, seed=300)
    empty = ScanSpec(np.zeros(0), (0.0, 0.0, 0.0), 0.0, 0.1)
    all_nan = ScanSpec(np.full(16, np.nan), (0.1, 0.0, 0.0), -1.0, 0.1)
    add("128 base scans", "scans", room_query(181), short[:128], dict(limit="scans", scans=128, listed=128, reason=0), pairs=ONE)
    add("129 base scans", "scans", room_query(181), short, dict(limit="scans", scans=129, listed=129, reason=5), pairs=ONE)
    # an empty scan (n = 0) is skipped like a NULL one; an all-NaN scan has readings and counts, though FindValidPoints keeps none
    add("129 listed: one empty, one all-NaN", "scans", room_query(181), short[:60] + [empty] + short[60:100] + [all_nan] + short[100:127],
        dict(limit="scans", scans=128, listed=129, reason=0, counts="all-NaN", skipped="empty"), pairs=ONE)
    add("128 scans between empty ones", "scans", room_query(181), [empty] + short[:50] + [empty, empty] + short[50:128] + [empty],
        dict(limit="scans", scans=128, listed=132, reason=0, empty_at=(0, 51, 52, 131)), pairs=ONE)
    # ---- points (reason 5) and the LDS rule (reason 6).  S: n_foot = 4, a state byte per point; K: n_foot = 0.
    arcs = [arc_scan(2.0 + 0.05 * i) for i in range(64)]
    one_more = [ScanSpec(np.array([1.5]), (0.0, 0.0, 0.0), 0.0, 0.1)]
    for preset in ("S", "K"):
        add(f"131072 points ({preset})", "points", room_query(65), arcs, dict(limit="points", points=MAX_POINTS, reason=0), preset=preset, pairs=ONE)
        add(f"131073 points ({preset})", "points", room_query(65), arcs + one_more, dict(limit="points", points=MAX_POINTS + 1, reason=5), preset=preset,
            pairs=ONE)
    # 0.01 m cells, smear 0.1 (n_foot = 4), range threshold 24: 77 x 77 tiles; the state bytes fill the LDS before kSeqMaxPoints
    lds_geo = dict(create=(0.5, 0.01, 0.1, 24.0), params=OFFLINE_PARAMS)
    for n, reason in ((129856, 0), (129857, 6)):
        add(f"{n} points under the LDS rule", "lds", room_query(65), arcs[:63] + [arc_scan(5.5, n - 63 * 2048)],
            dict(limit="lds", points=n, reason=reason, bm_global=True), pairs=ONE, **lds_geo)
    # ---- tiles (reason 5): 0.005 m cells; 128 x 128 tiles exactly, then one step of the range threshold more
    for rt, tiles, reason in ((4051.5 * 0.005, 16384, 0), (4052.5 * 0.005, 16641, 5)):
        add(f"{tiles} tiles", "tiles", room_query(65), room_base(3, 91), dict(limit="tiles", tiles=tiles, reason=reason), pairs=ONE,
            create=(0.3, 0.005, 0.03, rt), params=PRESETS["C2"]["params"])
    # ---- reason 1
    add("response volume kept (debug)", "reason 1", room_query(181), base4, dict(reason=1), debug=True)
    # ---- query slices
    for n in (1, 63, 64, 65, 129):
        add(f"query of {n} readings", "slice readings", room_query(n, fov=math.radians(200.0)), base4, dict(readings=n, reason=0))
    for keep in (1, 63, 64, 65, 129):
        q = room_query(200)
        r, kept = sprinkle(q.ranges, keep, seed=keep)
        beyond = kept[::7][:max(0, keep // 8)]            # some kept readings beyond the range threshold: finite, so they ARE scored
        r[beyond] = 13.0 + 0.1 * np.arange(beyond.size)
        add(f"query with {keep} usable readings of 200", "slice valid", ScanSpec(r, q.pose, q.min_angle, q.ang_res), base4,
            dict(readings=200, usable=keep, beyond_threshold=int(beyond.size), reason=0))
    # ---- candidates
    # (the query's three beams see the one stamp: a unique coarse pose, and a fine pass ON THE DEVICE whose best response is shared by
    # several cells of the 3 x 3 lattice)
    add("one stamp candidate", "candidates", ScanSpec(np.array([1.0, 1.1, 1.3]), (0.02, -0.01, 0.0), 0.5, 0.5),
        [ScanSpec(np.array([1.0, 1.1]), (0.0, 0.0, 0.0), 0.5, 0.5)], dict(candidates=1, fine_tie_cells_over=1, on_device=True, reason=0))
    many = [arc_scan(2.0 + 0.4 * i) for i in range(6)]
    add("over 8192 candidates, n_foot = 4 (S)", "candidates", room_query(65), many, dict(candidates_over=BIN_REGS, n_foot=4, reason=0), preset="S", pairs=ONE)
    add("over 8192 candidates, n_foot = 0 (K)", "candidates", room_query(65), many, dict(candidates_over=BIN_REGS, n_foot=0, reason=0), preset="K", pairs=ONE)
    add("over 8192 candidates, n_foot = 0, 3 x 3 smear (L)", "candidates", room_query(65), [arc_scan(8.0 + i) for i in range(12)],
        dict(candidates_over=BIN_REGS, n_foot=0, reason=0), preset="L", pairs=ONE)
    # ---- clear: rings every 0.6 m out to 19.8 m write over half of S's 4096 tiles; then one short scan elsewhere
    centre = ScanSpec(room_query(65).ranges, (0.0, 0.0, 0.0), room_query(65).min_angle, room_query(65).ang_res)
    add("clear a: over 2048 tiles written", "clear", centre, [ring_scan(0.6 * (i + 1)) for i in range(33)], dict(tiles_over=CLEAR_WAVES, reason=0),
        preset="S", pairs=ONE)
    add("clear b: one short scan elsewhere", "clear", ScanSpec(centre.ranges, (3.0, -2.0, 0.0), centre.min_angle, centre.ang_res),
        [ScanSpec(np.full(16, 1.5), (3.0, -2.0, 0.0), 0.2, 0.05)], dict(tiles_at_most=9, reason=0), preset="S", pairs=ONE)
    # ---- coarse ties: one straight wall, translation-invariant along x over the whole search
    add("wall, no penalties", "coarse ties", wall_query(), wall_base(), dict(ties=(2, TIE_CAP), penalize=False, reason=0), pairs=((False, True), (False, False)))
    add("wall, penalties", "coarse ties", wall_query(), wall_base(), dict(ties="recorded", penalize=True, reason=0), pairs=((True, True),))
    # ---- at and past kTieCap: a query that looks away from everything rasterised, every pose ties at 0 (expansion off)
    away = wall_query(side=-1.0)
    for n_ang, nx, search, ties in ((8, 16, 0.3, 2048), (82, 5, 0.08, 2050), (9, 16, 0.3, 2304)):
        prm = dict(PRESETS["K"]["params"], coarse_search_angle_offset=0.5 * (n_ang - 1) * 0.0349)
        add(f"{ties} coarse ties", "tie cap", away, wall_base(), dict(ties=ties, nx=nx, na=n_ang, reason=0), create=(search, 0.01, 0.03, 12.0), params=prm,
            pairs=((True, True), (True, False)))
    # ---- fine lattice: 113 angles (1017 poses) fit kSeqMaxFine, 114 (1026) and 115 do not
    for n_ang in (113, 114, 115):
        prm = dict(PRESETS["K"]["params"], fine_search_angle_offset=0.0349 / (n_ang - 1))
        add(f"{n_ang} fine angles", "fine lattice", room_query(181), base4, dict(fine_angles=n_ang, on_device=n_ang * 9 <= MAX_FINE, reason=0), params=prm, pairs=ONE)
    # ---- fine ties: along the wall the fine pass ties too (general path: the coarse pass had several best poses); in the room the device's
    # fine pass has its ties along the angle axis only
    add("wall: fine ties over several cells", "fine ties", wall_query(), wall_base(), dict(fine_tie_cells_over=1, on_lattice=True, reason=0),
        pairs=((False, True),))
    prm = dict(PRESETS["K"]["params"], fine_search_angle_offset=0.0349 / 112)
    for beams, pen in ((3, True), (5, False)):
        add(f"room, {beams} beams: fine ties along the angle", "fine ties", room_query(beams), base4,
            dict(fine_ties_over=1, on_lattice=True, on_device=True, reason=0), params=prm, pairs=((pen, True),))
    # ---- response expansion: the coarse pass finishes on the fused path with response 0 (756 ties fit the list)
    for expansion in (True, False):
        prm = dict(PRESETS["K"]["params"], use_response_expansion=expansion)
        add(f"response 0, expansion {'on' if expansion else 'off'}", "expansion", away, wall_base(), dict(response=0.0, ties=756, expansion=expansion, reason=0),
            create=K_SMALL["create"], params=prm, pairs=((True, True), (True, False)))
    return out


# cases run one after the other on ONE handle: a refused call (or a large one) must leave the handle right for the next
SEQUENCES = (
    ("clear", ("clear a: over 2048 tiles written", "clear b: one short scan elsewhere", "clear a: over 2048 tiles written")),
    ("query readings", ("query of 2048 readings", "query of 2049 readings", "query of 2048 readings")),
    ("base readings", ("base scan of 2048 readings", "base scan of 2049 readings", "base scan of 2048 readings")),
    ("scans", ("128 base scans", "129 base scans", "128 scans between empty ones")),
    ("points", ("131072 points (S)", "131073 points (S)", "131072 points (S)")),
    ("lds", ("129856 points under the LDS rule", "129857 points under the LDS rule", "129856 points under the LDS rule")),
)
