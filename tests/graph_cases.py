"""Edge inputs of the graph-store kernels (k_loop_candidates, k_near_by_scan, k_near_by_radius, csrc/graph.hip) as plain data,
independent of the library: what tests/test_edge_cases_oracle.py runs through oracle/loops.py and tests/near_by_rule.py alone
(does every case still sit on the edge its name says?) and tests/test_graph_edges_gpu.py through the kernels next to them.

A loop case is (name, ref_xy, adj_ptr, adj_idx, queries, starts | None, n_visit | None, max_distance, min_chain, check):
`check(chains)` asserts, on the ORACLE's chains (one list of (first, last) per query), that the case sits on its edge.  Every
batch holds at least two queries, so the library answers it with the kernel; the GPU side also asks each query alone (the host
route).  Most graphs are written as a pattern, one letter per scan: Q the query at (0, 0); g a good scan (in range, no path of
links to Q); l a scan linked to Q; o a scan out of range.  Coordinates are exactly representable; where a threshold is the
subject, one coordinate is the double that puts the squared distance on the wanted side of it, one ulp apart.

A near-by case is (name, poses, queries, radii, check): `check(res)` gets, per query, the squared distances to every pose, the
nearest (index, dist_sq) and the hits per radius, all from tests/near_by_rule.py (which the CPU suite pins to nanoflann, with
the library's documented rule between equal distances: the lower index).  Equal distances are the SUBJECT here, so the
best_two_differ / hits_are_distinct guards of the random test are not applied.

The capped launch: k_near_by_radius runs on min(ceil(n / 256), 256) workgroups of 256, so its strided loop takes a second trip from
65 537 vertices on (NEAR_TRIP = 65 536); the size, tie and radius cases hold 1281 vertices at the most, near_trip_cases() holds
stores on either side of one and two trips.  k_near_by_scan is one workgroup per query whose loop of 1024 vertices a round the size
cases take into a second round at 1025 and 1281 vertices, and the trip cases through up to 129.

Not tested: non-finite poses or queries (NaN, and infinities as coordinates): nanoflann's answer to a NaN depends on the shape
of its tree, so there is no reference to hold the kernels to."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle.loops import KT_TOLERANCE, squared_distance

LoopCase = namedtuple("LoopCase", "name ref_xy adj_ptr adj_idx queries starts n_visit max_distance min_chain check")
NearCase = namedtuple("NearCase", "name poses queries radii check")
NearResult = namedtuple("NearResult", "d2 nearest hits")      # per query: distances to all poses, (index, dist_sq), [hits per radius]

up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
MAX_D = 5.0
LIM_PLUS, LIM_MINUS = MAX_D * MAX_D + KT_TOLERANCE, MAX_D * MAX_D - KT_TOLERANCE


def csr(n, edges):
    """Vertex::AddEdge appends to both ends, in insertion order"""
    nbr = [[] for _ in range(n)]
    for a, b in edges:
        nbr[a].append(b)
        nbr[b].append(a)
    ptr = np.zeros(n + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(v) for v in nbr])
    return ptr, np.asarray([w for v in nbr for w in v], dtype=np.int32)


def loop_case(name, xy, edges, queries, max_distance, min_chain, check, starts=None, n_visit=None):
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    ptr, idx = csr(xy.shape[0], edges)
    queries = np.asarray(queries, dtype=np.int32)
    assert queries.size >= 2, "one query alone never reaches the kernel"
    return LoopCase(name, xy, ptr, idx, queries, None if starts is None else np.asarray(starts, dtype=np.int32), n_visit,
                    float(max_distance), int(min_chain), check)


def expect(*want):
    want = [list(w) for w in want]

    def check(chains):
        assert chains == want, (chains, want)
    return check


def pattern(p):
    """-> xy, edges, q for MAX_D: Q at the origin, every l linked to it directly, g / o unlinked at 1 m / 100 m"""
    q = p.index("Q")
    assert p.count("Q") == 1 and set(p) <= set("Qglo")
    xy = np.zeros((len(p), 2))
    edges = []
    for i, c in enumerate(p):
        if c == "g":
            xy[i] = (1.0 + (i % 7) * 0.125, 0.25)
        elif c == "l":
            xy[i] = (0.5, -0.25 * (i % 3))
            edges.append((q, i))
        elif c == "o":
            xy[i] = (100.0 + i, 0.0)
    return xy, edges, q


def pattern_case(name, p, min_chain, want, starts=None, n_visit=None, n_queries=2):
    """the query asked n_queries times over; `want` is what each of them answers (a list per query where the starts differ)"""
    xy, edges, q = pattern(p)
    per_query = want if want and isinstance(want[0], list) else [want] * n_queries
    return loop_case(name, xy, edges, [q] * n_queries, MAX_D, min_chain, expect(*per_query), starts=starts, n_visit=n_visit)


# ---- sizes -------------------------------------------------------------------------------------------------------------------
LOOP_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 513)


def two_laps(n):
    """a robot that drives a circle of 8 m radius twice: scan i and scan i + n / 2 lie next to each other, linked only through
    the odometry chain.  Coordinates are multiples of 1 / 64."""
    t = 4.0 * math.pi * np.arange(n) / max(n, 1)
    r = 8.0 + 0.5 * (np.arange(n) >= n / 2)
    xy = np.round(64.0 * np.stack([r * np.cos(t), r * np.sin(t)], axis=1)) / 64.0
    return xy, [(i, i + 1) for i in range(n - 1)]


def size_cases():
    for n in LOOP_SIZES:
        xy, edges = two_laps(n)
        queries = [n - 1, 0, n // 2, n - 1, (3 * n) // 4]          # n - 1 twice; at n = 1 all five are the same scan

        def check(chains, n=n):
            assert chains[0] == chains[3]
            if n >= 255:
                # the last scan sees the first lap next to it as one long run, far from the end of the list
                assert any(last - first >= 10 and last < n // 2 + 20 for first, last in chains[0])
                assert sum(len(c) for c in chains) >= 4
        yield loop_case(f"sizes: {n} scans, flags row of {(n + 3) // 4 * 4} bytes", xy, edges, queries, 3.0, 3, check)


# ---- thresholds --------------------------------------------------------------------------------------------------------------
def point_with_d2(target, x):
    """(x, y) whose squared distance to the origin, x * x + y * y as the kernels round it, is exactly `target`; None where no y
    gives it"""
    y0 = math.sqrt(target - x * x)
    cands = [y0]
    for _ in range(8):
        cands = [down(cands[0])] + cands + [up(cands[-1])]
    for y in sorted(cands, key=lambda v: abs(v - y0)):
        if x * x + y * y == target:
            return x, y
    return None


def threshold_cases():
    # exactly at max_distance, and adjacent to the query: in range (25 < 25 + 1e-6), not visitable (25 <= 25 - 1e-6 is false), so
    # it is not a linked scan although it is linked directly, and it is a candidate
    yield loop_case("threshold: a neighbour exactly at max_distance is a candidate", [(0, 0), (3, 4), (100, 0)], [(0, 1)], [0, 0], MAX_D, 1,
                    expect([(1, 1)], [(1, 1)]))

    # d2 < max^2 + 1e-6: scan 1 is a chain on one side of the bound only
    for side, target, in_range in (("one ulp below", down(LIM_PLUS), True), ("at", LIM_PLUS, False), ("one ulp above", up(LIM_PLUS), False)):
        pt = point_with_d2(target, 5.0)
        assert pt is not None, side                      # 25 + y * y reaches every double next to the bound

        def check(chains, pt=pt, target=target, in_range=in_range):
            assert squared_distance(pt, (0.0, 0.0)) == target
            assert chains == [[(1, 1)] if in_range else []] * 2
        yield loop_case(f"threshold: d2 {side} max^2 + 1e-6", [(0, 0), pt, (100, 0)], [], [0, 0], MAX_D, 1, check)

    # d2 <= max^2 - 1e-6: scan 1 is linked to the query, scan 2 only to scan 1.  Visitable: both are linked scans, no chain.
    # Not visitable: scan 1 is a candidate and scan 2 is never reached, so it is one too.
    for side, target, visitable in (("one ulp below", down(LIM_MINUS), True), ("at", LIM_MINUS, True), ("one ulp above", up(LIM_MINUS), False)):
        pt = point_with_d2(target, 4.0)
        assert pt is not None, side

        def check(chains, pt=pt, target=target, visitable=visitable):
            assert squared_distance(pt, (0.0, 0.0)) == target
            assert chains == [[] if visitable else [(1, 2)]] * 2
        yield loop_case(f"threshold: d2 {side} max^2 - 1e-6", [(0, 0), pt, (1, 0), (100, 0)], [(0, 1), (1, 2)], [0, 0], MAX_D, 1, check)

    # dx * dx + dy * dy with every operation rounded on its own is below max^2 + 1e-6; with either product kept exact inside a
    # fused multiply-add the sum rounds to the bound itself, which is not in range (found with fractions.Fraction)
    dx, dy = float.fromhex("0x1.80aa84ce72f89p+1"), float.fromhex("0x1.ff7ff108b16e7p+1")

    def check(chains):
        unfused = dx * dx + dy * dy
        fused_x = float(Fraction(dx) * Fraction(dx) + Fraction(dy * dy))        # fma(dx, dx, dy * dy)
        fused_y = float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx))        # fma(dy, dy, dx * dx)
        assert unfused == squared_distance((dx, dy), (0.0, 0.0))
        assert unfused < LIM_PLUS and not fused_x < LIM_PLUS and not fused_y < LIM_PLUS
        assert chains == [[(1, 1)]] * 2                                         # the unfused value decides
    yield loop_case("threshold: fused and unfused d2 on different sides of max^2 + 1e-6", [(0, 0), (dx, dy), (100, 0)], [], [0, 0], MAX_D, 1, check)


# ---- breadth-first traversal -------------------------------------------------------------------------------------------------
def bfs_cases():
    # a hub: 300 neighbours of the query, each with one neighbour of its own: two frontiers wider than a workgroup of 256, and an
    # adjacency row of 300.  A traversal that loses a frontier entry leaves a scan unlinked, which splits off a chain.
    k = 300
    xy = np.zeros((2 * k + 5, 2))
    xy[1:k + 1] = [(1.0 + j / 512.0, 0.5) for j in range(k)]
    xy[k + 1:2 * k + 1] = [(2.0 + j / 512.0, -0.5) for j in range(k)]
    xy[2 * k + 1:2 * k + 4] = (1.0, 1.0)
    xy[2 * k + 4] = (100.0, 0.0)
    edges = [(0, 1 + j) for j in range(k)] + [(1 + j, k + 1 + j) for j in range(k)]
    # (asked from scan 2k + 2, which has no edges, everything in front of it is one run that it ends itself, as a linked scan)
    yield loop_case("bfs: a hub with 300 visitable neighbours, 300 more behind them", xy, edges, [0, 0, 2 * k + 2], MAX_D, 1,
                    expect([(2 * k + 1, 2 * k + 3)], [(2 * k + 1, 2 * k + 3)], [(2 * k + 3, 2 * k + 3)]))

    xy, _, _ = pattern("Qlllggo")
    yield loop_case("bfs: a cycle", xy, [(0, 1), (1, 2), (2, 3), (3, 0)], [0, 2], MAX_D, 1, expect([(4, 5)], [(4, 5)]))
    yield loop_case("bfs: duplicate adjacency entries", xy, [(0, 1), (0, 1), (1, 2), (1, 2), (2, 1), (2, 3)], [0, 0], MAX_D, 1,
                    expect([(4, 5)], [(4, 5)]))
    # scans 4, 5 form a component of their own, in range of the query and visitable, but never reached
    yield loop_case("bfs: two components", xy, [(0, 1), (1, 2), (2, 3), (4, 5)], [0, 4], MAX_D, 1, expect([(4, 5)], []))
    yield loop_case("bfs: the query has no edges", xy, [(1, 2), (2, 3), (4, 5)], [0, 0], MAX_D, 1, expect([(1, 5)], [(1, 5)]))
    yield loop_case("bfs: a store with no edges at all", xy, [], [0, 3, 0], MAX_D, 1, expect([(1, 5)], [(4, 5)], [(1, 5)]))
    # scan 1 sits exactly at max_distance (not visitable, not expanded): scan 2 behind it is visitable but never reached
    yield loop_case("bfs: a visitable scan reachable only through a non-visitable one", [(0, 0), (3, 4), (1, 0), (100, 0)], [(0, 1), (1, 2)],
                    [0, 0], MAX_D, 1, expect([(1, 2)], [(1, 2)]))


# ---- the run rule ------------------------------------------------------------------------------------------------------------
def alternating(n):
    """good / out / good ... with max_distance 0: nothing is visitable (0 <= -1e-6 is false), so the query is a good scan itself"""
    xy = np.zeros((n, 2))
    xy[1::2] = (1.0, 0.0)
    return xy


def run_cases():
    yield pattern_case("run: exactly min_chain, ended by an out-of-range scan", "Qogggol", 3, [(2, 4)])
    yield pattern_case("run: min_chain - 1, ended by an out-of-range scan", "Qoggol", 3, [])
    yield pattern_case("run: min_chain and longer, ended by a linked scan", "Qoggglogggggggloo", 3, [])
    yield pattern_case("run: min_chain - 1, ended by a linked scan", "Qogglo", 3, [])
    yield pattern_case("run: exactly min_chain at the end of the list", "Qoggg", 3, [(2, 4)])
    yield pattern_case("run: min_chain - 1 at the end of the list", "Qogg", 3, [(2, 3)])
    yield pattern_case("run: a short run returned at the end, behind a full one", "Qogggoog", 3, [(2, 4), (7, 7)])
    yield pattern_case("run: starting at scan 0", "gggoQ", 3, [(0, 2)])
    yield pattern_case("run: a single good scan at n - 1", "Qolog", 3, [(4, 4)])
    yield pattern_case("run: every scan linked", "lllQlll", 1, [])
    yield pattern_case("run: min_chain 1", "gQogoggolgo", 1, [(3, 3), (5, 6), (9, 9)])
    yield pattern_case("run: min_chain above n", "gggoQogggoggg", 100, [(10, 12)])
    n = 259
    xy = np.zeros((n, 2))
    xy[:, 0] = (np.arange(n) % 4) / 4096.0                       # d2 below 1e-6: all in range of each other at max_distance 0
    yield loop_case("run: every scan good", xy, [(i, i + 1) for i in range(n - 1)], [0, n - 1, 130], 0.0, 3, expect(*[[(0, n - 1)]] * 3))
    for n in (9, 257):
        def check(chains, n=n):
            assert chains[0] == [(i, i) for i in range(0, n, 2)] and len(chains[0]) == n // 2 + 1       # the slot capacity per query
            assert chains[1] == chains[0] and chains[2] == [(i, i) for i in range(1, n, 2)]
        yield loop_case(f"run: good and out alternating over {n} scans, min_chain 1", alternating(n), [], [0, n - 1, 1], 0.0, 1, check)


# ---- starts ------------------------------------------------------------------------------------------------------------------
RESUME = "ggggoggggolQogggg"              # runs 0-3, 5-8 and 13-16; out-of-range at 4, 9, 12; the query at 11
RUNS = [(0, 3), (5, 8), (13, 16)]


def start_cases():
    n = len(RESUME)
    yield pattern_case("starts: 0", RESUME, 3, RUNS, starts=[0, 0])
    yield pattern_case("starts: None", RESUME, 3, RUNS)
    yield pattern_case("starts: inside a run, min_chain left", RESUME, 3, [(6, 8), (13, 16)], starts=[6, 6])
    yield pattern_case("starts: inside a run, less than min_chain left", RESUME, 3, [(13, 16)], starts=[7, 7])
    yield pattern_case("starts: on a run's last scan", RESUME, 1, [(8, 8), (13, 16)], starts=[8, 8])
    yield pattern_case("starts: on the out-of-range scan that ended a run", RESUME, 3, [(5, 8), (13, 16)], starts=[4, 4])
    yield pattern_case("starts: n_visit - 1", RESUME, 3, [(16, 16)], starts=[n - 1, n - 1])
    yield pattern_case("starts: n_visit", RESUME, 1, [], starts=[n, n])
    yield pattern_case("starts: beyond n", RESUME, 1, [], starts=[1000, 2 ** 31 - 1])
    yield pattern_case("starts: n_visit - 1 and n_visit under a scan limit", RESUME, 1, [[(14, 14)], []], starts=[14, 15], n_visit=15)
    yield pattern_case("starts: different per query", RESUME, 3, [RUNS, [(6, 8), (13, 16)], [], [(5, 8), (13, 16)], [(13, 16)]],
                       starts=[0, 6, n, 4, 9], n_queries=5)


# ---- n_visit -----------------------------------------------------------------------------------------------------------------
def n_visit_cases():
    p = "Qoggggggol"
    for m in (1, 5):
        yield pattern_case(f"n_visit: a run cut at n_visit - 1, min_chain {m}", p, m, [(2, 4)], n_visit=5)
    yield pattern_case("n_visit: equal to n", p, 3, [(2, 7)], n_visit=len(p))
    yield pattern_case("n_visit: 0", "gQggo", 1, [], n_visit=0)
    yield pattern_case("n_visit: 1", "gQggo", 1, [(0, 0)], n_visit=1)
    yield pattern_case("n_visit: the query is scan n_visit", "ogggoQ", 1, [(1, 3)], n_visit=5)
    yield pattern_case("n_visit: the query lies beyond n_visit", "oggggoQ", 1, [(1, 3)], n_visit=4)
    # scan 0 is linked to the query (scan 3) only through scan 4, which the walk does not visit: the traversal still does
    yield loop_case("n_visit: a scan linked through a vertex beyond n_visit", [(1, 0), (1, 0.5), (100, 0), (0, 0), (0.5, 0)], [(3, 4), (4, 0)],
                    [3, 3], MAX_D, 1, expect([(1, 1)], [(1, 1)]), n_visit=3)


# ---- min_chain 0 -------------------------------------------------------------------------------------------------------------
def min_chain_zero_cases():
    """chain.size() >= 0 holds for the empty chain too: the reference returns at the FIRST out-of-range scan with whatever it
    holds and does not advance (Mapper.cpp:2001-2002); the call after it returns the empty chain from the same scan, and
    TryCloseLoop stops.  At most one chain per query, none when scan `start` is out of range."""
    yield pattern_case("min_chain 0: only the first run", RESUME, 0, [(0, 3)])
    yield pattern_case("min_chain 0: the start scan is out of range", RESUME, 0, [], starts=[4, 9])
    yield pattern_case("min_chain 0: started inside a run", RESUME, 0, [[(6, 8)], [(13, 16)]], starts=[6, 13])
    yield pattern_case("min_chain 0: what is left behind a linked scan", "Qggoggg", 0, [(1, 2)])
    yield pattern_case("min_chain 0: a linked scan in front of the first out-of-range one", "gglQoggg", 0, [])
    yield pattern_case("min_chain 0: no out-of-range scan at all", "ggQgg", 0, [(3, 4)])
    yield pattern_case("min_chain 0: cut by a scan limit", "Qggggoggg", 0, [(1, 2)], n_visit=3)
    yield pattern_case("min_chain 0: an out-of-range scan beyond the scan limit", "lQggog", 0, [(2, 3)], n_visit=4)


def loop_cases():
    for gen in (size_cases, threshold_cases, bfs_cases, run_cases, start_cases, n_visit_cases, min_chain_zero_cases):
        yield from gen()


# a store order that goes large -> small -> large, for one handle across the table (scratch left by a bigger store is reused)
def reuse_order(cases):
    by_size = sorted(cases, key=lambda c: -c.ref_xy.shape[0])
    out = []
    while by_size:
        out.append(by_size.pop(0))
        if by_size:
            out.append(by_size.pop())
    return out


# ==== near-by =================================================================================================================
NEAR_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1281)
NEAR_TRIP = 256 * 256                                       # vertices per trip of k_near_by_radius: at most 256 workgroups of 256
INF = float("inf")


def scatter(n, x0=0.0):
    """n distinct points on a 1 / 8 m lattice (distinct up to n = 101 * 89)"""
    i = np.arange(n)
    return np.stack([x0 + ((i * 37) % 101) / 8.0, ((i * 53) % 89) / 8.0], axis=1)


def near_size_cases():
    for n in NEAR_SIZES:
        poses = scatter(n)
        last, first = poses[n - 1], poses[0]
        queries = [last + (1.0 / 64.0, 0.0), last, first + (0.0, -1.0 / 64.0), (1000.0, 1000.0), (6.0, 5.0)]

        def check(res, n=n):
            # the nearest vertex is the LAST one: for n no multiple of 256 the clamped reads past the end return this very point
            # at indices >= n, which must not be reported
            assert res[0].nearest == (n - 1, 1.0 / 4096.0) and res[1].nearest == (n - 1, 0.0)
            assert res[2].nearest == (0, 1.0 / 4096.0)
            assert all(0 <= r.nearest[0] < n for r in res)
            assert [len(h) for h in res[1].hits] == [0, 1, int((res[1].d2 < 4.0).sum()), n]
        yield NearCase(f"near sizes: {n} vertices", poses, np.array(queries), [0.0, 1.0 / 64.0, 4.0, INF], check)


def tie_case(name, n, tied, swap):
    """the vertices `tied` at (3, 4) / (4, 3) in turn around the query (d2 = 25 both ways, the same bits), every other vertex at
    more than 10 m"""
    poses = scatter(n, x0=10.0)
    for k, i in enumerate(tied):
        poses[i] = (3.0, 4.0) if (k % 2 == 0) != swap else (4.0, 3.0)

    def check(res):
        for r in res[:2]:
            assert (r.d2[list(tied)].view(np.uint64) == np.float64(25.0).view(np.uint64)).all() and (np.delete(r.d2, list(tied)) > 25.0).all()
            assert r.nearest == (min(tied), 25.0)
            assert list(r.hits[0]) == [] and list(r.hits[1]) == sorted(tied)         # radius 25 excludes them, the next double holds all
    return NearCase(name, poses, np.array([(0.0, 0.0), (0.0, 0.0), (12.0, 3.0)]), [25.0, up(25.0)], check)


def near_tie_cases():
    pairs = (("two lanes", (5, 6)), ("two waves", (63, 64)), ("two unroll slots", (5, 261)), ("two outer iterations", (5, 1029)),
             ("wave, slot and iteration at once", (70, 390, 1100, 1280)), ("the lowest in a later slot and wave", (500, 1029, 1030, 1279)))
    for what, tied in pairs:
        for swap in (False, True):
            yield tie_case(f"near ties: {what} {tied}{', coordinates swapped' if swap else ''}", 1281, tied, swap)


def near_special_cases():
    poses = scatter(300, x0=1.0)
    poses[7], poses[200] = (0.0, -0.0), (-0.0, 0.0)

    def check(res):
        for r in res:
            assert r.nearest[0] == 7 and r.nearest[1] == 0.0 and not np.signbit(r.nearest[1])       # d2 = +0.0 twice: the lower index
            assert list(r.hits[0]) == [] and list(r.hits[1]) == [] and list(r.hits[2]) == [7, 200]
    yield NearCase("near special: plus and minus zero coordinates, a query on top of two vertices", poses,
                   np.array([(0.0, 0.0), (-0.0, -0.0), (-0.0, 0.0)]), [0.0, -1.0, 5e-324], check)

    big = scatter(300) * 1e198 + 1e200

    def check(res):
        for r in res:
            assert np.isposinf(r.d2).all() and r.nearest == (0, INF)        # every distance overflows: the lowest index
            assert list(r.hits[0]) == [] and list(r.hits[1]) == []          # inf < inf is false
    yield NearCase("near special: every squared distance overflows", big, np.array([(-1e200, -1e200), (-1e200, 1e200)]), [INF, 1e308], check)


def near_radius_cases():
    poses = scatter(700, x0=20.0)
    ring = {650: (3, 4), 3: (-4, 3), 300: (0, -5), 64: (5, 0), 255: (-3, -4), 256: (4, -3)}           # d2 = 25
    inner = {699: (0, 2), 0: (-2, 0), 63: (0, -2), 512: (2, 0)}                                        # d2 = 4
    for i, p in {**ring, **inner, 100: (0.5, 0.0)}.items():
        poses[i] = p

    def check(res):
        r = res[0]
        assert (r.d2[list(ring)] == 25.0).all() and (r.d2[list(inner)] == 4.0).all() and (np.sort(r.d2)[11:] > 25.0).all()
        got = [list(h) for h in r.hits]
        assert got[0] == [100] + sorted(inner)                                        # radius 25: d2 == radius is no hit
        assert got[1] == [100] + sorted(inner) + sorted(ring)                         # one ulp up: all six, by index
        assert got[2] == [100] + sorted(inner) and got[3] == [100] and got[4] == [] and got[5] == []
        assert list(res[1].hits[1]) == [] and res[1].nearest[1] > 25.0
    yield NearCase("near radius: d2 equal to the radius, groups of equal d2, radius 0 and below", poses,
                   np.array([(0.0, 0.0), (-40.0, -40.0)]), [25.0, up(25.0), down(25.0), 4.0, 0.0, -3.0], check)

    for n in (257, 1025):
        poses = scatter(n)

        def check(res, n=n):
            for r in res:
                order = np.lexsort((np.arange(n), r.d2))
                assert list(r.hits[0]) == list(order) and len(r.hits[0]) == n         # every vertex, from every block
                assert (np.sort(r.d2)[1:] == np.sort(r.d2)[:-1]).any()               # with equal distances among them
        yield NearCase(f"near radius: infinite over {n} vertices", poses, np.array([(6.0, 5.0), (0.0, 0.0)]), [INF], check)


CAP_CASE = "near radius: infinite over 257 vertices"      # the GPU side asks it with cap below the number of hits


# ---- stores beyond one trip of k_near_by_radius ------------------------------------------------------------------------------
def lattice(n, x0=0.0):
    """n distinct points on a 1 / 8 m lattice, LATTICE_ROW to a row: vertex i at column i % 512 of row i // 512 (distinct for every n)"""
    i = np.arange(n)
    return np.stack([x0 + (i % LATTICE_ROW) / 8.0, (i // LATTICE_ROW) / 8.0], axis=1)


LATTICE_ROW = 512
TIE_QUERY, TIED = (-50.0, -50.0), (5, NEAR_TRIP + 5)
NEAR_TRIP_SIZES = (NEAR_TRIP - 1, NEAR_TRIP, NEAR_TRIP + 1, NEAR_TRIP + 257, 2 * NEAR_TRIP + 1)
# on which side of vertex 65 536 the hits of radius 0.05 lie (trip one, trip two): around the last vertex, around vertex (100, 128)
# of the lattice, which is vertex 65 636 where the store holds it.  Around vertex (100, 10) they lie in trip one at every size.
SIDES = {NEAR_TRIP - 1: ((True, False), (True, False)), NEAR_TRIP: ((True, False), (True, False)), NEAR_TRIP + 1: ((True, True), (True, False)),
         NEAR_TRIP + 257: ((True, True), (True, True)), 2 * NEAR_TRIP + 1: ((False, True), (True, True))}
ROWS_HELD = {NEAR_TRIP - 1: 1, NEAR_TRIP: 1, NEAR_TRIP + 1: 1, NEAR_TRIP + 257: 2, 2 * NEAR_TRIP + 1: 3}      # of rows 127 .. 129 at columns 99 .. 101


def sides(hits):
    hits = np.asarray(hits)
    return bool((hits < NEAR_TRIP).any()), bool((hits >= NEAR_TRIP).any())


def near_trip_cases():
    """stores around one and two trips of k_near_by_radius' strided loop.  Radius 1 / 128 holds one lattice point, 0.05 the 3 x 3
    points around one (d2 0, 1 / 64, 2 / 64; the next is 4 / 64); the rows of a 3 x 3 block lie 512 vertices apart, so a block on
    rows 127 and 128 has hits on both sides of vertex 65 536."""
    for n in NEAR_TRIP_SIZES:
        poses = lattice(n)
        tied = tuple(i for i in TIED if i < n)
        for k, i in enumerate(tied):
            poses[i] = (TIE_QUERY[0] + (3.0, 4.0)[k], TIE_QUERY[1] + (4.0, 3.0)[k])
        last = poses[n - 1]
        queries = [last + (1.0 / 64.0, 0.0), last, (100 / 8.0, 10 / 8.0), TIE_QUERY, (100 / 8.0, 128 / 8.0)]

        def check(res, n=n, tied=tied):
            # the nearest vertex is the LAST one (the clamped reads past the end return this very point at indices >= n)
            assert res[0].nearest == (n - 1, 1.0 / 4096.0) and res[1].nearest == (n - 1, 0.0)
            assert all(0 <= r.nearest[0] < n for r in res)
            assert list(res[1].hits[0]) == [n - 1] and sides(res[1].hits[0]) == (n <= NEAR_TRIP, n > NEAR_TRIP)
            assert sides(res[1].hits[1]) == SIDES[n][0] and sides(res[4].hits[1]) == SIDES[n][1] and sides(res[2].hits[1]) == (True, False)
            assert len(res[2].hits[1]) == 9 and len(res[4].hits[1]) == 3 * ROWS_HELD[n]
            # equal distances on either side of vertex 65 536: the lower index, in the nearest and in the list
            assert (res[3].d2[list(tied)].view(np.uint64) == np.float64(25.0).view(np.uint64)).all() and (np.delete(res[3].d2, list(tied)) > 25.0).all()
            assert res[3].nearest == (5, 25.0) and list(res[3].hits[2]) == list(tied) and list(res[3].hits[1]) == []
            assert len(tied) == (2 if n > TIED[1] else 1)
            for r in res:                                                             # every vertex, every slot of the hit list used
                assert len(r.hits[3]) == n and np.array_equal(r.hits[3], np.lexsort((np.arange(n), r.d2)))
                assert (np.sort(r.d2)[1:] == np.sort(r.d2)[:-1]).any()
        yield NearCase(f"near trips: {n} vertices", poses, np.array(queries), [1.0 / 128.0, 0.05, up(25.0), INF], check)


TRIP_CAP_CASE = f"near trips: {NEAR_TRIP + 257} vertices"   # ... and this one with caps on either side of the first trip


def near_cases():
    """the stores of more than one trip come last: every test on the shared handle after them, the short-output test on 257
    vertices among them, runs in scratch that a store of 131 073 vertices left"""
    for gen in (near_size_cases, near_tie_cases, near_special_cases, near_radius_cases, near_trip_cases):
        yield from gen()
