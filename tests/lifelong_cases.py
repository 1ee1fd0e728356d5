"""Edge inputs of the node-decay scoring as plain data, independent of the library: what tests/test_edge_cases_oracle.py runs
through oracle/lifelong.py alone (does every case still sit on the decision its name says?) and
tests/test_lifelong_edges_gpu.py through kh_lifelong_scores next to the oracle.

A case is (name, reference, candidates, params, check): `check(kept, iou, area, reading, score)` asserts, on the ORACLE's
results, that the candidates straddle the edge the case is named after (slam_toolbox_lifelong.cpp:199-329, 373-478).
Box sizes are chosen so that the metric under test is exactly representable (IoU 0.25 = a 1 x 1 box inside a 2 x 2 one, 0.5 = a
2 x 1 box inside it), and the parameter is then moved one ulp to either side of it.  Zero-area boxes are left out: the oracle
divides by the area and raises."""
from collections import namedtuple

import numpy as np

from oracle.lifelong import DecayParams, ScanBox, intersect_bounds

Case = namedtuple("Case", "name reference candidates params check")

REF_ID, OLD_ID = 500, 100                      # OLD_ID: far outside the scan buffer, scored by the objective
up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))


def box(centre, size, points=None, uid=OLD_ID, edges=4, score=0.7):
    pts = np.zeros((0, 2)) if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    return ScanBox(barycenter=(float(centre[0]), float(centre[1])), bbox_size=(float(size[0]), float(size[1])), points=pts, unique_id=uid,
                   n_edges=edges, score=score)


def lattice(centre, size, n, fraction_inside=1.0):
    """n points: the first round(fraction * n) on a lattice well inside the box, the rest far outside every box"""
    k = np.arange(n)
    inside = np.stack([centre[0] + size[0] * (((k * 7) % 11) - 5) / 24.0, centre[1] + size[1] * (((k * 5) % 13) - 6) / 28.0], axis=1)
    n_in = int(round(fraction_inside * n))
    inside[n_in:] += 1000.0
    return inside


REF = box((0.0, 0.0), (2.0, 2.0), uid=REF_ID)
QUARTER = dict(centre=(0.0, 0.0), size=(1.0, 1.0))     # IoU with REF = 1 / 4 exactly, area overlap 1
HALF = dict(centre=(0.0, 0.0), size=(2.0, 1.0))        # IoU with REF = 2 / 4 exactly, area overlap 1


def _objective(c_score, overlap, csf, penalty):
    return c_score * (1.0 + csf) - overlap - penalty


def decision_cases():
    # --- iou < iou_thresh
    for name, th, keep in (("one ulp below", down(0.25), True), ("equal to", 0.25, True), ("one ulp above", up(0.25), False)):
        def check(kept, iou, area, reading, score, keep=keep):
            assert iou[0] == 0.25 and iou[1] == 0.5
            assert bool(kept[0]) is keep and kept[1]           # `iou < thresh` drops: equality keeps
            assert bool(score[0] != 0.0) is keep
        cands = [box(**QUARTER, points=lattice((0, 0), (1, 1), 10)), box(**HALF, points=lattice((0, 0), (2, 1), 10))]
        yield Case(f"decision: iou_thresh {name} an IoU of 0.25", REF, cands, DecayParams(iou_thresh=th), check)
    for name, th, keep in (("one ulp below", down(0.5), True), ("equal to", 0.5, True), ("one ulp above", up(0.5), False)):
        def check(kept, iou, area, reading, score, keep=keep):
            assert iou[0] == 0.5 and bool(kept[0]) is keep
        yield Case(f"decision: iou_thresh {name} an IoU of 0.5", REF, [box(HALF["centre"], HALF["size"], lattice((0, 0), (2, 1), 10))],
                   DecayParams(iou_thresh=th), check)

    # --- edges < 2
    def check(kept, iou, area, reading, score):
        assert list(kept) == [False, False, True, True] and score[0] == 0.0 and score[1] == 0.0 and score[2] != 0.0
    yield Case("decision: 0, 1, 2 and 3 edges", REF, [box(**HALF, points=lattice((0, 0), (2, 1), 5), edges=e) for e in (0, 1, 2, 3)], DecayParams(), check)

    # --- ref.id - c.id < scan_buffer_size, and the two lynch-pins
    ids = [REF_ID - 9, REF_ID - 10, REF_ID - 11, REF_ID + 100, REF_ID, 0, 1, 2]

    def check(kept, iou, area, reading, score):
        assert kept.all()
        own = [s == 0.7 for s in score]
        assert own == [True, False, False, True, True, True, True, False]     # 9 back keeps its score, 10 back is scored
    yield Case("decision: age against a scan buffer of 10", REF, [box(**HALF, points=lattice((0, 0), (2, 1), 6), uid=i) for i in ids], DecayParams(scan_buffer_size=10), check)

    def check(kept, iou, area, reading, score):
        assert kept.all() and [s == 0.7 for s in score] == [True, True, True, True, True, True, True, True]
    yield Case("decision: everything inside a scan buffer of 1000", REF, [box(**HALF, points=lattice((0, 0), (2, 1), 6), uid=i) for i in ids],
               DecayParams(scan_buffer_size=1000), check)

    def check(kept, iou, area, reading, score):
        assert kept.all() and [s == 0.7 for s in score] == [False, False, False, True, False, True, True, False]   # 0 < 0 is false: the scan itself is scored
    yield Case("decision: a scan buffer of 0", REF, [box(**HALF, points=lattice((0, 0), (2, 1), 6), uid=i) for i in ids], DecayParams(scan_buffer_size=0), check)

    # --- iou > iou_match && edges < 3
    def check(kept, iou, area, reading, score):
        assert iou[0] == 1.0 and iou[1] == 1.0 and iou[2] == 0.5 and iou[3] == 0.5 and kept.all()
        assert score[0] == -1.0 and score[1] != -1.0            # the same box with 2 and with 3 edges
        assert score[2] != -1.0 and score[3] != -1.0            # IoU EQUAL to iou_match is not a match
    cands = [box((0, 0), (2, 2), lattice((0, 0), (2, 2), 9), edges=2), box((0, 0), (2, 2), lattice((0, 0), (2, 2), 9), edges=3),
             box(**HALF, points=lattice((0, 0), (2, 1), 9), edges=2), box(**HALF, points=lattice((0, 0), (2, 1), 9), edges=3)]
    yield Case("decision: iou_match 0.5 against IoU 1 and 0.5, 2 and 3 edges", REF, cands, DecayParams(iou_match=0.5), check)

    def check(kept, iou, area, reading, score):
        assert score[2] == -1.0 and score[3] != -1.0
    yield Case("decision: iou_match one ulp below an IoU of 0.5", REF, cands, DecayParams(iou_match=down(0.5)), check)

    # --- the three clamps of the constraint factor
    # area overlap 1 (nested); 4 of 10 readings inside -> reading 0.4; overlap = overlap_scale * 0.4
    def cand(edges, score=0.7, frac=0.4):
        return box(**HALF, points=lattice((0, 0), (2, 1), 10, frac), edges=edges, score=score)

    def check(kept, iou, area, reading, score):
        assert list(kept) == [False, True, True, True, True]    # a negative factor (edges < 2) is never scored
        ov = 0.5 * 0.4
        assert reading[1] == 0.4 and area[1] == 1.0
        assert score[1] == _objective(0.7, ov, 0.0, 0.001)                   # edges 2: factor 0
        assert score[2] == _objective(0.7, ov, 0.05 * 1, 0.001)              # edges 3: in (0, 1) and below the overlap
        assert 0.05 * 10 > ov and score[3] == _objective(0.7, ov, ov, 0.001)  # edges 12: above the overlap -> the overlap
        assert 0.05 * 38 > 1.0 and score[4] == _objective(0.7, ov, ov, 0.001)  # edges 40: above 1, then above the overlap
    yield Case("decision: constraint factor below 0, 0, in (0, 1), above the overlap, above 1", REF, [cand(e) for e in (1, 2, 3, 12, 40)], DecayParams(), check)

    def check(kept, iou, area, reading, score):
        ov = 3.0 * 1.0
        assert reading[0] == 1.0 and area[0] == 1.0
        assert score[0] == 1.0 and _objective(0.7 * 4, ov, 1.0, 0.001) > 1.0        # factor clamps to 1 (below the overlap of 3), score clamps to 1
        assert score[1] == _objective(0.7, ov, 1.0, 0.001) and score[1] < 0.0
        assert score[2] == _objective(0.7, ov, 0.05 * 18, 0.001)                    # 0.9: the clamp to 1 does not bite
        assert score[3] == _objective(0.7, ov, 1.0, 0.001)                          # 0.05 * 20 = 1.0 exactly
    yield Case("decision: constraint factor clamps to 1 under an overlap of 3", REF,
               [cand(40, 2.8, 1.0), cand(40, 0.7, 1.0), cand(20, 0.7, 1.0), cand(22, 0.7, 1.0)], DecayParams(overlap_scale=3.0), check)

    # --- std::min(area, reading): either side
    def check(kept, iou, area, reading, score):
        assert reading[0] < area[0] and area[1] < reading[1] and area[2] == reading[2] == 0.5
        for k in range(3):
            ov = 0.5 * min(area[k], reading[k])
            assert score[k] == _objective(0.7, ov, min(0.05 * 2, ov), 0.001)
    half_out = dict(centre=(1.0, 0.0), size=(2.0, 2.0))                   # half of it inside REF: area overlap 0.5, IoU 1 / 3
    yield Case("decision: reading overlap below, above and equal to the area overlap", REF,
               [box(**half_out, points=lattice((0.5, 0), (1, 2), 10, 0.2)), box(**half_out, points=lattice((0.5, 0), (1, 2), 10, 0.9)),
                box(**half_out, points=lattice((0.5, 0), (1, 2), 10, 0.5))], DecayParams(), check)

    # --- score > 1
    def check(kept, iou, area, reading, score):
        assert reading[0] == 0.0 and list(score) == [1.0, 1.0, down(1.0), 1.0]
    outside = lattice((0, 0), (1, 1), 4, 0.0)
    yield Case("decision: a score one ulp above 1, at 1, one ulp below, and far above", REF,
               [box(**HALF, points=outside, score=s) for s in (up(1.0), 1.0, down(1.0), 17.0)], DecayParams(nearby_penalty=0.0), check)


def on_bounds_points(reference, centre, size):
    """the four bounds of the intersection by the oracle's own expression, one point ON each (strict test: not counted) and one
    an ulp inside (counted), the other coordinate mid-way"""
    x_l, x_u, y_l, y_u = intersect_bounds(reference, box(centre, size))
    mx, my = (x_l + x_u) / 2.0, (y_l + y_u) / 2.0
    on = [(x_l, my), (x_u, my), (mx, y_l), (mx, y_u), (x_l, y_l), (x_u, y_u)]
    inside = [(up(x_l), my), (down(x_u), my), (mx, up(y_l)), (mx, down(y_u)), (up(x_l), up(y_l)), (down(x_u), down(y_u))]
    return np.array(on), np.array(inside)


def geometry_cases():
    p = DecayParams(iou_thresh=0.0)                  # nothing is dropped for its IoU (`iou < 0.0` is false, for -0.0 too)
    ref = box((0.1, -0.3), (0.7, 1.3), uid=REF_ID)

    def check(kept, iou, area, reading, score):
        assert iou[0] == 1.0 and area[0] == 1.0                                     # identical
        assert 0.0 < iou[1] < 1.0 and area[1] == 1.0                                # candidate nested in the reference
        assert 0.0 < iou[2] < 1.0 and 0.0 < area[2] < 1.0                           # reference nested in the candidate
        assert iou[3] == 0.0 and iou[4] == 0.0                                      # touching: zero extent
        assert iou[5] == 0.0 and iou[6] == 0.0                                      # disjoint in one axis only: negative product -> 0
        # disjoint in BOTH: the two negative extents multiply to a positive "intersection" (upstream's behaviour, which parity
        # has to reproduce): a small one gives IoU > 0, a large one exceeds both areas and turns the union, hence the IoU, negative
        assert iou[7] > 0.0 and area[7] > 0.0
        assert iou[8] < 0.0 and area[8] > 1.0
        assert kept[:8].all() and not kept[8]
    r = box((0.0, 0.0), (2.0, 2.0), uid=REF_ID)
    pts = lattice((0, 0), (0.5, 0.5), 7)
    cands = [box((0, 0), (2, 2), pts), box((0.25, -0.25), (1, 0.5), pts), box((0.5, 0.5), (8, 6), pts),
             box((2.0, 0.0), (2, 2), pts), box((0.0, -1.5), (1, 1), pts),           # touching at x = 1 and at y = -1
             box((5.0, 0.5), (2, 2), pts), box((0.5, 7.0), (1, 3), pts),            # disjoint in x only / in y only
             box((2.25, 2.5), (2, 2), pts), box((5.0, 7.0), (2, 3), pts)]           # diagonal, near and far: both extents negative
    yield Case("geometry: identical, nested, touching, disjoint in one axis, disjoint in both", r, cands, p, check)

    def check(kept, iou, area, reading, score):
        assert reading[0] == 0.0 and reading[1] == 1.0 and reading[2] == 0.5 and reading[3] == 0.5
    centre, size = (0.37, 0.21), (0.9, 0.6)          # overlaps ref partly: two bounds from each box, none of them exact in binary
    on, inside = on_bounds_points(ref, centre, size)
    both = np.concatenate([on, inside])
    yield Case("geometry: readings on the four bounds and one ulp inside", ref,
               [box(centre, size, on), box(centre, size, inside), box(centre, size, both), box(centre, size, both[::-1])], p, check)

    def check(kept, iou, area, reading, score):
        # a corner touching with the other extent NEGATIVE gives 0 * negative = -0.0, which `v < 0` lets through
        assert iou[0] == 0.0 and np.signbit(iou[0]) and not np.signbit(iou[1])
    yield Case("geometry: minus zero intersection", r, [box((2.0, 5.0), (2, 2), pts), box((2.0, 0.5), (2, 2), pts)], p, check)


def bulk(n, point_counts, salt=0, ref=None):
    """n candidates scattered over and around the reference, ages / edges / scores cycling through every branch; candidate k has
    point_counts[k % len] readings, a deterministic share of them inside its box"""
    ref = ref or box((3.0, -2.0), (9.0, 7.0), uid=REF_ID + salt)
    out = []
    for k in range(n):
        j = k + 13 * salt
        centre = (ref.barycenter[0] + ((j * 29) % 23 - 11) * 0.61, ref.barycenter[1] + ((j * 17) % 19 - 9) * 0.53)
        size = (2.0 + (j % 9) * 1.3, 1.5 + (j % 7) * 1.7)
        npts = int(point_counts[k % len(point_counts)])
        i = np.arange(npts)
        pts = np.stack([centre[0] + size[0] * (((i * 31 + j) % 97) - 48) / 90.0, centre[1] + size[1] * (((i * 57 + 3 * j) % 89) - 44) / 80.0], axis=1)
        uid = (0, 1, ref.unique_id - 3, ref.unique_id - 10, ref.unique_id + 5)[j % 11] if j % 11 < 5 else 20 + j % 300
        out.append(box(centre, size, pts, uid=uid, edges=(j * 3) % 8, score=0.05 + ((j * 7) % 40) / 40.0))
    return ref, out


CANDIDATE_COUNTS = (0, 1, 3, 4, 5, 64, 1000)
POINT_COUNTS = (0, 1, 63, 64, 65, 128, 4097, 20000)


def launch_cases():
    for n in CANDIDATE_COUNTS:
        ref, cands = bulk(n, (5, 0, 64, 1, 130, 63, 65), salt=n)
        yield Case(f"launch: {n} candidates", ref, cands, DecayParams(), None)
    ref, cands = bulk(2 * len(POINT_COUNTS) + 1, POINT_COUNTS[::-1], salt=3)
    for c in cands:
        c.n_edges, c.unique_id = max(c.n_edges, 2), OLD_ID

    def check(kept, iou, area, reading, score):
        assert sorted({c.points.shape[0] for c in cands}) == sorted(POINT_COUNTS)
        assert int(np.isnan(reading).sum()) == sum(c.points.shape[0] == 0 for c in cands) > 0
        assert np.nanmax(reading) > 0.0
    yield Case(f"launch: {POINT_COUNTS} readings within one call", ref, cands, DecayParams(iou_thresh=0.0), check)


def call_sizes(n_calls, seed):
    """1 -> 1000 -> 2 -> 500 ..., then seeded sizes: the scratch blocks grow, are reused by smaller calls, and grow again"""
    rng = np.random.default_rng(seed)
    head = [1, 1000, 2, 500, 3, 1200, 4, 5, 64, 65]
    return (head + [int(v) for v in rng.integers(1, 400, n_calls)])[:n_calls]


RESIDENT_N_SCAN = (64, 65, 1081)              # one full mask word; one reading in a second word; 17 words, the last one partial


def resident_slots(m, n_scan):
    """which of the n_scan readings of a scan carry the m filtered ones: spread evenly, the first and the last slot included"""
    if m == 1:
        return np.array([n_scan - 1])
    return np.unique(np.round(np.linspace(0, n_scan - 1, m)).astype(np.int64))


def to_resident(case, n_scan):
    """the candidates of a case as the mapper holds them: n_scan UNFILTERED readings per candidate and one flag per reading.  The
    candidate's own readings go, in order, to resident_slots with the flag set; every other slot holds a decoy in the middle of
    the intersection with the flag cleared -- a kernel that ignores a mask bit counts it.  -> (readings, passed), or None when a
    candidate has more readings than n_scan."""
    readings, passed = [], []
    for c in case.candidates:
        m = c.points.shape[0]
        if m > n_scan:
            return None
        x_l, x_u, y_l, y_u = intersect_bounds(case.reference, c)
        r = np.tile(np.array([(x_l + x_u) / 2.0, (y_l + y_u) / 2.0]), (n_scan, 1))
        flag = np.zeros(n_scan, dtype=bool)
        if m:
            slots = resident_slots(m, n_scan)
            r[slots] = c.points
            flag[slots] = True
        readings.append(r)
        passed.append(flag)
    return readings, passed


def resident_cases():
    """(case, n_scan, readings, passed) for every case and scan length it fits"""
    for case in all_cases():
        for n_scan in RESIDENT_N_SCAN:
            res = to_resident(case, n_scan)
            if res is not None and case.candidates:
                yield case, n_scan, res[0], res[1]


def all_cases():
    for gen in (decision_cases, geometry_cases, launch_cases):
        yield from gen()
