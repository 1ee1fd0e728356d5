"""Edge inputs for the relocalization enumeration (k_seed_cover, k_prefix_list, k_base_gather in csrc/graph.hip), and the small map the
end-to-end tests share.  tests/test_relocalize_rule_oracle.py checks on the CPU that every case sits on the edge its name says
(Case.check, fed with tests/relocalize_rule.py's answer); tests/test_relocalize_edges_gpu.py asks the library for the same cases and
compares seed lists, base_begin and base_idx exactly.  Non-finite poses are out, as for the near-by kernels."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import relocalize_rule as rr

Case = namedtuple("Case", "name poses spacing max_distance max_base center radius check")
SPACING, MAX_D = 1.5, 3.0


def _case(name, poses, check, spacing=SPACING, max_distance=MAX_D, max_base=40, center=None, radius=0.0):
    return Case(name, np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 2), spacing, max_distance, max_base, center, radius, check)


def edge_of(limit):
    """the largest x with x * x < limit, and the next double (x * x >= limit)"""
    x = math.sqrt(limit)
    while x * x >= limit:
        x = math.nextafter(x, 0.0)
    while math.nextafter(x, math.inf) ** 2 < limit:
        x = math.nextafter(x, math.inf)
    return x, math.nextafter(x, math.inf)


def cases():
    out = []

    def sizes(n_seeds, n_base):
        def check(s, begin, idx):
            assert s.size == n_seeds and begin.size == n_seeds + 1 and begin[-1] == idx.size == n_base
        return check
    out.append(_case("empty store", np.zeros((0, 2)), sizes(0, 0)))
    out.append(_case("one vertex", [[0.25, -0.75]], sizes(1, 1)))
    rng = np.random.default_rng(5)
    one_cell = rng.uniform(0.0, 1.0, size=(300, 2))
    out.append(_case("all vertices in one cell", one_cell, sizes(1, 38), spacing=1000.0))       # 300 in range: stride 8, 38 kept
    gx, gy = np.meshgrid(np.arange(-8, 9) * SPACING + 0.5, np.arange(-7, 8) * SPACING + 0.25)
    lattice = np.stack([gx.ravel(), gy.ravel()], axis=1)

    def every_vertex(s, begin, idx):
        assert np.array_equal(s, np.arange(lattice.shape[0])) and (np.diff(begin) > 1).all()
    out.append(_case("one vertex per cell", lattice, every_vertex))
    # cell edges and corners on both signs: k * spacing is exact, so x / spacing = k; the double below it falls into cell k - 1
    ks = [-2.0, -1.0, 0.0, 1.0, 2.0]
    pts = []
    for kx in ks:
        for ky in ks:
            x, y = kx * SPACING, ky * SPACING
            pts += [(x, y), (math.nextafter(x, -math.inf), y), (x, math.nextafter(y, -math.inf)), (math.nextafter(x, -math.inf), math.nextafter(y, -math.inf))]
    pts += [(-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (5e-324, -5e-324)]
    edges = np.asarray(pts)

    def on_edges(s, begin, idx):
        # 6 x 6 cells (-3 .. 2 on both axes), one seed each; of the signed zeros none is a seed (cell (0, 0) has its seed at the corner
        # (0, 0) above), and the denormal pair (+, -) shares cell (0, -1) with the point below the corner
        assert s.size == 36 and not np.isin(np.arange(edges.shape[0] - 4, edges.shape[0]), s).any()
        c = rr.cells(edges, SPACING)
        assert c[-4:, :].tolist() == [[-0.0, -0.0], [0.0, -0.0], [-0.0, 0.0], [0.0, -1.0]] and c.min() == -3.0 and c.max() == 2.0
    out.append(_case("vertices on cell edges and corners, both signs", edges, on_edges))
    for n in (257, 513):
        cloud = np.random.default_rng(n).uniform(-12.0, 12.0, size=(n, 2))

        def ragged(s, begin, idx, n=n):
            assert 100 < s.size < n and np.diff(begin).max() == 7 and np.diff(begin).min() >= 1
        out.append(_case(f"{n} vertices: more than one workgroup, a ragged last wave", cloud, ragged, max_base=7))
    # a base exactly at R * R + KT_TOLERANCE: the last double inside and the first outside, on both axes and both signs
    lo, hi = edge_of(MAX_D * MAX_D + rr.KT_TOLERANCE)
    ring = np.asarray([(0.0, 0.0), (lo, 0.0), (hi, 0.0), (-lo, 0.0), (-hi, 0.0), (0.0, lo), (0.0, hi), (0.0, -lo), (0.0, -hi)])

    def tolerance(s, begin, idx):
        assert s[0] == 0 and idx[begin[0]:begin[1]].tolist() == [0, 1, 3, 5, 7]
        assert lo * lo < MAX_D * MAX_D + rr.KT_TOLERANCE <= hi * hi and lo > MAX_D
    out.append(_case("base at the KT_TOLERANCE boundary, inside and outside", ring, tolerance))
    # the stride rule at c = max_base, max_base + 1 and 2 * max_base + 1 (max_base 5), three clusters far apart, one cell each
    mb = 5
    cluster = lambda n, x0: np.stack([x0 + 0.01 * np.arange(n), np.full(n, 0.5)], axis=1)
    stride = np.concatenate([cluster(mb, 0.1), cluster(mb + 1, 30.1), cluster(2 * mb + 1, 60.1)])

    def strides(s, begin, idx):
        assert s.tolist() == [0, mb, 2 * mb + 1]
        assert [idx[begin[k]:begin[k + 1]].tolist() for k in range(3)] == [[0, 1, 2, 3, 4], [5, 7, 9], [11, 14, 17, 20]]
    out.append(_case("counts at the three stride boundaries", stride, strides, max_base=mb))
    # subsampling drops the seed from its own base: the seed of the second cell is entry 1 of a list of 6 (max_base 5: stride 2)
    drop = np.asarray([(1.4, 0.5), (1.6, 0.5), (1.45, 0.5), (1.65, 0.5), (1.7, 0.5), (1.75, 0.5)])

    def dropped(s, begin, idx):
        assert s.tolist() == [0, 1] and idx.tolist() == [0, 2, 4, 0, 2, 4]
    out.append(_case("the stride drops the seed from its own base", drop, dropped, max_base=mb))
    # regions: one that keeps no seed; one whose boundary runs between two seeds a double apart in squared distance
    out.append(_case("a region that keeps no seed", lattice, sizes(0, 0), center=(500.0, 500.0), radius=1.0))
    rlo, rhi = edge_of(2.0 * 2.0 + rr.KT_TOLERANCE)

    def region(s, begin, idx):
        assert s.tolist() == [0, 2, 4], "five seeds, the two a double outside the region dropped"
    out.append(_case("a region boundary at radius * radius + KT_TOLERANCE", [(rlo, 0.0), (0.0, rhi), (0.0, 0.0), (-rhi, 0.0), (0.0, -rlo)], region,
                     center=(0.0, 0.0), radius=2.0))
    return out


# ---- the small map of the end-to-end tests -------------------------------------------------------------------------------------------
# Nine consecutive nodes of the warehouse trajectory (aisle x = 2.5, y = 3.0 .. 7.0, half a metre apart, heading pi / 2) without node
# HELD_OUT; the query is a scan taken AT the held-out node's position with the robot turned by TURN from the trajectory's heading --
# more than one coarse window (2 * 0.349 rad) from the heading of every scan of the map.  World / scan-noise seeds tried with the rule
# alone (tests/test_relocalize_rule_oracle.py): (12345, 1), (12345, 2) and (7, 1) all put the best hypothesis in the held-out pose's
# neighbouring cell, one centimetre or less from the truth; (12345, 2) is kept because one of its hypotheses passes the coarse gate
# and fails the acceptance, so the two are told apart.
WORLD_SEED, SCAN_SEED, N_NODES, HELD_OUT = 12345, 2, 9, 5
TURN = math.pi / 4 + 0.1
N_HEADINGS = 8                          # 3 seeds x 8 headings = 24 hypotheses; the scan's heading lies 0.1 rad from heading 7
MAPPER_PARAMS = dict(loop_search_space_dimension=4.0, loop_search_space_resolution=0.05, loop_search_space_smear_deviation=0.03)
SmallMap = namedtuple("SmallMap", "nodes poses ranges true_pose query")
_small_map = None


def small_map():
    global _small_map
    if _small_map is None:
        from slam_toolbox_amd import synth
        world = synth.make_world(WORLD_SEED)
        truth, _ = synth.trajectory(N_NODES + 1)
        rng = np.random.default_rng(SCAN_SEED)
        ranges = [synth.make_scan(world, truth[i], rng) for i in range(N_NODES)]
        nodes = [i for i in range(N_NODES) if i != HELD_OUT]
        true_pose = truth[HELD_OUT].copy()
        true_pose[2] += TURN
        query = synth.make_scan(world, true_pose, rng)
        _small_map = SmallMap(nodes, truth[nodes].copy(), [ranges[i] for i in nodes], true_pose, query)
    return _small_map


_rule_result = {}


GATES = (0.35, 3.0 * 3.0, 0.45)         # loop_match_minimum_response_coarse, _maximum_variance_coarse (as stored: squared), _minimum_response_fine
OPEN_GATES = (-1.0, 1e30, -1.0)         # every hypothesis passes and is accepted: all 24 come back with both matches


def rule_on_small_map(poses=None, center=None, radius=0.0, gates=GATES, threads=8):
    """the rule's answer on the small map (computed once per distinct argument set, shared by the tests of a process)"""
    from common import LASER, OFFLINE_PARAMS
    from oracle import karto
    sm = small_map()
    poses = sm.poses if poses is None else np.asarray(poses)
    key = (poses.tobytes(), center, radius, gates)
    if key not in _rule_result:
        scans = [karto.Scan(r, p, LASER) for r, p in zip(sm.ranges, poses)]
        coarse = karto.Matcher(4.0, 0.05, 0.03, LASER.range_threshold, OFFLINE_PARAMS, threads=threads)
        fine = karto.Matcher(0.5, 0.01, 0.1, LASER.range_threshold, OFFLINE_PARAMS, threads=threads)
        _rule_result[key] = rr.relocalize(poses[:, :2], scans, sm.query, LASER, coarse, fine, gates[0], gates[1], gates[2], SPACING, MAX_D, N_HEADINGS,
                                          center_xy=center, radius=radius)
    return _rule_result[key]
