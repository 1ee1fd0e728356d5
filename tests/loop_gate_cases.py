"""Inputs of the gated loop-candidate enumeration (kh_graph_find_loop_candidates_gated, k_loop_candidates<gated>, csrc/graph.hip) as
plain data, independent of the library: tests/test_loop_gate_rule_oracle.py runs them through tests/loop_gate_rule.py alone (does
every case still show what its name says?), tests/test_loop_gate_gpu.py through the kernel (the batch) and the host route (each
query alone) next to the rule.

A case is (name, ref_xy, adj_ptr, adj_idx, queries, starts | None, n_visit | None, max_distance, min_chain, chi2, gate, check):
gate is (n_queries, n_scans, 3, 3), `check(chains, case)` asserts on the RULE's chains.  Every batch holds at least two queries."""
import math
from collections import namedtuple

import numpy as np

import graph_cases as gc
import loop_gate_rule as rule
from oracle import loops

GateCase = namedtuple("GateCase", "name ref_xy adj_ptr adj_idx queries starts n_visit max_distance min_chain chi2 gate check")


def gate_case(name, xy, edges, queries, max_distance, min_chain, chi2, gate, check, starts=None, n_visit=None):
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    ptr, idx = gc.csr(xy.shape[0], edges)
    queries = np.asarray(queries, dtype=np.int32)
    assert queries.size >= 2, "one query alone never reaches the kernel"
    gate = np.ascontiguousarray(gate, dtype=np.float64).reshape(queries.size, xy.shape[0], 3, 3)
    return GateCase(name, xy, ptr, idx, queries, None if starts is None else np.asarray(starts, dtype=np.int32), n_visit, float(max_distance),
                    int(min_chain), float(chi2), gate, check)


def rule_chains(case, gate=None, chi2=None):
    starts = case.starts if case.starts is not None else [0] * len(case.queries)
    gate = case.gate if gate is None else gate
    return [rule.find_loop_candidates(int(q), case.ref_xy, case.adj_ptr, case.adj_idx, case.max_distance, case.min_chain,
                                      case.chi2 if chi2 is None else chi2, gate[k], start=int(s), n_visit=case.n_visit)
            for k, (q, s) in enumerate(zip(case.queries, starts))]


def plain_chains(case):
    starts = case.starts if case.starts is not None else [0] * len(case.queries)
    return [loops.find_possible_loop_closures(int(q), case.ref_xy, case.adj_ptr, case.adj_idx, case.max_distance, case.min_chain, start=int(s),
                                              n_visit=case.n_visit) for q, s in zip(case.queries, starts)]


def random_rows(rng, n_queries, n, scale):
    """covariances L L^T whose position block reaches `scale` m^2"""
    L = np.tril(rng.uniform(-1.0, 1.0, size=(n_queries, n, 3, 3))) * math.sqrt(scale)
    return L @ np.swapaxes(L, -1, -2)


def differs_from_plain(chains, case):
    assert chains != plain_chains(case), "the gate changes nothing here"
    assert sum(len(c) for c in chains) >= 1


def expect(*want):
    want = [list(w) for w in want]

    def check(chains, case):
        assert chains == want, (chains, want)
    return check


def cases():
    rng = np.random.default_rng(20)
    # one scan: the query is its own linked scan, no chain
    yield gate_case("n = 1", [(0.0, 0.0)], [], [0, 0], 3.0, 1, 5.991, random_rows(rng, 2, 1, 2.0), expect([], []))

    # the sizes around one block of 256 threads (and a flags row that is / is not a multiple of four bytes)
    for n in (255, 256, 257):
        xy, edges = gc.two_laps(n)
        queries = [n - 1, 0, n // 2, (3 * n) // 4]
        yield gate_case(f"sizes: {n} scans", xy, edges, queries, 3.0, 3, 5.991, random_rows(rng, len(queries), n, 1.5), differs_from_plain)

    # one query asked three times with three different rows: none, moderate, large
    n = 96
    xy, edges = gc.two_laps(n)
    gate = np.zeros((3, n, 3, 3))
    gate[1] = np.diag([0.5, 0.5, 0.01])
    gate[2] = np.diag([6.0, 6.0, 0.01])

    def three(chains, case):
        assert chains[0] == plain_chains(case)[0]
        assert chains[0] != chains[1] and chains[1] != chains[2] and chains[0] != chains[2], chains
    yield gate_case("three queries with different rows in one call", xy, edges, [n - 1] * 3, 3.0, 3, 5.991, gate, three)

    # start inside a run: the chain counts from there
    n = 128
    xy, edges = gc.two_laps(n)
    gate = np.broadcast_to(np.diag([1.0, 0.25, 0.01]), (2, n, 3, 3)).copy()
    whole = rule.find_loop_candidates(n - 1, xy, *gc.csr(n, edges), 3.0, 3, 5.991, gate[0])
    first, last = max(whole, key=lambda c: c[1] - c[0])
    assert last - first >= 6

    def inside(chains, case, first=first, last=last):
        assert (first + 2, last) in chains[0] and (first, last) in chains[1]
    yield gate_case("start inside a run", xy, edges, [n - 1, n - 1], 3.0, 3, 5.991, gate, inside, starts=[first + 2, 0])

    # n_visit < n: the walk stops there, the breadth-first walk does not
    n = 128
    xy, edges = gc.two_laps(n)
    gate = random_rows(rng, 2, n, 1.0)

    def short(chains, case):
        assert all(b < case.n_visit for c in chains for _, b in c) and sum(len(c) for c in chains) >= 1
        assert chains != rule_chains(case._replace(n_visit=None))
    yield gate_case("n_visit < n", xy, edges, [n - 1, n - 2], 3.0, 3, 5.991, gate, short, n_visit=64)

    # min_chain 0: at most one chain per query, the walk ends at the first out-of-range scan
    xy, edges = gc.two_laps(128)

    def at_most_one(chains, case):
        assert all(len(c) <= 1 for c in chains)
        assert chains != rule_chains(case._replace(min_chain=3))
    yield gate_case("min_chain = 0", xy, edges, [127, 64], 3.0, 0, 5.991, random_rows(rng, 2, 128, 1.0), at_most_one)

    # an ellipse at 30 degrees: semi-axes sqrt(4 + 4 * 9) = 6.32 m along it and 2 m across.  Scans at 5 m on the major axis, on the
    # minor axis and on the x and y axes, each followed by a scan far away
    cs, sn = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    R = np.array([[cs, -sn], [sn, cs]])
    D = np.zeros((3, 3))
    D[:2, :2] = R @ np.diag([9.0, 0.0]) @ R.T
    far = (100.0, 100.0)
    xy = [(0.0, 0.0), far, (5.0 * cs, 5.0 * sn), far, (-5.0 * sn, 5.0 * cs), far, (5.0, 0.0), far, (0.0, 5.0), far, (-5.0 * cs, -5.0 * sn), far]
    gate = np.broadcast_to(D, (2, len(xy), 3, 3)).copy()
    gate[1] = 0.0
    yield gate_case("an ellipse at 30 degrees, scans on both axes", xy, [], [0, 0], 2.0, 1, 4.0, gate, expect([(2, 2), (10, 10)], []))

    # r = 2, chi2 = 4, Dxx = 3: a scan at (4, 0) has q = 16 / 4 = 4.0 exactly -- a candidate (4 < 4 + 1e-6), not visitable
    # (4 <= 4 - 1e-6 is false), so the edge to the query does not make it a linked scan; (4.000001, 0) and (0, 2.000001) are out
    D = np.diag([3.0, 0.0, 0.0])
    xy = [(0.0, 0.0), (4.0, 0.0), (4.000001, 0.0), (0.0, 2.000001), far]

    def boundary(chains, case):
        assert rule.gated_sq(4.0, 0.0, 1.0, 3.0, 0.0, 0.0) == 4.0
        assert rule.gated_sq(4.000001, 0.0, 1.0, 3.0, 0.0, 0.0) >= 4.0 + 1e-6 and rule.gated_sq(0.0, 2.000001, 1.0, 3.0, 0.0, 0.0) >= 4.0 + 1e-6
        assert chains == [[(1, 1)], [(1, 1)]], chains
    yield gate_case("the exact boundary: q = r * r", xy, [(0, 1)], [0, 0], 2.0, 1, 4.0, np.broadcast_to(D, (2, 5, 3, 3)), boundary)

    # rows that are no covariance: the plain test applies to that scan.  Each bad row sits on a scan at 4 m (out of the plain 3 m
    # disk; a row of +50 m^2 like its neighbours' would let it in) and on a scan at 2 m (in)
    bad = {"negative diagonal": np.diag([-0.5, 50.0, 0.0]), "NaN entry": np.array([[50.0, np.nan, 0], [np.nan, 50.0, 0], [0, 0, 0]]),
           "infinite entry": np.diag([np.inf, 50.0, 0.0]), "det <= 0": np.array([[1.0, 5.0, 0], [5.0, 1.0, 0], [0, 0, 0]]),
           "negative yy": np.diag([50.0, -1e-3, 0.0]), "NaN yy": np.diag([50.0, np.nan, 0.0])}
    xy, rows = [(0.0, 0.0), far], [np.zeros((3, 3)), np.zeros((3, 3))]
    for k, row in enumerate(bad.values()):
        xy += [(4.0, 0.125 * k), far, (0.0, 2.0 + 0.125 * k), far, (4.0, -0.125 * k - 0.125), far]
        rows += [row, row, row, row, np.diag([50.0, 50.0, 0.0]), row]
    gate = np.broadcast_to(np.asarray(rows), (2, len(xy), 3, 3))

    def plain_where_bad(chains, case, n_bad=len(bad)):
        want = [(2 + 6 * k + 2, 2 + 6 * k + 2) for k in range(n_bad)] + [(2 + 6 * k + 4, 2 + 6 * k + 4) for k in range(n_bad)]
        assert chains[0] == sorted(want), chains[0]
        assert [c for c in chains[0] if (c[0] - 2) % 6 == 2] == plain_chains(case)[0]
    yield gate_case("rows that are no covariance fall back to the plain test", xy, [], [0, 0], 3.0, 1, 5.991, gate, plain_where_bad)

    # the wider visitable set links a run: scans 2-4 lie within 3 m but hang on the query only through scan 1 at 3.5 m, which
    # the plain walk cannot pass (not visitable) -- a chain; with Dxx = 3 and chi2 = 9 scan 1 is visitable and 2-4 are linked scans
    xy = [(0.0, 0.0), (3.5, 0.0), (2.0, 0.0), (2.125, 0.0), (2.25, 0.0), far]
    gate = np.zeros((2, 6, 3, 3))
    gate[0] = np.diag([3.0, 0.0, 0.0])

    def linked(chains, case):
        assert plain_chains(case) == [[(2, 4)], [(2, 4)]]
        assert chains == [[], [(2, 4)]], chains
    yield gate_case("the wider visitable set links a run the plain walk leaves as a chain", xy, [(0, 1), (1, 2), (2, 3), (3, 4)], [0, 0], 3.0, 2,
                    9.0, gate, linked)
