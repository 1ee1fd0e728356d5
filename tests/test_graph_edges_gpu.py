"""GPU: the graph-store kernels (k_loop_candidates, k_near_by_scan, k_near_by_radius, csrc/graph.hip) against oracle/loops.py and
tests/near_by_rule.py on the edge inputs of tests/graph_cases.py.  Every loop case is asked as a batch (two or more queries: the
kernel) and query by query (one query: the host route of kh_graph_find_loop_candidates_from); both must give the oracle's
chains, chain for chain, in order.  The near-by cases compare indices and the bits of dist_sq.  All comparisons are exact.
Around the table: truncated outputs, one handle across stores of every size, edits of the store between two batches (the
stale-store upload), and the arguments the host rejects before any launch.
tests/test_edge_cases_oracle.py checks on the CPU that each case sits on its edge."""
import ctypes as C

import numpy as np
import pytest

import graph_cases as gc
import near_by_rule
from oracle import loops

pytestmark = pytest.mark.gpu
LOOPS = list(gc.loop_cases())
NEAR = list(gc.near_cases())
SENTINEL = -77


@pytest.fixture(scope="module")
def search(kartohip_lib):
    """one store for the whole file: every case meets the scratch the cases before it left"""
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    s = MapperGraphSearch()
    yield s
    s.close()


def oracle_chains(case):
    starts = case.starts if case.starts is not None else [0] * len(case.queries)
    return [loops.find_possible_loop_closures(int(q), case.ref_xy, case.adj_ptr, case.adj_idx, case.max_distance, case.min_chain,
                                              start=int(s), n_visit=case.n_visit) for q, s in zip(case.queries, starts)]


def load(s, case):
    s.SetGraph(case.ref_xy, case.adj_ptr, case.adj_idx)
    if case.n_visit is not None:
        s.SetScanLimit(case.n_visit)


def run_case(s, case, alone=True):
    load(s, case)
    want = oracle_chains(case)
    got = s.FindPossibleLoopClosures(case.queries, case.max_distance, case.min_chain, starts=case.starts)
    assert got == want, f"{case.name}: the batch (kernel) differs from the oracle"
    case.check(got)                                   # the kernel's own chains sit on the edge too
    if alone:
        for k, q in enumerate(case.queries):
            one = s.FindPossibleLoopClosures([q], case.max_distance, case.min_chain, starts=None if case.starts is None else case.starts[k:k + 1])
            assert one == [want[k]], f"{case.name}: query {k} alone (host route) differs from the oracle"


@pytest.mark.parametrize("case", LOOPS, ids=[c.name for c in LOOPS])
def test_loop_case_equals_the_oracle(search, case):
    run_case(search, case)


def test_one_handle_across_the_table_large_small_large(kartohip_lib):
    """513 scans, then 1, then the next largest, the next smallest ...: flags, frontier and chain scratch sized for a bigger store
    and filled by the batch before are what a smaller store's batch runs in"""
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    s = MapperGraphSearch()
    order = gc.reuse_order(LOOPS)
    assert order[0].ref_xy.shape[0] > 500 and order[1].ref_xy.shape[0] == 1
    for case in order + order[::-1]:
        run_case(s, case, alone=False)
    s.close()


def raw_candidates(lib, handle, case, cap):
    """kh_graph_find_loop_candidates_from with a chains buffer of 2 * cap behind which SENTINEL values stand (NULL for cap 0)"""
    fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                     C.c_void_p)(("kh_graph_find_loop_candidates_from", lib))
    q = np.ascontiguousarray(case.queries, dtype=np.int32)
    begin = np.full(q.size + 1, SENTINEL, dtype=np.int32)
    buf = np.full(2 * cap + 8, SENTINEL, dtype=np.int32)
    total = np.full(1, SENTINEL, dtype=np.int32)
    rc = fn(handle, q.size, q.ctypes.data, None if case.starts is None else case.starts.ctypes.data, case.max_distance, case.min_chain,
            begin.ctypes.data, buf.ctypes.data if cap else None, cap, total.ctypes.data)
    return rc, int(total[0]), begin, buf


@pytest.mark.parametrize("name", ["starts: different per query", "run: good and out alternating over 257 scans, min_chain 1", "sizes: 513 scans, flags row of 516 bytes"])
def test_truncated_output(search, kartohip_lib, name):
    """cap_chains below the total: *n_chains and chain_begin are the full values, the first cap pairs are written and nothing
    behind them"""
    case = next(c for c in LOOPS if c.name == name)
    load(search, case)
    want = oracle_chains(case)
    flat = np.asarray([v for chains in want for pair in chains for v in pair], dtype=np.int32)
    total = flat.size // 2
    begin = np.concatenate([[0], np.cumsum([len(c) for c in want])])
    assert total >= 4
    for cap in (0, 1, total - 1, total):
        rc, got_total, got_begin, buf = raw_candidates(kartohip_lib, search._h, case, cap)
        assert rc == 0 and got_total == total and np.array_equal(got_begin, begin), cap
        assert np.array_equal(buf[:2 * cap], flat[:2 * cap]) and (buf[2 * cap:] == SENTINEL).all(), cap


def test_store_edits_reach_the_kernel(kartohip_lib):
    """the device copy of the store is refreshed by the first batch after an edit (kh_graph_append_scan_with_pose, kh_graph_add_edge,
    kh_graph_set_position, kh_graph_set_positions): a batch before each edit leaves the device copy current, the edit changes
    the answer, and the batch after it equals the oracle on the edited graph"""
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    xy, edges, q = gc.pattern(gc.RESUME)
    xy, edges = [tuple(p) for p in xy], list(edges)
    queries, d, m = [q, 3, q], gc.MAX_D, 3
    s = MapperGraphSearch()
    ptr, idx = gc.csr(len(xy), edges)
    s.SetGraph(np.array(xy), ptr, idx)
    s.SetPoses(np.array(xy))

    def batch():
        ptr, idx = gc.csr(len(xy), edges)
        want = [loops.find_possible_loop_closures(k, np.array(xy), ptr, idx, d, m) for k in queries]
        assert s.FindPossibleLoopClosures(queries, d, m) == want
        return want
    seen = [batch()]
    assert seen[0][0] == gc.RUNS

    def edited(what):
        seen.append(batch())
        assert seen[-1] != seen[-2], f"{what} does not change the answer"
    xy.append((1.0, 0.5))                                     # the run at the end of the list grows by one
    s.AppendScan(xy[-1], xy[-1])
    edited("append (a good scan)")
    for p in ((100.0, 50.0), (1.0, 0.5)):                     # an out-of-range scan ends that run; a run of one at the new end of the list
        xy.append(p)
        s.AppendScan(p, p)
    edited("append (out of range, then good)")
    edges.append((q, 5))                                      # the first scan of the run 5-8 becomes a linked scan: 6-8 is left
    s.AddEdge(q, 5)
    edited("add_edge")
    edges.append((5, 6))                                      # scan 6 is linked through it: 7-8 is shorter than min_chain
    s.AddEdge(5, 6)
    edited("add_edge behind the added edge")
    xy[2] = (200.0, 0.0)                                      # splits the run 0-3
    s.SetPosition(2, xy[2])
    edited("set_position")
    moved = np.array(xy) + (0.25, 0.0)
    moved[13:15] = (300.0, 0.0)
    xy = [tuple(p) for p in moved]
    s.SetPositions(moved)
    edited("set_positions")
    s.close()


def test_rejected_arguments_leave_the_handle_usable(search, kartohip_lib):
    """what the host refuses before any launch: the return code, and the next case still answers"""
    from slam_toolbox_amd import capi
    lib = kartohip_lib
    case = next(c for c in LOOPS if c.name == "starts: different per query")
    n = case.ref_xy.shape[0]
    run_case(search, case)
    for bad_starts, bad_queries, code in (([0, -1, 0, 0, 0], case.queries, capi.KH_ERR_INVALID_ARG), ([-1], case.queries[:1], capi.KH_ERR_INVALID_ARG),
                                          (case.starts, [0, 1, n, 2, 3], capi.KH_ERR_NOT_FOUND), (case.starts[:1], [n], capi.KH_ERR_NOT_FOUND),
                                          (case.starts[:2], [0, -1], capi.KH_ERR_NOT_FOUND)):
        rc, _, _, buf = raw_candidates(lib, search._h, case._replace(queries=np.asarray(bad_queries, dtype=np.int32),
                                                                     starts=np.asarray(bad_starts, dtype=np.int32)), 64)
        assert rc == code and (buf == SENTINEL).all(), (bad_starts, bad_queries)
        run_case(search, case, alone=False)
    assert lib.kh_graph_set_scan_limit(search._h, n + 1) == capi.KH_ERR_INVALID_ARG
    assert lib.kh_graph_set_scan_limit(search._h, -1) == capi.KH_ERR_INVALID_ARG
    run_case(search, case, alone=False)
    for bad in (n, -1):
        idx = case.adj_idx.copy()
        idx[idx.size // 2] = bad
        assert lib.kh_graph_set(search._h, n, case.ref_xy.reshape(-1), case.adj_ptr, idx) == capi.KH_ERR_INVALID_ARG
        got = search.FindPossibleLoopClosures(case.queries, case.max_distance, case.min_chain, starts=case.starts)      # the store it held
        assert got == oracle_chains(case)


# ---- near-by -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def load_near(s, case):
    n = case.poses.shape[0]
    s.SetGraph(case.poses, np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    s.SetPoses(case.poses)


@pytest.mark.parametrize("case", NEAR, ids=[c.name for c in NEAR])
def test_near_by_case_equals_the_rule(search, case):
    load_near(search, case)
    n = case.poses.shape[0]
    with np.errstate(over="ignore"):
        want = [gc.NearResult(near_by_rule.dist_sq(case.poses, q), near_by_rule.find_near_by_scan(case.poses, q),
                              [near_by_rule.find_near_by_vertices(case.poses, q, r) for r in case.radii]) for q in case.queries]
    idx, d2 = search.FindNearByScan(case.queries)
    assert ((0 <= idx) & (idx < n)).all(), "an index past the end of the store"
    assert list(idx) == [w.nearest[0] for w in want], case.name
    assert np.array_equal(bits(d2), bits([w.nearest[1] for w in want])), case.name
    hits = []
    for k, q in enumerate(case.queries):
        i1, d1 = search.FindNearByScan(q)
        assert i1 == want[k].nearest[0] and bits([d1])[0] == bits([want[k].nearest[1]])[0], f"{case.name}: query {k} alone"
        hits.append([search.FindNearByVertices(q, r) for r in case.radii])
        for r, got, exp in zip(case.radii, hits[-1], want[k].hits):
            assert list(got) == list(exp), f"{case.name}: query {k}, radius {r!r}"
    with np.errstate(over="ignore"):
        case.check([gc.NearResult(w.d2, (int(i), float(d)), h) for w, i, d, h in zip(want, idx, d2, hits)])


def test_near_by_vertices_with_a_short_output(search, kartohip_lib):
    """cap below the number of hits: *n_found is the total, cap entries are written, the sentinel behind them is intact -- on a store
    of one trip of k_near_by_radius, and on one of two trips with caps on either side of the first trip's 65 536 vertices"""
    for name, caps in ((gc.CAP_CASE, lambda n: (0, 1, 64, n - 1, n)), (gc.TRIP_CAP_CASE, lambda n: (0, 1, gc.NEAR_TRIP, n - 1))):
        case = next(c for c in NEAR if c.name == name)
        load_near(search, case)
        n = case.poses.shape[0]
        q = np.ascontiguousarray(case.queries[0], dtype=np.float64)
        want = near_by_rule.find_near_by_vertices(case.poses, q, gc.INF)
        assert want.size == n
        for cap in caps(n):
            out = np.full(cap + 4, SENTINEL, dtype=np.int32)
            found = C.c_int32(SENTINEL)
            rc = kartohip_lib.kh_graph_find_near_by_vertices(search._h, q.ctypes.data, gc.INF, out.ctypes.data if cap else None, cap, C.byref(found))
            assert rc == 0 and found.value == n, (name, cap)
            assert np.array_equal(out[:cap], want[:cap]) and (out[cap:] == SENTINEL).all(), (name, cap)
