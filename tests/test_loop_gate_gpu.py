"""GPU: the gated loop-candidate enumeration (kh_graph_find_loop_candidates_gated: k_loop_candidates<gated> for a batch, the host
route for one query) against the numpy rule of tests/loop_gate_rule.py on the cases of tests/loop_gate_cases.py -- chains equal
exactly, as a batch and query by query -- and against kh_graph_find_loop_candidates_from on the reference's golden graph with
D = 0 and with chi2 = 0: chain_begin, chains and n_chains byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_gate_cases as lgc

pytestmark = pytest.mark.gpu
CASES = list(lgc.cases())
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "loop_candidates.npz"))
SENTINEL = -77


@pytest.fixture(scope="module")
def search(kartohip_lib):
    """one store for the whole file: every case meets the scratch (and the gate planes) the cases before it left"""
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    s = MapperGraphSearch()
    yield s
    s.close()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gated_case_equals_the_rule(search, case):
    search.SetGraph(case.ref_xy, case.adj_ptr, case.adj_idx)
    if case.n_visit is not None:
        search.SetScanLimit(case.n_visit)
    want = lgc.rule_chains(case)
    got = search.find_loop_candidates(case.queries, case.max_distance, case.min_chain, starts=case.starts, gate=case.gate, chi2=case.chi2)
    assert got == want, f"{case.name}: the batch (kernel) differs from the rule"
    case.check(got, case)
    for k, q in enumerate(case.queries):
        one = search.find_loop_candidates([q], case.max_distance, case.min_chain, starts=None if case.starts is None else case.starts[k:k + 1],
                                          gate=case.gate[k:k + 1], chi2=case.chi2)
        assert one == [want[k]], f"{case.name}: query {k} alone (host route) differs from the rule"
    # the null gates: the ungated call's answer
    plain = search.FindPossibleLoopClosures(case.queries, case.max_distance, case.min_chain, starts=case.starts)
    assert plain == lgc.plain_chains(case)
    assert search.find_loop_candidates(case.queries, case.max_distance, case.min_chain, starts=case.starts, gate=np.zeros_like(case.gate),
                                       chi2=case.chi2) == plain
    assert search.find_loop_candidates(case.queries, case.max_distance, case.min_chain, starts=case.starts,
                                       gate=np.where(np.isfinite(case.gate), case.gate, 0.0), chi2=0.0) == plain


def raw(lib, handle, queries, starts, d, m, cap, gate=None, chi2=0.0):
    """the two entry points with identical, sentinel-filled outputs"""
    q = np.ascontiguousarray(queries, dtype=np.int32)
    begin = np.full(q.size + 1, SENTINEL, dtype=np.int32)
    buf = np.full(2 * cap + 8, SENTINEL, dtype=np.int32)
    total = np.full(1, SENTINEL, dtype=np.int32)
    sp = None if starts is None else starts.ctypes.data_as(C.c_void_p)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    if gate is None:
        rc = lib.kh_graph_find_loop_candidates_from(handle, q.size, q, sp, d, m, begin, buf, cap, total.ctypes.data_as(C.POINTER(C.c_int32)))
    else:
        rc = lib.kh_graph_find_loop_candidates_gated(handle, q.size, ptr(q), sp, d, m, chi2, ptr(gate), ptr(begin), ptr(buf), cap,
                                                     total.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return begin.tobytes(), buf.tobytes(), total.tobytes()


def test_golden_graph_with_a_null_gate_is_the_ungated_call_byte_for_byte(search, kartohip_lib):
    xy, ptr, idx = G["ref_xy"], G["adj_ptr"], G["adj_idx"]
    n = xy.shape[0]
    d, m = float(G["loop_search_maximum_distance"]), int(G["loop_match_minimum_chain_size"])
    search.SetGraph(xy, ptr, idx)
    queries = np.arange(n, dtype=np.int32)
    zeros = np.zeros((n, n, 3, 3))
    some = np.ascontiguousarray(np.broadcast_to(lgc.random_rows(np.random.default_rng(3), 1, n, 4.0), (n, n, 3, 3)))
    n_chains = 0
    for starts in (None, np.zeros(n, dtype=np.int32), (queries // 2).astype(np.int32), np.full(n, n - 1, dtype=np.int32)):
        for cap in (4 * n, 3):
            want = raw(kartohip_lib, search._h, queries, starts, d, m, cap)
            assert raw(kartohip_lib, search._h, queries, starts, d, m, cap, gate=zeros, chi2=5.991) == want
            assert raw(kartohip_lib, search._h, queries, starts, d, m, cap, gate=some, chi2=0.0) == want
            n_chains += int(np.frombuffer(want[2], dtype=np.int32)[0])
    assert n_chains > 100
    for q in (0, 57, n - 1):                                   # one query: the host route of both
        one = np.array([q], dtype=np.int32)
        want = raw(kartohip_lib, search._h, one, None, d, m, 16)
        assert raw(kartohip_lib, search._h, one, None, d, m, 16, gate=zeros[:1], chi2=5.991) == want
        assert raw(kartohip_lib, search._h, one, None, d, m, 16, gate=some[:1], chi2=0.0) == want


def test_rejected_arguments_leave_the_store_usable(search, kartohip_lib):
    from slam_toolbox_amd import capi
    case = next(c for c in CASES if c.name.startswith("the wider visitable set"))
    search.SetGraph(case.ref_xy, case.adj_ptr, case.adj_idx)
    L = kartohip_lib
    q, begin, chains, total = case.queries, np.zeros(3, dtype=np.int32), np.zeros(32, dtype=np.int32), C.c_int32(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    gate = np.ascontiguousarray(case.gate)
    for chi2, gp in ((1.0, None), (-1.0, ptr(gate)), (float("nan"), ptr(gate))):
        assert L.kh_graph_find_loop_candidates_gated(search._h, 2, ptr(q), None, 3.0, 2, chi2, gp, ptr(begin), ptr(chains), 16,
                                                     C.byref(total)) == capi.KH_ERR_INVALID_ARG
    bad = np.array([0, 6], dtype=np.int32)
    assert L.kh_graph_find_loop_candidates_gated(search._h, 2, ptr(bad), None, 3.0, 2, 9.0, ptr(gate), ptr(begin), ptr(chains), 16,
                                                 C.byref(total)) == capi.KH_ERR_NOT_FOUND
    assert search.find_loop_candidates(case.queries, case.max_distance, case.min_chain, gate=case.gate, chi2=case.chi2) == lgc.rule_chains(case)
