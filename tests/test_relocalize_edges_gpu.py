"""GPU: the relocalization enumeration (k_seed_cover, k_prefix_list, k_base_gather, csrc/graph.hip) through
kh_graph_relocalize_candidates against tests/relocalize_rule.py on the edge inputs of tests/relocalize_cases.py: seed lists,
base_begin and base_idx compared exactly.  Around the table: one handle across stores of every size, the store after a vertex
left it (the list is renumbered), and truncated outputs.  tests/test_relocalize_rule_oracle.py checks on the CPU that each case
sits on its edge."""
import ctypes as C

import numpy as np
import pytest

import relocalize_cases as rc
import relocalize_rule as rr

pytestmark = pytest.mark.gpu
CASES = rc.cases()
SENTINEL = -77


@pytest.fixture(scope="module")
def search(kartohip_lib):
    """one store for the whole file: every case meets the scratch the cases before it left"""
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    s = MapperGraphSearch()
    yield s
    s.close()


def load(s, poses):
    n = poses.shape[0]
    s.SetGraph(poses, np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    s.SetPoses(poses)


def run_case(s, case):
    load(s, case.poses)
    want = rr.candidates(case.poses, case.spacing, case.max_distance, case.max_base, case.center, case.radius)
    got = s.RelocalizeCandidates(case.spacing, case.max_distance, case.max_base, case.center, case.radius)
    for name, g, w in zip(("seeds", "base_begin", "base_idx"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), f"{case.name}: {name} differs from the rule"
    case.check(*got)                                   # the library's own answer sits on the edge too


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_rule(search, case):
    run_case(search, case)


def test_one_handle_large_small_large(kartohip_lib):
    """513 vertices, then none, then the next largest, the next smallest ...: flags, prefixes and lists sized for a bigger store and
    filled by the call before are what a smaller store's call runs in"""
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    by_size = sorted(CASES, key=lambda c: c.poses.shape[0])
    order = []
    while by_size:
        order.append(by_size.pop())
        if by_size:
            order.append(by_size.pop(0))
    assert order[0].poses.shape[0] == 513 and order[1].poses.shape[0] == 0
    s = MapperGraphSearch()
    for case in order + order[::-1]:
        run_case(s, case)
    s.close()


def test_store_after_a_vertex_left(search):
    """a removal renumbers the list: the seed of the removed vertex's cell becomes the next vertex of that cell, and every index
    behind it moves down by one"""
    case = next(c for c in CASES if c.name.startswith("257"))
    load(search, case.poses)
    before = search.RelocalizeCandidates(case.spacing, case.max_distance, case.max_base)
    gone = int(before[0][3])                                          # a seed
    poses = np.delete(case.poses, gone, axis=0)
    load(search, poses)
    got = search.RelocalizeCandidates(case.spacing, case.max_distance, case.max_base)
    want = rr.candidates(poses, case.spacing, case.max_distance, case.max_base)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert not np.array_equal(got[0], before[0]) and got[0].size in (before[0].size, before[0].size - 1)


def test_truncated_output(search, kartohip_lib):
    """caps below the totals: *n_seeds and *n_base are the full values, the first cap entries are written and nothing behind them"""
    case = next(c for c in CASES if c.name.startswith("513"))
    load(search, case.poses)
    seeds, begin, idx = rr.candidates(case.poses, case.spacing, case.max_distance, case.max_base)
    for cap_s, cap_b in ((0, 0), (1, 3), (seeds.size - 1, idx.size - 1), (seeds.size, idx.size)):
        s = np.full(cap_s + 4, SENTINEL, dtype=np.int32)
        b = np.full(cap_s + 5, SENTINEL, dtype=np.int32)
        i = np.full(cap_b + 4, SENTINEL, dtype=np.int32)
        n_s, n_b = C.c_int32(SENTINEL), C.c_int32(SENTINEL)
        rc_ = kartohip_lib.kh_graph_relocalize_candidates(search._h, case.spacing, case.max_distance, case.max_base, None, 0.0,
                                                          s.ctypes.data if cap_s else None, cap_s, C.byref(n_s), b.ctypes.data,
                                                          i.ctypes.data if cap_b else None, cap_b, C.byref(n_b))
        assert rc_ == 0 and n_s.value == seeds.size and n_b.value == idx.size, (cap_s, cap_b)
        assert np.array_equal(s[:cap_s], seeds[:cap_s]) and (s[cap_s:] == SENTINEL).all(), (cap_s, cap_b)
        assert np.array_equal(b[:cap_s + 1], begin[:cap_s + 1]) and (b[cap_s + 1:] == SENTINEL).all(), (cap_s, cap_b)
        assert np.array_equal(i[:cap_b], idx[:cap_b]) and (i[cap_b:] == SENTINEL).all(), (cap_s, cap_b)


def test_rejected_arguments_leave_the_handle_usable(search, kartohip_lib):
    from slam_toolbox_amd import capi
    case = next(c for c in CASES if c.name.startswith("counts at"))
    run_case(search, case)
    n, begin = C.c_int32(0), np.zeros(8, dtype=np.int32)
    for spacing, max_base, cap in ((0.0, 5, 0), (-1.0, 5, 0), (float("nan"), 5, 0), (1.5, 0, 0), (1.5, 5, -1)):
        assert kartohip_lib.kh_graph_relocalize_candidates(search._h, spacing, 3.0, max_base, None, 0.0, None, cap, C.byref(n), begin.ctypes.data,
                                                           None, 0, C.byref(n)) == capi.KH_ERR_INVALID_ARG
    run_case(search, case)
    # a store without poses cannot answer
    search.SetGraph(case.poses, np.zeros(case.poses.shape[0] + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert kartohip_lib.kh_graph_relocalize_candidates(search._h, 1.5, 3.0, 5, None, 0.0, None, 0, C.byref(n), begin.ctypes.data, None, 0,
                                                       C.byref(n)) == capi.KH_ERR_INVALID_ARG
    run_case(search, case)
