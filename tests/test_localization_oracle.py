"""CPU: (1) tests/near_by_rule.py -- the numpy restatement the GPU test of the near-by queries compares the kernels with --
against nanoflann itself: tests/golden/near_by.npz holds what the reference's KD-tree (same index type, metric and leaf size
as MapperGraph::FindNearByScan / FindNearByVertices, Mapper.cpp:1837-1912) answered for seeded random points, recorded by
tests/golden/make_golden_near_by.py.  This is the pin of the two quirks of the reference's radius search: maxDistance is
compared with the SQUARED distance, and the hits come back by ascending distance.  (2) the localization-mode entry points
exist in libkartohip.so with the documented signatures and check their arguments."""
import ctypes as C
import os

import numpy as np
import pytest

import near_by_rule
from slam_toolbox_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "near_by.npz")


def test_near_by_rule_equals_nanoflann():
    g = np.load(GOLDEN)
    points, queries, radii = g["points"], g["queries"], g["radii"]
    assert points.shape[0] >= 2000 and queries.shape[0] == 64 and radii.size == 3
    n_hits = 0
    for k, q in enumerate(queries):
        # the fixture is only an oracle where nanoflann's answer does not depend on its tree: no exact ties
        assert near_by_rule.best_two_differ(points, q)
        idx, d = near_by_rule.find_near_by_scan(points, q)
        assert idx == int(g["nearest"][k])
        assert np.float64(d).tobytes() == np.float64(g["nearest_dist_sq"][k]).tobytes()
        for j, r in enumerate(radii):
            assert near_by_rule.hits_are_distinct(points, q, r)
            want = g["hits"][g["hit_begin"][k, j]: g["hit_begin"][k, j + 1]]
            got = near_by_rule.find_near_by_vertices(points, q, r)
            assert np.array_equal(got, want), (k, j)
            n_hits += got.size
    assert n_hits > 1000


def test_radius_is_compared_with_the_squared_distance():
    """the quirk by itself: with radius 9.0 nanoflann returned the points closer than 3 (9 = 3 squared), not closer than 9"""
    g = np.load(GOLDEN)
    points, j = g["points"], int(np.argmax(g["radii"]))
    r = float(g["radii"][j])
    assert r > 1.0
    for k, q in enumerate(g["queries"]):
        want = g["hits"][g["hit_begin"][k, j]: g["hit_begin"][k, j + 1]]
        dist = np.hypot(points[:, 0] - q[0], points[:, 1] - q[1])
        assert np.count_nonzero(dist < r) > want.size or want.size == 0
        assert set(want) == set(np.nonzero(near_by_rule.dist_sq(points, q) < r)[0])
        assert np.all(np.diff(near_by_rule.dist_sq(points, q)[want]) > 0)       # ascending


def test_empty_store_rule():
    assert near_by_rule.find_near_by_scan(np.zeros((0, 2)), (1.0, 2.0)) == (-1, np.inf)
    assert near_by_rule.find_near_by_vertices(np.zeros((0, 2)), (1.0, 2.0), 3.0).size == 0


NEW_SYMBOLS = {
    "kh_graph_set_poses": [C.c_void_p, C.c_int32, C.c_void_p],
    "kh_graph_set_pose": [C.c_void_p, C.c_int32, C.c_void_p],
    "kh_graph_append_scan_with_pose": [C.c_void_p, C.c_void_p, C.c_void_p],
    "kh_graph_find_near_by_scan": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "kh_graph_find_near_by_vertices": [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
    "kh_mapper_process_localization": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p],
    "kh_mapper_process_against_node": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.c_void_p,
                                       C.c_void_p],
    "kh_mapper_process_against_nodes_near_by": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int32),
                                                C.c_void_p, C.c_void_p],
    "kh_mapper_clear_localization_buffer": [C.c_void_p],
    "kh_mapper_localization_buffer": [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
}


def test_localization_symbols_and_argument_checks(kartohip_lib):
    L = kartohip_lib
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name, argtypes in NEW_SYMBOLS.items():
        assert name in capi.SYMBOLS and hasattr(L, name), name
        assert f"KH_API int {name}(" in header, name
        assert list(getattr(L, name).argtypes) == argtypes, name
    buf = (C.c_double * 2048)()
    acc, n = C.c_int32(7), C.c_int32(7)
    ids = (C.c_int32 * 4)()
    bad = capi.KH_ERR_INVALID_ARG
    # no handle
    assert L.kh_mapper_process_localization(None, buf, buf, 0.0, C.byref(acc), None, None) == bad
    assert L.kh_mapper_process_against_node(None, buf, buf, 0.0, 0, C.byref(acc), None, None) == bad
    assert L.kh_mapper_process_against_nodes_near_by(None, buf, buf, 0.0, 1, C.byref(acc), None, None) == bad
    assert L.kh_mapper_clear_localization_buffer(None) == bad
    assert L.kh_mapper_localization_buffer(None, ids, 4, C.byref(n)) == bad
    assert L.kh_graph_set_poses(None, 0, None) == bad
    assert L.kh_graph_set_pose(None, 0, buf) == bad
    assert L.kh_graph_append_scan_with_pose(None, buf, buf) == bad
    assert L.kh_graph_find_near_by_scan(None, 1, buf, ids, None) == bad
    assert L.kh_graph_find_near_by_vertices(None, buf, 1.0, ids, 4, C.byref(n)) == bad


def test_localization_needs_a_device(kartohip_lib):
    """no CPU fallback: without a GPU neither the store the queries run on nor a mapper can be made"""
    L = kartohip_lib
    if L.kh_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert hasattr(L, "kh_graph_find_near_by_scan") and hasattr(L, "kh_mapper_process_localization")
    g = C.c_void_p()
    assert L.kh_graph_create(0, C.byref(g)) == capi.KH_ERR_NO_DEVICE and not g.value
    p, laser, m = capi.KhMapperParams(), capi.KhLaser(1081, -2.35, 0.004, 0.1, 20.0, 12.0, 0.0, 0.0, 0.0), C.c_void_p()
    L.kh_mapper_params_default(C.byref(p))
    assert L.kh_mapper_create(C.byref(p), C.byref(laser), 0, 8, C.byref(m)) == capi.KH_ERR_NO_DEVICE and not m.value
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    with pytest.raises(capi.KartoHipError) as err:
        MapperGraphSearch().FindNearByScan((0.0, 0.0))
    assert err.value.args and "status 2" in str(err.value)
