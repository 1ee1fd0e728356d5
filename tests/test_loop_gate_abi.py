"""CPU: the entry points of the covariance gate (kh_spa_get_difference_covariances, kh_mapper_get_difference_covariances,
kh_graph_find_loop_candidates_gated, kh_loop_gate_params_default, kh_mapper_set_loop_gate, kh_mapper_get_loop_gate,
kh_mapper_get_loop_gate_stats) are exported and bound with prototypes, the two structs have the header's layout, the defaults are
the documented ones, and every invalid argument is refused with KH_ERR_INVALID_ARG before a device is looked for.  (No solver,
graph store or mapper can exist without a device, so the handle is NULL throughout.)"""
import ctypes as C
import os
import re

import numpy as np

from slam_toolbox_amd import capi

NEW = ("kh_spa_get_difference_covariances", "kh_mapper_get_difference_covariances", "kh_graph_find_loop_candidates_gated",
       "kh_mapper_set_loop_gate", "kh_mapper_get_loop_gate", "kh_mapper_get_loop_gate_stats")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "karto_hip.h")


def without_a_device(lib, rc):
    if lib.kh_device_count() > 0:
        assert rc == capi.KH_ERR_INVALID_ARG                   # a device is visible: the NULL handle is what is wrong
    else:
        assert rc == capi.KH_ERR_NO_DEVICE and b"no CPU fallback" in lib.kh_last_error()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_new_entry_points_are_exported_and_bound(kartohip_lib):
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(kartohip_lib, name), name
        assert name in capi.SYMBOLS and getattr(kartohip_lib, name).argtypes is not None, name
        assert re.search(r"KH_API int " + name + r"\(", text), name
    assert hasattr(kartohip_lib, "kh_loop_gate_params_default") and "kh_loop_gate_params_default" in capi.SYMBOLS
    assert re.search(r"KH_API void kh_loop_gate_params_default\(", text)


def test_structs_match_the_header():
    P, S = capi.KhLoopGateParams, capi.KhLoopGateStats
    assert C.sizeof(P) == 8 + 4 * 8 and C.sizeof(S) == 3 * 8 + 2 * 8
    assert [k for k, _ in P._fields_] == ["enabled", "refresh_scans", "chi2_position", "chi2_jump", "covariance_scale", "max_reach"]
    assert P.enabled.offset == 0 and P.refresh_scans.offset == 4 and P.chi2_position.offset == 8 and P.max_reach.offset == 32
    assert [k for k, _ in S._fields_] == ["column_passes", "ungated_searches", "jump_rejected", "column_ms", "max_semi_axis"]
    text = open(HEADER).read()
    body = re.search(r"typedef struct kh_loop_gate_params \{(.*?)\} kh_loop_gate_params;", text, re.S).group(1)
    assert re.findall(r"(?:int32_t|double) (\w+);", body) == [k for k, _ in P._fields_]
    body = re.search(r"typedef struct kh_loop_gate_stats \{(.*?)\} kh_loop_gate_stats;", text, re.S).group(1)
    assert re.findall(r"(?:int64_t|double) (\w+);", body) == [k for k, _ in S._fields_]
    # kh_mapper_stats is as it was
    assert C.sizeof(capi.KhMapperStats) == 18 * 8


def test_defaults(kartohip_lib):
    L = kartohip_lib
    p = capi.KhMapperParams()
    L.kh_mapper_params_default(C.byref(p))
    g = capi.KhLoopGateParams()
    L.kh_loop_gate_params_default(C.byref(p), C.byref(g))
    assert (g.enabled, g.refresh_scans, g.chi2_position, g.chi2_jump, g.covariance_scale) == (0, 1, 5.991, 7.815, 1.0)
    assert g.max_reach == p.loop_search_maximum_distance + p.loop_search_space_dimension / 2
    p.loop_search_maximum_distance, p.loop_search_space_dimension = 5.0, 12.0
    L.kh_loop_gate_params_default(C.byref(p), C.byref(g))
    assert g.max_reach == 11.0
    h = capi.KhLoopGateParams()
    L.kh_loop_gate_params_default(None, C.byref(h))                      # no parameters: the default distances
    assert h.max_reach == 3.0 + 8.0 / 2
    L.kh_loop_gate_params_default(C.byref(p), None)                      # (nothing to write to: no effect)


def test_bad_arguments_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    out = np.zeros(9 * 8)
    ids = np.arange(8, dtype=np.int32)
    s = capi.KhSpaCovColumnsSummary()
    assert L.kh_spa_get_difference_covariances(None, 1, -2, ptr(ids), ptr(out)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_difference_covariances(None, 1, 2, ptr(ids), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_get_difference_covariances(None, 1, -1, ptr(ids), ptr(out), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_get_difference_covariances(None, 1, 2, ptr(ids), None, C.byref(s)) == capi.KH_ERR_INVALID_ARG
    begin, chains, total = np.zeros(3, dtype=np.int32), np.zeros(32, dtype=np.int32), C.c_int32(0)
    q = np.zeros(2, dtype=np.int32)
    gate = np.zeros(2 * 9 * 4)
    for chi2, gp in ((1.0, None), (-1.0, ptr(gate)), (float("nan"), ptr(gate)), (-0.5, None)):
        assert L.kh_graph_find_loop_candidates_gated(None, 2, ptr(q), None, 3.0, 3, chi2, gp, ptr(begin), ptr(chains), 16,
                                                     C.byref(total)) == capi.KH_ERR_INVALID_ARG, chi2
    assert L.kh_graph_find_loop_candidates_gated(None, 2, ptr(q), None, 3.0, 3, 1.0, ptr(gate), ptr(begin), ptr(chains), 16,
                                                 C.byref(total)) == capi.KH_ERR_INVALID_ARG                     # (the NULL store)
    good = capi.KhLoopGateParams()
    L.kh_loop_gate_params_default(None, C.byref(good))
    assert L.kh_mapper_set_loop_gate(None, None) == capi.KH_ERR_INVALID_ARG
    for field, value in (("refresh_scans", 0), ("refresh_scans", -3), ("chi2_position", -1.0), ("chi2_position", float("nan")),
                         ("chi2_position", float("inf")), ("chi2_jump", float("nan")), ("covariance_scale", -0.5),
                         ("covariance_scale", float("nan")), ("covariance_scale", float("inf")), ("max_reach", 0.0), ("max_reach", -1.0),
                         ("max_reach", float("nan")), ("max_reach", float("inf"))):
        g = capi.KhLoopGateParams.from_buffer_copy(good)
        setattr(g, field, value)
        L.kh_clear_error() if hasattr(L, "kh_clear_error") else None
        assert L.kh_mapper_set_loop_gate(None, C.byref(g)) == capi.KH_ERR_INVALID_ARG, (field, value)
    assert L.kh_mapper_get_loop_gate(None, C.byref(good)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_get_loop_gate_stats(None, None) == capi.KH_ERR_INVALID_ARG


def test_valid_calls_without_a_device_are_no_device(kartohip_lib):
    L = kartohip_lib
    out = np.zeros(9 * 8)
    ids = np.arange(8, dtype=np.int32)
    s = capi.KhSpaCovColumnsSummary()
    without_a_device(L, L.kh_spa_get_difference_covariances(None, 3, 4, ptr(ids), ptr(out)))
    without_a_device(L, L.kh_spa_get_difference_covariances(None, 3, 0, None, None))
    without_a_device(L, L.kh_mapper_get_difference_covariances(None, 3, 4, ptr(ids), ptr(out), C.byref(s)))
    good = capi.KhLoopGateParams()
    L.kh_loop_gate_params_default(None, C.byref(good))
    for jump in (7.815, 0.0, -1.0, float("inf")):
        good.chi2_jump = jump
        without_a_device(L, L.kh_mapper_set_loop_gate(None, C.byref(good)))
