"""CPU: the covariance-column entry points (kh_spa_compute_covariance_columns, kh_spa_get_covariance_column,
kh_spa_get_joint_covariance_any, kh_spa_get_relative_covariances, kh_mapper_get_relative_covariances) are exported and bound with
prototypes, the summary struct has the header's layout, every invalid argument is refused with KH_ERR_INVALID_ARG before a device is
looked for, and -- there is no CPU fallback -- a valid call answers KH_ERR_NO_DEVICE where no device is visible.  (A solver cannot
exist without a device, so the handle is NULL throughout: that is what is wrong with an otherwise valid call where one is visible.)"""
import ctypes as C
import os
import re

import numpy as np

from slam_toolbox_amd import capi

NEW = ("kh_spa_compute_covariance_columns", "kh_spa_get_covariance_column", "kh_spa_get_joint_covariance_any",
       "kh_spa_get_relative_covariances", "kh_mapper_get_relative_covariances")
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


def test_summary_struct_and_limit_match_the_header():
    # the embedded kh_spa_cov_summary (64 bytes), 2 int32, 3 doubles, 1 int64
    S = capi.KhSpaCovColumnsSummary
    assert C.sizeof(S) == 64 + 8 + 24 + 8
    assert S.cov.offset == 0 and S.n_queries.offset == 64 and S.path_fronts.offset == 68 and S.forward_ms.offset == 72
    assert S.backward_ms.offset == 80 and S.total_ms.offset == 88 and S.column_flops.offset == 96
    assert [k for k, _ in S._fields_] == ["cov", "n_queries", "path_fronts", "forward_ms", "backward_ms", "total_ms", "column_flops"]
    assert re.search(r"#define KH_SPA_MAX_COV_COLUMNS 64\b", open(HEADER).read()) and capi.KH_SPA_MAX_COV_COLUMNS == 64


def test_bad_arguments_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    out = np.zeros(9 * 70)
    ids = np.arange(70, dtype=np.int32)
    s = capi.KhSpaCovColumnsSummary()
    assert L.kh_spa_compute_covariance_columns(None, 0, ptr(ids), C.byref(s)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_compute_covariance_columns(None, -1, ptr(ids), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_compute_covariance_columns(None, 65, ptr(ids), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_compute_covariance_columns(None, 3, None, None) == capi.KH_ERR_INVALID_ARG
    twice = np.array([4, 9, 2, 9], dtype=np.int32)
    assert L.kh_spa_compute_covariance_columns(None, 4, ptr(twice), C.byref(s)) == capi.KH_ERR_INVALID_ARG
    assert b"twice" in L.kh_last_error()
    assert s.n_queries == 0 and s.total_ms == 0.0
    assert L.kh_spa_get_covariance_column(None, 1, -1, ptr(ids), ptr(out)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_covariance_column(None, 1, 2, ptr(ids), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_joint_covariance_any(None, 0, 1, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_relative_covariances(None, 1, -2, ptr(ids), ptr(out)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_relative_covariances(None, 1, 2, ptr(ids), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_get_relative_covariances(None, 1, -1, ptr(ids), ptr(out), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_get_relative_covariances(None, 1, 2, ptr(ids), None, C.byref(s)) == capi.KH_ERR_INVALID_ARG


def test_valid_calls_without_a_device_are_no_device(kartohip_lib):
    L = kartohip_lib
    out = np.zeros(9 * 64)
    ids = np.arange(64, dtype=np.int32)
    s = capi.KhSpaCovColumnsSummary()
    without_a_device(L, L.kh_spa_compute_covariance_columns(None, 1, ptr(ids), C.byref(s)))
    without_a_device(L, L.kh_spa_compute_covariance_columns(None, 64, ptr(ids), None))
    without_a_device(L, L.kh_spa_get_covariance_column(None, 3, 4, ptr(ids), ptr(out)))
    without_a_device(L, L.kh_spa_get_covariance_column(None, 3, 0, None, None))
    without_a_device(L, L.kh_spa_get_joint_covariance_any(None, 0, 1, ptr(out)))
    without_a_device(L, L.kh_spa_get_relative_covariances(None, 3, 4, ptr(ids), ptr(out)))
    without_a_device(L, L.kh_mapper_get_relative_covariances(None, 3, 4, ptr(ids), ptr(out), C.byref(s)))
    without_a_device(L, L.kh_mapper_get_relative_covariances(None, 3, 0, None, None, None))
