"""CPU: the covariance entry points (kh_spa_compute_covariances, kh_spa_get_covariances, kh_spa_get_joint_covariance,
kh_spa_covariance_device, kh_mapper_get_covariances) are declared with prototypes, the summary struct has the header's size, every
invalid argument is refused with KH_ERR_INVALID_ARG before a device is looked for, and -- there is no CPU fallback -- a valid call
answers KH_ERR_NO_DEVICE where no device is visible.  (A solver cannot exist without a device, so the handle is NULL throughout:
that is what is wrong with an otherwise valid call where a device is visible.)"""
import ctypes as C

import numpy as np

from slam_toolbox_amd import capi

NEW = ("kh_spa_compute_covariances", "kh_spa_get_covariances", "kh_spa_get_joint_covariance", "kh_spa_covariance_device",
       "kh_mapper_get_covariances")


def without_a_device(lib, rc):
    if lib.kh_device_count() > 0:
        assert rc == capi.KH_ERR_INVALID_ARG                   # a device is visible: the NULL handle is what is wrong
    else:
        assert rc == capi.KH_ERR_NO_DEVICE and b"no CPU fallback" in lib.kh_last_error()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_new_entry_points_are_bound(kartohip_lib):
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(kartohip_lib, name).argtypes is not None, name


def test_summary_struct_matches_the_header():
    # 4 int32 + 5 doubles + 1 int64
    assert C.sizeof(capi.KhSpaCovSummary) == 64
    assert capi.KhSpaCovSummary.linearize_ms.offset == 16 and capi.KhSpaCovSummary.inverse_flops.offset == 56
    assert [k for k, _ in capi.KhSpaCovSummary._fields_] == ["n_free", "levels", "analysis", "pad", "linearize_ms", "factor_ms",
                                                             "inverse_ms", "gather_ms", "total_ms", "inverse_flops"]


def test_bad_arguments_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    cov, ids = np.zeros(36), np.zeros(4, dtype=np.int32)
    assert L.kh_spa_get_covariances(None, -1, ptr(ids), ptr(cov)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_covariances(None, 2, ptr(ids), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_covariances(None, 2, None, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_get_joint_covariance(None, 0, 1, None) == capi.KH_ERR_INVALID_ARG
    p, n = C.c_void_p(), C.c_int64()
    assert L.kh_spa_covariance_device(None, None, C.byref(n)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_covariance_device(None, C.byref(p), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_get_covariances(None, -3, ptr(ids), ptr(cov), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_get_covariances(None, 1, ptr(ids), None, None) == capi.KH_ERR_INVALID_ARG


def test_valid_calls_without_a_device_are_no_device(kartohip_lib):
    L = kartohip_lib
    cov, ids = np.zeros(36), np.zeros(4, dtype=np.int32)
    s = capi.KhSpaCovSummary()
    without_a_device(L, L.kh_spa_compute_covariances(None, C.byref(s)))
    without_a_device(L, L.kh_spa_compute_covariances(None, None))
    without_a_device(L, L.kh_spa_get_covariances(None, 4, ptr(ids), ptr(cov)))
    without_a_device(L, L.kh_spa_get_covariances(None, 0, None, None))
    without_a_device(L, L.kh_spa_get_joint_covariance(None, 0, 1, ptr(cov)))
    p, n = C.c_void_p(), C.c_int64()
    without_a_device(L, L.kh_spa_covariance_device(None, C.byref(p), C.byref(n)))
    without_a_device(L, L.kh_mapper_get_covariances(None, 4, ptr(ids), ptr(cov), C.byref(s)))
    without_a_device(L, L.kh_mapper_get_covariances(None, 0, None, None, None))
