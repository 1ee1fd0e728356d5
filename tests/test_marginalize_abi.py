"""CPU: the marginalizing-removal entry points (kh_spa_marginalize_nodes, kh_mapper_marginalize_nodes, kh_mapper_set_removal_mode)
are declared with prototypes, the structs have the header's layout (kh_mapper_stats grew by one field at its END), invalid
arguments are refused before a device is looked for, and a valid call answers KH_ERR_NO_DEVICE where no device is visible: there
is no CPU fallback.  (A solver cannot exist without a device, so the handle is NULL throughout.)"""
import ctypes as C

import numpy as np

from slam_toolbox_amd import capi

NEW = ("kh_spa_marginalize_nodes", "kh_mapper_marginalize_nodes", "kh_mapper_set_removal_mode")


def without_a_device(lib, rc):
    if lib.kh_device_count() > 0:
        assert rc == capi.KH_ERR_INVALID_ARG                   # a device is visible: the NULL handle is what is wrong
    else:
        assert rc == capi.KH_ERR_NO_DEVICE and b"no CPU fallback" in lib.kh_last_error()


def test_new_entry_points_are_bound(kartohip_lib):
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(kartohip_lib, name).argtypes is not None, name


def test_structs_match_the_header():
    # 6 int32 + 4 doubles
    assert C.sizeof(capi.KhMarginalizeSummary) == 56 and capi.KhMarginalizeSummary.pack_ms.offset == 24
    assert [k for k, _ in capi.KhMarginalizeSummary._fields_] == ["n_marginalized", "n_plain", "n_rounds", "n_added", "n_fused", "max_degree",
                                                                  "pack_ms", "kernel_ms", "apply_ms", "total_ms"]
    # 6 int64 + 5 doubles + 6 int64, then the new counter
    assert capi.KhMapperStats._fields_[-1][0] == "marginalize_fallbacks" and capi.KhMapperStats.marginalize_fallbacks.offset == 136
    assert C.sizeof(capi.KhMapperStats) == 144
    assert (capi.KH_REMOVE_PLAIN, capi.KH_REMOVE_MARGINALIZE) == (0, 1)


def test_bad_arguments_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    ids = np.zeros(4, dtype=np.int32)
    assert L.kh_spa_marginalize_nodes(None, -1, ids.ctypes.data_as(C.c_void_p), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_spa_marginalize_nodes(None, 2, None, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_marginalize_nodes(None, -1, ids.ctypes.data_as(C.c_void_p)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_marginalize_nodes(None, 2, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_set_removal_mode(None, capi.KH_REMOVE_MARGINALIZE) == capi.KH_ERR_INVALID_ARG


def test_valid_calls_without_a_device_are_no_device(kartohip_lib):
    L = kartohip_lib
    ids = np.zeros(4, dtype=np.int32)
    s = capi.KhMarginalizeSummary()
    without_a_device(L, L.kh_spa_marginalize_nodes(None, 4, ids.ctypes.data_as(C.c_void_p), C.byref(s)))
    without_a_device(L, L.kh_spa_marginalize_nodes(None, 0, None, None))
    without_a_device(L, L.kh_mapper_marginalize_nodes(None, 4, ids.ctypes.data_as(C.c_void_p)))
    without_a_device(L, L.kh_mapper_marginalize_nodes(None, 0, None))
