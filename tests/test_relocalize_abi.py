"""CPU: the relocalization entry points (kh_mapper_relocalize, kh_relocalize_params_default, kh_graph_relocalize_candidates) are
declared with prototypes, give the documented defaults, refuse every invalid argument with KH_ERR_INVALID_ARG before a device is
looked for, and -- there is no CPU fallback -- answer KH_ERR_NO_DEVICE where no device is visible."""
import ctypes as C

import numpy as np
import pytest

from slam_toolbox_amd import capi

NEW = ("kh_graph_relocalize_candidates", "kh_graph_last_relocalize_kernel_ms", "kh_relocalize_params_default", "kh_mapper_relocalize",
       "kh_mapper_get_params")


def defaults(lib, mapper_params=None):
    p = capi.KhRelocalizeParams()
    lib.kh_relocalize_params_default(None if mapper_params is None else C.byref(mapper_params), C.byref(p))
    return p


def call(lib, p, ranges=True, cap=4, out=True, summary=True, mapper=None):
    r = np.ones(8)
    hyps = (capi.KhRelocalizeHyp * 4)()
    s = capi.KhRelocalizeSummary()
    return lib.kh_mapper_relocalize(mapper, r.ctypes.data if ranges else None, C.byref(p) if p is not None else None, hyps if out else None, cap,
                                    C.byref(s) if summary else None)


def test_new_entry_points_are_bound(kartohip_lib):
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(kartohip_lib, name).argtypes is not None, name


def test_structs_match_the_header():
    # 1 double + 4 int32 + 3 doubles / 2 int32 + 30 doubles / 6 int32 + 5 doubles (include/karto_hip.h)
    assert C.sizeof(capi.KhRelocalizeParams) == 48 and C.sizeof(capi.KhRelocalizeHyp) == 248 and C.sizeof(capi.KhRelocalizeSummary) == 64


def test_documented_defaults(kartohip_lib):
    p = defaults(kartohip_lib)
    # loop_search_maximum_distance / 2 of the offline parameters, heading count left to the call, BASELINE config 3's longest chain
    assert (p.seed_spacing, p.n_headings, p.max_base, p.top_k, p.radius, tuple(p.center_xy)) == (1.5, 0, 40, 8, 0.0, (0.0, 0.0))
    mp = capi.KhMapperParams()
    kartohip_lib.kh_mapper_params_default(C.byref(mp))
    mp.loop_search_maximum_distance = 5.0
    assert defaults(kartohip_lib, mp).seed_spacing == 2.5
    kartohip_lib.kh_relocalize_params_default(None, None)               # tolerated


@pytest.mark.parametrize("field,value", [("seed_spacing", 0.0), ("seed_spacing", -1.5), ("seed_spacing", float("nan")), ("seed_spacing", float("inf")),
                                         ("n_headings", -1), ("max_base", 0), ("max_base", -3), ("top_k", -1), ("radius", float("nan"))])
def test_bad_parameters_are_invalid_arguments(kartohip_lib, field, value):
    p = defaults(kartohip_lib)
    setattr(p, field, value)
    assert call(kartohip_lib, p) == capi.KH_ERR_INVALID_ARG


def test_null_and_negative_arguments_are_invalid(kartohip_lib):
    p = defaults(kartohip_lib)
    assert call(kartohip_lib, p, ranges=False) == capi.KH_ERR_INVALID_ARG
    assert call(kartohip_lib, None) == capi.KH_ERR_INVALID_ARG
    assert call(kartohip_lib, p, summary=False) == capi.KH_ERR_INVALID_ARG
    assert call(kartohip_lib, p, cap=-1) == capi.KH_ERR_INVALID_ARG
    assert call(kartohip_lib, p, out=False) == capi.KH_ERR_INVALID_ARG          # cap 4 with nowhere to write
    p.center_xy[0] = float("inf")
    assert call(kartohip_lib, p) == capi.KH_ERR_INVALID_ARG
    assert kartohip_lib.kh_mapper_get_params(None, C.byref(capi.KhMapperParams())) == capi.KH_ERR_INVALID_ARG


def test_valid_call_without_a_device_is_no_device(kartohip_lib):
    """every argument but the mapper is valid (a mapper cannot exist without a device)"""
    rc = call(kartohip_lib, defaults(kartohip_lib))
    if kartohip_lib.kh_device_count() > 0:
        assert rc == capi.KH_ERR_INVALID_ARG                   # a device is visible: the NULL mapper is what is wrong
    else:
        assert rc == capi.KH_ERR_NO_DEVICE and b"no CPU fallback" in kartohip_lib.kh_last_error()


def test_enumeration_refuses_bad_arguments(kartohip_lib):
    n, begin = C.c_int32(-5), np.zeros(2, dtype=np.int32)
    f = kartohip_lib.kh_graph_relocalize_candidates
    assert f(None, 1.5, 3.0, 40, None, 0.0, None, 0, C.byref(n), begin.ctypes.data, None, 0, C.byref(n)) == capi.KH_ERR_INVALID_ARG
    assert kartohip_lib.kh_graph_last_relocalize_kernel_ms(None) == 0.0
