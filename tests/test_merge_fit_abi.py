"""CPU: the fit and alignment entry points of the merger (kh_merge_fit, kh_merge_fit_stats, kh_merge_align_params_default,
kh_merge_align) are declared with prototypes, their structs have the header's sizes, the defaults are the documented ones, every
invalid argument is refused with KH_ERR_INVALID_ARG before a device is looked for, and -- there is no CPU fallback -- a valid call
answers KH_ERR_NO_DEVICE where no device is visible.  (A merger cannot exist without a device, so the merger is NULL throughout:
that is what is wrong with an otherwise valid call where a device is visible.)"""
import ctypes as C

import numpy as np
import pytest

from slam_toolbox_amd import capi

NEW = ("kh_merge_fit", "kh_merge_fit_stats", "kh_merge_align_params_default", "kh_merge_align")


def defaults(lib):
    p = capi.KhMergeAlignParams()
    lib.kh_merge_align_params_default(None, 0, C.byref(p))
    return p


def fit(lib, corrections=(0.0, 0.0, 0.0), n=None, out=True, threshold=0.1):
    c = None if corrections is None else np.ascontiguousarray(corrections, dtype=np.float64)
    n = (c.size // 3 if c is not None else 1) if n is None else n
    res = (capi.KhMergeFit * 4)()
    return lib.kh_merge_fit(None, 0, n, None if c is None else c.ctypes.data, 2, threshold, res if out else None)


def align(lib, p, moving=0, target=1, cap=4, out=True, count=True):
    res = (capi.KhMergeAlignCand * 4)()
    n = C.c_int32(-7)
    return lib.kh_merge_align(None, moving, target, C.byref(p) if p is not None else None, res if out else None, cap,
                              C.byref(n) if count else None, None)


def without_a_device(lib, rc):
    if lib.kh_device_count() > 0:
        assert rc == capi.KH_ERR_INVALID_ARG                   # a device is visible: the NULL merger is what is wrong
    else:
        assert rc == capi.KH_ERR_NO_DEVICE and b"no CPU fallback" in lib.kh_last_error()


def test_new_entry_points_are_bound(kartohip_lib):
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(kartohip_lib, name).argtypes is not None, name


def test_structs_match_the_header():
    # 9 uint64 + 1 double / 2 int32 + uint64 + 2 uint32 + double + kh_relocalize_params (48) / 3 doubles + 2 int32 + double + 2 int32 + fit
    assert C.sizeof(capi.KhMergeFit) == 80 and C.sizeof(capi.KhMergeAlignParams) == 80 and C.sizeof(capi.KhMergeAlignCand) == 128
    assert capi.KhMergeAlignParams.relocalize.offset == 32 and capi.KhMergeAlignCand.fit.offset == 48
    from slam_toolbox_amd import merge
    assert merge.FIT_DTYPE.itemsize == 80 and merge.ALIGN_DTYPE.itemsize == 128
    assert merge.ALIGN_DTYPE.fields["fit"][1] == 48 and merge.ALIGN_DTYPE.fields["index"][1] == 40


def test_documented_defaults(kartohip_lib):
    p = defaults(kartohip_lib)
    assert (p.n_probes, p.top_k, p.min_known, p.min_pass_through, p.pad, p.occupancy_threshold) == (4, 4, 0, 2, 0, 0.1)
    r = capi.KhRelocalizeParams()
    kartohip_lib.kh_relocalize_params_default(None, C.byref(r))
    assert bytes(p.relocalize) == bytes(r)
    kartohip_lib.kh_merge_align_params_default(None, 0, None)               # tolerated


def test_fit_refuses_bad_arguments_before_a_device_is_looked_for(kartohip_lib):
    assert fit(kartohip_lib, corrections=None) == capi.KH_ERR_INVALID_ARG
    assert fit(kartohip_lib, out=False) == capi.KH_ERR_INVALID_ARG
    assert fit(kartohip_lib, n=0) == capi.KH_ERR_INVALID_ARG
    assert fit(kartohip_lib, n=-2) == capi.KH_ERR_INVALID_ARG
    for k in range(6):
        for bad in (float("nan"), float("inf"), float("-inf")):
            c = np.zeros(6)
            c[k] = bad
            assert fit(kartohip_lib, corrections=c) == capi.KH_ERR_INVALID_ARG, (k, bad)
    for bad in (float("nan"), float("inf")):
        assert fit(kartohip_lib, threshold=bad) == capi.KH_ERR_INVALID_ARG
    assert kartohip_lib.kh_merge_fit_stats(None, np.zeros(4, dtype=np.int64)) == capi.KH_ERR_INVALID_ARG


@pytest.mark.parametrize("field,value", [("n_probes", 0), ("n_probes", -1), ("top_k", 0), ("top_k", -4), ("occupancy_threshold", float("nan")),
                                         ("occupancy_threshold", float("inf"))])
def test_align_refuses_bad_parameters(kartohip_lib, field, value):
    p = defaults(kartohip_lib)
    setattr(p, field, value)
    assert align(kartohip_lib, p) == capi.KH_ERR_INVALID_ARG


@pytest.mark.parametrize("field,value", [("seed_spacing", 0.0), ("seed_spacing", float("nan")), ("n_headings", -1), ("max_base", 0),
                                         ("radius", float("nan"))])
def test_align_refuses_bad_relocalization_parameters(kartohip_lib, field, value):
    p = defaults(kartohip_lib)
    setattr(p.relocalize, field, value)
    assert align(kartohip_lib, p) == capi.KH_ERR_INVALID_ARG


def test_align_refuses_null_negative_and_self(kartohip_lib):
    p = defaults(kartohip_lib)
    assert align(kartohip_lib, None) == capi.KH_ERR_INVALID_ARG
    assert align(kartohip_lib, p, count=False) == capi.KH_ERR_INVALID_ARG
    assert align(kartohip_lib, p, cap=-1) == capi.KH_ERR_INVALID_ARG
    assert align(kartohip_lib, p, out=False) == capi.KH_ERR_INVALID_ARG          # cap 4 with nowhere to write
    assert align(kartohip_lib, p, moving=3, target=3) == capi.KH_ERR_INVALID_ARG
    assert b"itself" in kartohip_lib.kh_last_error()
    p.relocalize.center_xy[1] = float("inf")
    assert align(kartohip_lib, p) == capi.KH_ERR_INVALID_ARG


def test_valid_calls_without_a_device_are_no_device(kartohip_lib):
    without_a_device(kartohip_lib, fit(kartohip_lib, corrections=np.zeros(6)))
    p = defaults(kartohip_lib)
    p.relocalize.top_k = -5                                     # overridden by the alignment's own top_k: not looked at
    without_a_device(kartohip_lib, align(kartohip_lib, p))
    without_a_device(kartohip_lib, align(kartohip_lib, p, cap=0, out=False))
