"""CPU: the ABI of the map change layer -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes, the
layout of the summary, and the argument checks that come before a device is looked for (then KH_ERR_NO_DEVICE on a machine without
one; with one, the NULL handle is the next thing refused)."""
import ctypes as C
import math
import os
import re

import numpy as np

from slam_toolbox_amd import capi
from test_map_localize_abi import MALFORMED, _header_layout, _laser, _layout, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_changes_create", "kh_map_changes_destroy", "kh_map_changes_clear", "kh_map_changes_decay", "kh_map_changes_observe",
         "kh_map_changes_diff", "kh_map_changes_read", "kh_map_changes_view", "kh_map_changes_read_nav"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    assert "map_changes.cpp" in __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES


def test_summary_layout_and_codes_match_the_header():
    want, size = _header_layout("kh_map_changes_summary_t", {})
    assert _layout(capi.KhMapChangesSummary) == want
    assert C.sizeof(capi.KhMapChangesSummary) == size == 112
    assert capi.KhMapChangesSummary.n_changed.offset == 48 and capi.KhMapChangesSummary.observe_kernel_ms.offset == 80
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in ("KH_BEAM_DROPPED", "KH_BEAM_EXPLAINED", "KH_BEAM_NOVEL", "KH_BEAM_UNKNOWN", "KH_BEAM_THROUGH", "KH_BEAM_CLEAR", "KH_CELL_UNOBSERVED",
                 "KH_CELL_CONFIRMED", "KH_CELL_APPEARED", "KH_CELL_VANISHED", "KH_CELL_DISCOVERED_OCCUPIED", "KH_CELL_DISCOVERED_FREE"):
        assert int(re.search(name + r" = (\d+)", header).group(1)) == getattr(capi, name), name


def after_the_arguments(L, rc):
    """every argument was taken: no device, or (with one) the NULL handle"""
    return rc == (NO_DEVICE if L.kh_device_count() == 0 else BAD)


def test_create_arguments(kartohip_lib):
    L = kartohip_lib
    v, h = _view(), C.c_void_p(1)
    assert L.kh_map_changes_create(C.byref(v), None) == BAD
    assert L.kh_map_changes_create(None, C.byref(h)) == BAD and h.value is None, "a refused create leaves NULL"
    for field, value in MALFORMED + (("device", -1),):
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        h = C.c_void_p(1)
        assert L.kh_map_changes_create(C.byref(w), C.byref(h)) == BAD and h.value is None, field
    if L.kh_device_count() == 0:
        assert L.kh_map_changes_create(C.byref(v), C.byref(h)) == NO_DEVICE and h.value is None
    L.kh_map_changes_destroy(None)


def test_observe_arguments(kartohip_lib):
    L = kartohip_lib
    laser = _laser()
    ranges, poses, labels = np.ones(16), np.array([1.0, 2.0, 0.3, 1.5, 2.5, -0.2]), np.zeros(32, dtype=np.int32)
    call = lambda **kw: L.kh_map_changes_observe(None, kw.get("laser", C.byref(laser)), kw.get("n", 2), kw.get("ranges", ranges.ctypes.data),  # noqa: E731
                                                 kw.get("poses", poses.ctypes.data), kw.get("t", 1), kw.get("labels", labels.ctypes.data))
    for kw in (dict(laser=None), dict(ranges=None), dict(poses=None), dict(n=0), dict(n=-1), dict(t=-1), dict(t=5)):
        assert call(**kw) == BAD, kw
    for field, value in (("n_beams", 0), ("range_threshold", math.inf), ("range_threshold", 0.0), ("range_threshold", math.nan),
                         ("minimum_range", math.nan), ("maximum_range", math.nan), ("minimum_angle", math.nan), ("angular_resolution", math.inf)):
        l2 = capi.KhLaser.from_buffer_copy(laser)
        setattr(l2, field, value)
        assert call(laser=C.byref(l2)) == BAD, field
    for k, value in ((0, math.nan), (1, math.inf), (2, math.nan), (5, -math.inf)):
        bad = poses.copy()
        bad[k] = value
        assert call(poses=bad.ctypes.data) == BAD, (k, value)
    assert after_the_arguments(L, call())
    assert after_the_arguments(L, call(labels=None)), "the labels are optional"
    assert after_the_arguments(L, call(t=0)) and after_the_arguments(L, call(t=4))


def test_the_other_calls(kartohip_lib):
    L = kartohip_lib
    for shift in (0, 32, -1):
        assert L.kh_map_changes_decay(None, shift) == BAD, shift
    assert after_the_arguments(L, L.kh_map_changes_decay(None, 1)) and after_the_arguments(L, L.kh_map_changes_decay(None, 31))
    assert after_the_arguments(L, L.kh_map_changes_clear(None))
    cells, s = np.zeros(6, dtype=np.int32), capi.KhMapChangesSummary()
    diff = lambda **kw: L.kh_map_changes_diff(None, 2, kw.get("threshold", 0.1), kw.get("cells", cells.ctypes.data), kw.get("cap", 2),  # noqa: E731
                                              kw.get("out", C.byref(s)))
    for kw in (dict(out=None), dict(cap=-1), dict(cells=None), dict(threshold=math.nan)):
        assert diff(**kw) == BAD, kw
    assert after_the_arguments(L, diff()) and after_the_arguments(L, diff(cells=None, cap=0)), "cap 0 needs no room"
    assert after_the_arguments(L, L.kh_map_changes_read(None, None, None, None, None))
    v, nav = capi.KhMapView(), np.zeros(4, dtype=np.int8)
    assert L.kh_map_changes_view(None, None) == BAD and L.kh_map_changes_read_nav(None, None) == BAD
    assert after_the_arguments(L, L.kh_map_changes_view(None, C.byref(v)))
    assert after_the_arguments(L, L.kh_map_changes_read_nav(None, nav.ctypes.data))
