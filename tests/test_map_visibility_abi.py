"""CPU: the ABI of the visibility analysis -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes, the
layout of the new structs, the defaults, and the argument checks that come before a device is looked for (then KH_ERR_NO_DEVICE on a
machine without one; with one, the NULL handle is the next thing refused)."""
import ctypes as C
import math
import os
import re

import numpy as np

import map_visibility_rule as rule
from slam_toolbox_amd import capi
from test_map_localize_abi import MALFORMED, _header_layout, _laser, _layout, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_visibility_params_default", "kh_map_visibility_create", "kh_map_visibility_destroy", "kh_map_visibility_set_map", "kh_map_visibility_clear",
         "kh_map_visibility_commit", "kh_map_visibility_gain", "kh_map_visibility_select", "kh_map_visibility_read_mask", "kh_map_visibility_stats_get",
         "kh_map_visibility_set_skip"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    sources = __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "map_visibility.cpp" in sources and "occupancy_visibility.hip" in sources
    from slam_toolbox_amd.map_localizer import MapLocalizer
    from slam_toolbox_amd.map_visibility import VISIBILITY_DTYPE, MapVisibility
    assert callable(MapLocalizer.visibility) and all(hasattr(MapVisibility, k) for k in ("gain", "commit", "clear", "mask", "select", "set_map", "stats", "close",
                                                                                         "candidates"))
    assert VISIBILITY_DTYPE == rule.DTYPE and VISIBILITY_DTYPE.itemsize == 40


def test_layouts_match_the_header():
    ints = {"uint32_t": (4, 4)}
    for name, struct, want_size in (("kh_visibility_params", capi.KhVisibilityParams, 16), ("kh_visibility_t", capi.KhVisibility, 40),
                                    ("kh_map_visibility_stats", capi.KhMapVisibilityStats, 56)):
        want, size = _header_layout(name, ints)
        assert _layout(struct) == want, name
        assert C.sizeof(struct) == size == want_size, name
    assert [k for k, _ in capi.KhVisibility._fields_] == list(rule.FIELDS)
    assert capi.KhVisibility.gain.offset == 24 and capi.KhMapVisibilityStats.rounds.offset == 32 and capi.KhMapVisibilityStats.kernel_ms.offset == 40


def test_defaults(kartohip_lib):
    p = capi.KhVisibilityParams(7, 7, 7, 7)
    kartohip_lib.kh_map_visibility_params_default(C.byref(p))
    assert {k: getattr(p, k) for k in rule.PARAMS} == rule.PARAMS == dict(max_unknown=20, w_unknown=1, w_free=0, w_occupied=0)
    kartohip_lib.kh_map_visibility_params_default(None)        # a NULL output is ignored


def test_create_is_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    v, laser, p, h = _view(), _laser(), capi.KhVisibilityParams(), C.c_void_p(1)
    L.kh_map_visibility_params_default(C.byref(p))
    call = lambda **kw: L.kh_map_visibility_create(kw.get("view", C.byref(v)), kw.get("laser", C.byref(laser)), kw.get("params", C.byref(p)),  # noqa: E731
                                                   kw.get("out", C.byref(h)))
    for kw in (dict(view=None), dict(laser=None), dict(params=None), dict(out=None)):
        h.value = 1
        assert call(**kw) == BAD, kw
        assert "out" in kw or h.value is None, "a refused create leaves NULL"
    for field, value in MALFORMED:
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        assert call(view=C.byref(w)) == BAD, field
    for field, value in (("n_beams", 0), ("range_threshold", math.inf), ("range_threshold", 0.0), ("range_threshold", (2 ** 20 - 1) / 20.0), ("range_threshold", math.nan),
                         ("minimum_range", math.nan), ("maximum_range", math.nan), ("minimum_angle", math.nan), ("angular_resolution", math.inf),
                         ("range_threshold", 510 / 20.0), ("range_threshold", 100.0)):                          # ... and a reach of 512
        l2 = capi.KhLaser.from_buffer_copy(laser)
        setattr(l2, field, value)
        assert call(laser=C.byref(l2)) == BAD, (field, value)
    for field, value in (("max_unknown", -2), ("w_unknown", 0), ("w_unknown", -1), ("w_free", 256), ("w_occupied", -1)):
        q = capi.KhVisibilityParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert call(params=C.byref(q)) == BAD, field
    if L.kh_device_count() == 0:
        edge = capi.KhLaser.from_buffer_copy(laser)
        edge.range_threshold = float(np.nextafter(510 / 20.0, 0.0))                                            # reach 511
        q = capi.KhVisibilityParams(-1, 0, 0, 255)
        assert call() == NO_DEVICE and call(laser=C.byref(edge)) == NO_DEVICE and call(params=C.byref(q)) == NO_DEVICE and h.value is None
    w = capi.KhMapView.from_buffer_copy(v)
    w.device = 1 << 20
    assert call(view=C.byref(w)) == NO_DEVICE, "a device that does not exist"
    L.kh_map_visibility_destroy(None)


def test_calls_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD     # a NULL handle is looked at after the device
    poses = np.array([1.0, 2.0, 0.3, 1.5, 2.5, -0.2])
    out, ms = (capi.KhVisibility * 2)(), C.c_double(7.0)
    picks, gains, n = (C.c_int32 * 4)(), (C.c_uint32 * 4)(), C.c_int32(9)
    assert L.kh_map_visibility_gain(None, 2, None, out, C.byref(ms)) == BAD and ms.value == 0.0
    assert L.kh_map_visibility_gain(None, 2, poses.ctypes.data, None, None) == BAD
    assert L.kh_map_visibility_gain(None, 0, poses.ctypes.data, out, None) == BAD and L.kh_map_visibility_gain(None, 65537, poses.ctypes.data, out, None) == BAD
    assert L.kh_map_visibility_gain(None, 2, poses.ctypes.data, out, None) == after
    assert L.kh_map_visibility_commit(None, 2, None) == BAD and L.kh_map_visibility_commit(None, 0, poses.ctypes.data) == BAD
    assert L.kh_map_visibility_commit(None, -1, poses.ctypes.data) == BAD and L.kh_map_visibility_commit(None, 2, poses.ctypes.data) == after
    select = lambda **kw: L.kh_map_visibility_select(None, kw.get("n", 2), kw.get("poses", poses.ctypes.data), kw.get("k", 2), kw.get("min_gain", 1),  # noqa: E731
                                                     kw.get("picks", picks), kw.get("gains", gains), kw.get("n_picked", C.byref(n)))
    for kw in (dict(poses=None), dict(picks=None), dict(gains=None), dict(n_picked=None), dict(n=0), dict(n=65537), dict(k=0), dict(k=3), dict(k=-1), dict(min_gain=0)):
        assert select(**kw) == BAD, kw
    assert n.value == 0
    assert select() == after and select(k=1, min_gain=0xFFFFFFFF) == after
    for k, value in ((0, math.nan), (1, math.inf), (2, math.nan), (3, 1e12), (4, -(2.0 ** 30 + 1.0))):
        bad = poses.copy()
        bad[k] = value
        assert L.kh_map_visibility_gain(None, 2, bad.ctypes.data, out, None) == BAD and L.kh_map_visibility_commit(None, 2, bad.ctypes.data) == BAD
        assert select(poses=bad.ctypes.data) == BAD, (k, value)
    v = _view()
    assert L.kh_map_visibility_set_map(None, None) == BAD and L.kh_map_visibility_set_map(None, C.byref(v)) == after
    for field, value in MALFORMED:
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        assert L.kh_map_visibility_set_map(None, C.byref(w)) == BAD, field
    st = capi.KhMapVisibilityStats()
    assert L.kh_map_visibility_stats_get(None, None) == BAD and L.kh_map_visibility_stats_get(None, C.byref(st)) == after
    assert L.kh_map_visibility_read_mask(None, None) == BAD and L.kh_map_visibility_read_mask(None, picks) == after
    assert L.kh_map_visibility_clear(None) == after
    assert L.kh_map_visibility_set_skip(None, 2) == BAD and L.kh_map_visibility_set_skip(None, -1) == BAD and L.kh_map_visibility_set_skip(None, 0) == after
