"""CPU: the ABI of the ray cast and of the map alignment -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with
prototypes, the layout of the new structs, the codes, the defaults, and the argument checks that come before a device is looked for
(then KH_ERR_NO_DEVICE on a machine without one; with one, the NULL handle is the next thing refused)."""
import ctypes as C
import math
import os
import re

import numpy as np

from slam_toolbox_amd import capi
from test_map_localize_abi import MALFORMED, _header_layout, _laser, _layout, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_raycast", "kh_map_align_params_default", "kh_map_align"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    assert "map_align.cpp" in __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES


def test_layouts_and_codes_match_the_header():
    want, size = _header_layout("kh_ray_t", {})
    assert _layout(capi.KhRay) == want
    assert C.sizeof(capi.KhRay) == size == 24 == capi.RAY_DTYPE.itemsize
    assert [capi.RAY_DTYPE.fields[k][1] for k in ("range", "cell", "steps", "code")] == [0, 8, 16, 20]
    nested = {"kh_merge_fit_t": (C.sizeof(capi.KhMergeFit), 8), "kh_map_relocalize_params": (C.sizeof(capi.KhMapRelocalizeParams), 8), "uint64_t": (8, 8)}
    for name, struct, want_size in (("kh_map_align_params", capi.KhMapAlignParams, 144), ("kh_map_align_cand", capi.KhMapAlignCand, 128)):
        want, size = _header_layout(name, nested)
        assert _layout(struct) == want, name
        assert C.sizeof(struct) == size == want_size, name
    assert capi.KhMapAlignParams.min_known.offset == 24 and capi.KhMapAlignParams.initial.offset == 32 and capi.KhMapAlignParams.relocalize.offset == 56
    assert capi.KhMapAlignCand.probe_seed.offset == 24 and capi.KhMapAlignCand.fit.offset == 48
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name, value in (("KH_RAY_FREE", 0), ("KH_RAY_HIT", 1), ("KH_RAY_UNKNOWN", 2)):
        assert int(re.search(name + r" = (\d+)", header).group(1)) == getattr(capi, name) == value, name


def after_the_arguments(L, rc):
    """every argument was taken: no device, or (with one) the NULL handle"""
    return rc == (NO_DEVICE if L.kh_device_count() == 0 else BAD)


def test_raycast_arguments(kartohip_lib):
    L = kartohip_lib
    v, laser = _view(), _laser()
    poses, out, ms = np.array([1.0, 2.0, 0.3, 1.5, 2.5, -0.2]), (capi.KhRay * 16)(), C.c_double(7.0)
    args = lambda **kw: [kw.get("view", C.byref(v)), kw.get("laser", C.byref(laser)), kw.get("n", 2), kw.get("poses", poses.ctypes.data),  # noqa: E731
                         kw.get("budget", -1), kw.get("no_return", math.nan), kw.get("out", out), kw.get("ms", C.byref(ms))]
    for kw in (dict(view=None), dict(laser=None), dict(poses=None), dict(out=None), dict(n=0), dict(n=-1), dict(budget=-2), dict(budget=-(2 ** 31))):
        assert L.kh_map_raycast(*args(**kw)) == BAD, kw
    assert ms.value == 0.0
    for field, value in MALFORMED:
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        assert L.kh_map_raycast(*args(view=C.byref(w))) == BAD, field
    for field, value in (("n_beams", 0), ("range_threshold", math.inf), ("range_threshold", 0.0), ("range_threshold", (2 ** 20 - 1) / 20.0),
                         ("range_threshold", math.nan), ("minimum_range", math.nan), ("maximum_range", math.nan), ("minimum_angle", math.nan),
                         ("angular_resolution", math.inf)):
        l2 = capi.KhLaser.from_buffer_copy(laser)
        setattr(l2, field, value)
        assert L.kh_map_raycast(*args(laser=C.byref(l2))) == BAD, field
    for k, value in ((0, math.nan), (1, math.inf), (2, math.nan), (3, 1e12), (4, -(2.0 ** 30 / 20.0 + 1.0))):      # a walk that could leave the lattice
        bad = poses.copy()
        bad[k] = value
        assert L.kh_map_raycast(*args(poses=bad.ctypes.data)) == BAD, (k, value)
    if L.kh_device_count() == 0:
        for kw in (dict(), dict(ms=None), dict(budget=0), dict(budget=2 ** 31 - 1), dict(no_return=math.inf)):
            assert L.kh_map_raycast(*args(**kw)) == NO_DEVICE, kw


def test_align_defaults(kartohip_lib):
    L = kartohip_lib
    rp, p = capi.KhMapRelocalizeParams(), capi.KhMapAlignParams()
    L.kh_map_relocalize_params_default(None, C.byref(rp))
    p.n_probes = 77
    L.kh_map_align_params_default(None, C.byref(p))
    assert (p.probe_spacing, p.n_probes, p.top_k, p.max_unknown, p.min_known) == (rp.seed_spacing, 3, 4, 20, 0)
    assert list(p.initial) == [0.0, 0.0, 0.0]
    assert bytes(p.relocalize) == bytes(rp)
    L.kh_map_align_params_default(None, None)                  # a NULL output is ignored


def test_align_arguments(kartohip_lib):
    L = kartohip_lib
    v, p = _view(), capi.KhMapAlignParams()
    L.kh_map_align_params_default(None, C.byref(p))
    out, n, times = (capi.KhMapAlignCand * 4)(), C.c_int32(9), np.full(4, 7.0)
    call = lambda **kw: L.kh_map_align(None, kw.get("view", C.byref(v)), kw.get("params", C.byref(p)), kw.get("out", out), kw.get("cap", 4),  # noqa: E731
                                       kw.get("n", C.byref(n)), kw.get("times", times.ctypes.data))
    for kw in (dict(view=None), dict(params=None), dict(out=None), dict(cap=-1), dict(n=None)):
        assert call(**kw) == BAD, kw
    assert n.value == 0 and (times == 0.0).all()
    for field, value in MALFORMED:
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        assert call(view=C.byref(w)) == BAD, field
    for field, value in (("probe_spacing", 0.0), ("probe_spacing", -1.0), ("probe_spacing", math.inf), ("probe_spacing", math.nan), ("n_probes", 0),
                         ("top_k", 0), ("max_unknown", -2)):
        q = capi.KhMapAlignParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert call(params=C.byref(q)) == BAD, field
    for k in range(3):
        q = capi.KhMapAlignParams.from_buffer_copy(p)
        q.initial[k] = math.nan if k else math.inf
        assert call(params=C.byref(q)) == BAD, k
    for field, value in (("seed_spacing", 0.0), ("n_headings", -1), ("n_headings", 4097), ("radius", math.nan), ("minimum_response_fine", math.nan),
                         ("merge_heading", math.nan)):
        q = capi.KhMapAlignParams.from_buffer_copy(p)
        setattr(q.relocalize, field, value)
        assert call(params=C.byref(q)) == BAD, field
    assert after_the_arguments(L, call()), "a NULL localizer is looked at after the device"
    assert after_the_arguments(L, call(out=None, cap=0)) and after_the_arguments(L, call(times=None))
    q = capi.KhMapAlignParams.from_buffer_copy(p)
    q.max_unknown, q.min_known = -1, 2 ** 63
    assert after_the_arguments(L, call(params=C.byref(q))), "every min_known is valid"
