"""CPU: the ABI of the map merge -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes, the layout of
the two new structs, the codes, the defaults, and the argument checks that come before a device is looked for (then KH_ERR_NO_DEVICE
on a machine without one)."""
import ctypes as C
import math
import os
import re

from slam_toolbox_amd import capi
from test_map_localize_abi import MALFORMED, _header_layout, _layout, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_merge_params_default", "kh_map_merge_create", "kh_map_merge_destroy", "kh_map_merge_stats_get", "kh_map_merge_view",
         "kh_map_merge_read", "kh_map_merge_read_nav"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    assert "map_merge.cpp" in __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES


def test_layouts_and_codes_match_the_header():
    for name, struct, want_size in (("kh_map_merge_params", capi.KhMapMergeParams, 40), ("kh_map_merge_stats", capi.KhMapMergeStats, 128)):
        want, size = _header_layout(name, {"uint64_t": (8, 8)})
        assert _layout(struct) == want, name
        assert C.sizeof(struct) == size == want_size, name
    assert capi.KhMapMergeParams.footprint.offset == 24 and capi.KhMapMergeParams.grow.offset == 32
    assert capi.KhMapMergeStats.known_box.offset == 24 and capi.KhMapMergeStats.target_only.offset == 40
    assert capi.KhMapMergeStats.overlap.offset == 88 and capi.KhMapMergeStats.agreement.offset == 96 and capi.KhMapMergeStats.times_ms.offset == 104
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for k, name in enumerate(("NEITHER", "TARGET_ONLY", "MOVING_ONLY", "AGREE", "MOVING_OCCUPIED", "MOVING_FREE")):
        assert int(re.search("KH_MERGED_" + name + r" = (\d+)", header).group(1)) == getattr(capi, "KH_MERGED_" + name) == k, name
    for k, name in enumerate(("TARGET", "MOVING", "OCCUPIED", "UNKNOWN")):
        assert int(re.search("KH_MERGE_CONFLICT_" + name + r" = (\d+)", header).group(1)) == getattr(capi, "KH_MERGE_CONFLICT_" + name) == k, name


def test_defaults(kartohip_lib):
    L = kartohip_lib
    p = capi.KhMapMergeParams()
    p.footprint, p.conflict, p.grow, p.pad = 3, 1, 0, 9
    p.correction[1] = 4.0
    L.kh_map_merge_params_default(C.byref(p))
    assert list(p.correction) == [0.0, 0.0, 0.0]
    assert (p.footprint, p.conflict, p.grow, p.pad) == (0, capi.KH_MERGE_CONFLICT_OCCUPIED, 1, 0)
    L.kh_map_merge_params_default(None)                        # a NULL output is ignored


def test_create_arguments(kartohip_lib):
    L = kartohip_lib
    t, m, p, h = _view(), _view(), capi.KhMapMergeParams(), C.c_void_p(1)
    L.kh_map_merge_params_default(C.byref(p))
    p.correction[0], p.correction[1], p.correction[2] = 0.73, -0.41, 0.3
    call = lambda **kw: L.kh_map_merge_create(kw.get("target", C.byref(t)), kw.get("moving", C.byref(m)), kw.get("params", C.byref(p)),  # noqa: E731
                                              kw.get("out", C.byref(h)))
    for kw in (dict(target=None), dict(moving=None), dict(params=None)):
        h.value = 1
        assert call(**kw) == BAD, kw
        assert h.value is None, "a refused create leaves NULL"
    assert call(out=None) == BAD
    for which in ("target", "moving"):
        for field, value in MALFORMED:
            w = capi.KhMapView.from_buffer_copy(t)
            setattr(w, field, value)
            assert call(**{which: C.byref(w)}) == BAD, (which, field)
    for k in range(3):
        for value in (math.nan, math.inf, -math.inf):
            q = capi.KhMapMergeParams.from_buffer_copy(p)
            q.correction[k] = value
            assert call(params=C.byref(q)) == BAD, (k, value)
    for field, value in (("footprint", -1), ("footprint", 5), ("conflict", -1), ("conflict", 4), ("grow", -1), ("grow", 2)):
        q = capi.KhMapMergeParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert call(params=C.byref(q)) == BAD, (field, value)
    if L.kh_device_count() == 0:
        assert call() == NO_DEVICE and h.value is None
        for field, value in (("footprint", 0), ("footprint", 4), ("conflict", 0), ("conflict", 3), ("grow", 0)):
            q = capi.KhMapMergeParams.from_buffer_copy(p)
            setattr(q, field, value)
            assert call(params=C.byref(q)) == NO_DEVICE, (field, value)
        other = capi.KhMapView.from_buffer_copy(m)
        other.device = 1
        assert call(moving=C.byref(other)) == NO_DEVICE, "the devices are compared after one is looked for"


def test_handle_calls(kartohip_lib):
    L = kartohip_lib
    st, v = capi.KhMapMergeStats(), capi.KhMapView()
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD     # a NULL handle is looked at after the device
    L.kh_map_merge_destroy(None)
    assert L.kh_map_merge_stats_get(None, None) == BAD and L.kh_map_merge_view(None, None) == BAD and L.kh_map_merge_read_nav(None, None) == BAD
    assert L.kh_map_merge_stats_get(None, C.byref(st)) == after and L.kh_map_merge_view(None, C.byref(v)) == after
    assert L.kh_map_merge_read(None, None, None) == after
    out = (C.c_int8 * 4)()
    assert L.kh_map_merge_read_nav(None, out) == after
