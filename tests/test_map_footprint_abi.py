"""CPU: the ABI of the footprint analysis -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes, the
layout of the new structs, the status codes, and the argument checks that come before a device is looked for (then KH_ERR_NO_DEVICE on
a machine without one; with one, the NULL handle is the next thing refused).  A footprint is made from a field, and a field needs a
device: what create refuses of a polygon is tests/test_map_footprint_plan.py's, on the same code."""
import ctypes as C
import os
import re

import numpy as np

import map_footprint_rule as rule
from slam_toolbox_amd import capi
from test_map_localize_abi import _header_layout, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_footprint_create", "kh_map_footprint_recompute", "kh_map_footprint_destroy", "kh_map_footprint_stats_get", "kh_map_footprint_check",
         "kh_map_footprint_layer"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    sources = __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "map_footprint.cpp" in sources and "occupancy_footprint.hip" in sources
    from slam_toolbox_amd.map_field import MapField
    from slam_toolbox_amd.map_footprint import FOOTPRINT_DTYPE, MapFootprint
    from slam_toolbox_amd.map_localizer import MapLocalizer
    assert callable(MapLocalizer.footprint) and callable(MapField.footprint)
    assert all(hasattr(MapFootprint, k) for k in ("check", "check_path", "layer", "recompute", "stats", "close", "path_poses"))
    assert FOOTPRINT_DTYPE == rule.DTYPE and FOOTPRINT_DTYPE.itemsize == 32


def test_layouts_and_codes_match_the_header():
    ints = {"uint32_t": (4, 4), "uint64_t": (8, 8)}
    for name, struct, want_size in (("kh_footprint_t", capi.KhFootprint, 32), ("kh_footprint_layer_t", capi.KhFootprintLayer, 8 * 34),
                                    ("kh_map_footprint_stats", capi.KhMapFootprintStats, 56)):
        want, size = _header_layout(name, ints)
        assert _layout(struct) == want, name
        assert C.sizeof(struct) == size == want_size, name
    assert [k for k, _ in capi.KhFootprint._fields_] == list(rule.FIELDS)
    assert capi.KhFootprint.min_d2.offset == 24 and capi.KhFootprintLayer.n_any.offset == 256 and capi.KhMapFootprintStats.times_ms.offset == 32
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    codes = re.search(r"enum \{ (KH_FOOTPRINT_FREE.*?) \};", header).group(1)
    assert [c.strip() for c in codes.split(",")] == ["KH_FOOTPRINT_FREE = 0", "KH_FOOTPRINT_UNKNOWN = 1", "KH_FOOTPRINT_OUTSIDE = 2", "KH_FOOTPRINT_COLLISION = 3",
                                                     "KH_FOOTPRINT_LATTICE = 4"]
    assert (capi.KH_FOOTPRINT_FREE, capi.KH_FOOTPRINT_UNKNOWN, capi.KH_FOOTPRINT_OUTSIDE, capi.KH_FOOTPRINT_COLLISION, capi.KH_FOOTPRINT_LATTICE) == \
        (rule.FREE, rule.UNKNOWN, rule.OUTSIDE, rule.COLLISION, rule.LATTICE) == (0, 1, 2, 3, 4)
    assert "#define KH_FOOTPRINT_LAYER_REACH 64" in header and capi.KH_FOOTPRINT_LAYER_REACH == rule.LAYER_MAX_REACH == 64


def test_calls_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD     # a NULL handle is looked at after the device
    verts = np.array(rule.rectangle()).ravel()
    h = C.c_void_p(1)
    assert L.kh_map_footprint_create(None, 4, verts.ctypes.data, C.byref(h)) == BAD and h.value is None, "a refused create leaves NULL"
    assert L.kh_map_footprint_create(None, 4, verts.ctypes.data, None) == BAD and L.kh_map_footprint_create(None, 4, None, C.byref(h)) == BAD
    L.kh_map_footprint_destroy(None)
    assert L.kh_map_footprint_recompute(None, None) == BAD
    poses = np.array([1.0, 2.0, 0.3, 1.5, 2.5, -0.2])
    out = (capi.KhFootprint * 2)()
    check = lambda n=2, p=poses.ctypes.data, o=out: L.kh_map_footprint_check(None, n, p, o)  # noqa: E731
    assert check(n=0) == BAD and check(n=-1) == BAD and check(n=65537) == BAD and check(p=None) == BAD and check(o=None) == BAD
    for k, value in ((0, np.nan), (1, np.inf), (5, -np.inf)):
        bad = poses.copy()
        bad[k] = value
        assert check(p=bad.ctypes.data) == BAD, (k, value)
    assert check() == after and check(n=1) == after
    huge = np.array([1e300, -1e300, 1e300])
    assert check(n=1, p=huge.ctypes.data) == after, "a finite pose far off the lattice is a record, not a refusal"
    s = capi.KhFootprintLayer()
    for n_headings, max_status in ((0, 0), (33, 0), (-1, 0), (1, -1), (1, 3)):
        assert L.kh_map_footprint_layer(None, n_headings, max_status, None, C.byref(s)) == BAD, (n_headings, max_status)
    assert L.kh_map_footprint_layer(None, 1, 0, None, None) == after and L.kh_map_footprint_layer(None, 32, 2, None, C.byref(s)) == after
    st = capi.KhMapFootprintStats()
    assert L.kh_map_footprint_stats_get(None, None) == BAD and L.kh_map_footprint_stats_get(None, C.byref(st)) == after
