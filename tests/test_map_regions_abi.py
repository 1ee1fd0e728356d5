"""CPU: the ABI of the region analysis -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes, the layout
of the new structs, the codes, the defaults, and the argument checks that come before a device is looked for (then KH_ERR_NO_DEVICE
on a machine without one).  A field cannot be made without a device, so kh_map_regions_create's parameter refusals and their order
are tests/test_map_regions_plan.py's."""
import ctypes as C
import math
import os
import re

import map_regions_rule as rule
from slam_toolbox_amd import capi
from test_map_localize_abi import _header_layout, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_regions_params_default", "kh_map_regions_create", "kh_map_regions_recompute", "kh_map_regions_destroy", "kh_map_regions_stats_get",
         "kh_map_regions_read", "kh_map_regions_get", "kh_map_regions_lookup"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    sources = __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "map_regions.cpp" in sources and "occupancy_regions.hip" in sources


def test_layouts_and_codes_match_the_header():
    ints = {"uint64_t": (8, 8), "uint32_t": (4, 4)}
    for name, struct, want_size in (("kh_map_regions_params", capi.KhMapRegionsParams, 32), ("kh_region", capi.KhRegion, 88),
                                    ("kh_map_regions_stats", capi.KhMapRegionsStats, 120)):
        want, size = _header_layout(name, ints)
        assert _layout(struct) == want, name
        assert C.sizeof(struct) == size == want_size, name
    assert capi.KhRegion.sum_i.offset == 24 and capi.KhRegion.max_d2.offset == 40 and capi.KhRegion.centroid.offset == 56
    assert capi.KhMapRegionsStats.n_traversable.offset == 24 and capi.KhMapRegionsStats.n_total.offset == 40 and capi.KhMapRegionsStats.times_ms.offset == 64
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    assert int(re.search(r"#define KH_REGION_NONE (0x[0-9A-Fa-f]+)u", header).group(1), 16) == capi.KH_REGION_NONE == rule.NONE
    assert int(re.search(r"#define KH_REGION_DROPPED (0x[0-9A-Fa-f]+)u", header).group(1), 16) == capi.KH_REGION_DROPPED == rule.DROPPED
    for k, name in enumerate(("KH_REGION_AT_OK", "KH_REGION_AT_NONE", "KH_REGION_AT_DROPPED", "KH_REGION_OUTSIDE")):
        assert int(re.search(name + r" = (\d+)", header).group(1)) == getattr(capi, name) == k, name
    assert (rule.AT_OK, rule.AT_NONE, rule.AT_DROPPED, rule.OUTSIDE) == (0, 1, 2, 3)
    for k, name in enumerate(("KH_REGIONS", "KH_FRONTIERS")):
        assert int(re.search(name + r" = (\d+)", header).group(1)) == getattr(capi, name) == k, name


def test_defaults(kartohip_lib):
    p = capi.KhMapRegionsParams(7.0, 1, 2, 3, 4, 5, 9)
    kartohip_lib.kh_map_regions_params_default(C.byref(p))
    assert {k: getattr(p, k) for k, _ in capi.KhMapRegionsParams._fields_ if k != "pad"} == rule.PARAMS and p.pad == 0
    kartohip_lib.kh_map_regions_params_default(None)           # a NULL output is ignored


def test_arguments_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD     # a NULL handle is looked at after the device
    p, h = capi.KhMapRegionsParams(), C.c_void_p(1)
    L.kh_map_regions_params_default(C.byref(p))
    assert L.kh_map_regions_create(None, C.byref(p), None) == BAD
    assert L.kh_map_regions_create(None, C.byref(p), C.byref(h)) == BAD and h.value is None, "a refused create leaves NULL"
    h.value = 1
    assert L.kh_map_regions_create(None, None, C.byref(h)) == BAD and h.value is None
    L.kh_map_regions_destroy(None)
    assert L.kh_map_regions_recompute(None, None) == BAD
    st = capi.KhMapRegionsStats()
    assert L.kh_map_regions_stats_get(None, None) == BAD and L.kh_map_regions_stats_get(None, C.byref(st)) == after
    ids = (C.c_uint32 * 4)()
    assert L.kh_map_regions_read(None, 0, None) == BAD and L.kh_map_regions_read(None, -1, ids) == BAD and L.kh_map_regions_read(None, 2, ids) == BAD
    assert L.kh_map_regions_read(None, 0, ids) == after and L.kh_map_regions_read(None, 1, ids) == after
    n, records = C.c_int32(5), (capi.KhRegion * 2)()
    assert L.kh_map_regions_get(None, 0, records, 2, None) == BAD and L.kh_map_regions_get(None, 2, records, 2, C.byref(n)) == BAD
    assert L.kh_map_regions_get(None, 0, records, -1, C.byref(n)) == BAD and L.kh_map_regions_get(None, 0, None, 2, C.byref(n)) == BAD
    assert L.kh_map_regions_get(None, 1, None, 0, C.byref(n)) == after and n.value == 0
    assert L.kh_map_regions_get(None, 0, records, 2, C.byref(n)) == after
    xy = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    assert L.kh_map_regions_lookup(None, 0, xy, None, None) == BAD and L.kh_map_regions_lookup(None, 2, None, None, None) == BAD
    for k, value in ((0, math.nan), (3, math.inf), (2, -math.inf)):
        bad = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
        bad[k] = value
        assert L.kh_map_regions_lookup(None, 2, bad, None, None) == BAD, (k, value)
    assert L.kh_map_regions_lookup(None, 2, xy, None, None) == after
