"""CPU: the ABI of the travel costs -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes, the layout
of the new structs, the codes, the defaults, and the argument checks that come before a device is looked for (then KH_ERR_NO_DEVICE
on a machine without one).  A field cannot be made without a device, so kh_map_travel_create's parameter refusals and their order are
tests/test_map_travel_plan.py's."""
import ctypes as C
import math
import os
import re

import map_field_rule as fr
import map_travel_rule as rule
from slam_toolbox_amd import capi
from test_map_localize_abi import _header_layout, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_travel_params_default", "kh_map_travel_create", "kh_map_travel_recompute", "kh_map_travel_destroy", "kh_map_travel_solve",
         "kh_map_travel_stats_get", "kh_map_travel_read", "kh_map_travel_lookup", "kh_map_travel_paths", "kh_map_travel_set_rounds_per_check"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    sources = __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "map_travel.cpp" in sources and "occupancy_travel.hip" in sources
    from slam_toolbox_amd.map_field import MapField
    from slam_toolbox_amd.map_localizer import MapLocalizer
    from slam_toolbox_amd.map_travel import MapTravel
    assert callable(MapField.travel) and callable(MapLocalizer.travel) and all(hasattr(MapTravel, k) for k in ("solve", "values", "weights", "lookup", "paths", "rank",
                                                                                                               "recompute", "close"))


def test_layouts_and_codes_match_the_header():
    ints = {"uint64_t": (8, 8), "uint32_t": (4, 4), "kh_inflation_params": (C.sizeof(capi.KhInflationParams), 8)}
    assert C.sizeof(capi.KhInflationParams) == 32
    for name, struct, want_size in (("kh_map_travel_params", capi.KhMapTravelParams, 64), ("kh_map_travel_stats", capi.KhMapTravelStats, 104),
                                    ("kh_travel_path", capi.KhTravelPath, 16)):
        want, size = _header_layout(name, ints)
        assert _layout(struct) == want, name
        assert C.sizeof(struct) == size == want_size, name
    assert capi.KhMapTravelParams.inflation.offset == 8 and capi.KhMapTravelParams.connectivity.offset == 40 and capi.KhMapTravelParams.goal_snap_cells.offset == 56
    assert capi.KhMapTravelStats.n_traversable.offset == 32 and capi.KhMapTravelStats.max_value.offset == 48 and capi.KhMapTravelStats.tile_runs.offset == 64
    assert capi.KhMapTravelStats.times_ms.offset == 72
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    assert int(re.search(r"#define KH_TRAVEL_FAR (0x[0-9A-Fa-f]+)u", header).group(1), 16) == capi.KH_TRAVEL_FAR == rule.FAR
    for names in (("KH_TRAVEL_GOAL_OK", "KH_TRAVEL_GOAL_BLOCKED", "KH_TRAVEL_GOAL_OUTSIDE"), ("KH_TRAVEL_AT_OK", "KH_TRAVEL_AT_UNREACHED", "KH_TRAVEL_AT_OUTSIDE"),
                  ("KH_TRAVEL_PATH_OK", "KH_TRAVEL_PATH_TRUNCATED", "KH_TRAVEL_PATH_UNREACHED", "KH_TRAVEL_PATH_OUTSIDE")):
        for k, name in enumerate(names):
            assert int(re.search(name + r" = (\d+)", header).group(1)) == getattr(capi, name) == k, name
    assert (rule.GOAL_OK, rule.GOAL_BLOCKED, rule.GOAL_OUTSIDE) == (0, 1, 2) and (rule.AT_OK, rule.AT_UNREACHED, rule.AT_OUTSIDE) == (0, 1, 2)
    assert (rule.PATH_OK, rule.PATH_TRUNCATED, rule.PATH_UNREACHED, rule.PATH_OUTSIDE) == (0, 1, 2, 3)


def test_defaults(kartohip_lib):
    p = capi.KhMapTravelParams(7.0, capi.KhInflationParams(1.0, 2.0, 3.0, 0, 1), 1, 2, 3, 4, 5, 9)
    kartohip_lib.kh_map_travel_params_default(C.byref(p))
    assert {k: getattr(p, k) for k in rule.PARAMS} == rule.PARAMS and p.pad == 0
    assert {k: getattr(p.inflation, k) for k in fr.INFLATION} == fr.INFLATION
    assert (p.min_clearance, p.connectivity, p.cut_corners, p.neutral_cost, p.cost_weight, p.goal_snap_cells) == (0.0, 8, 0, 50, 13, 0)
    kartohip_lib.kh_map_travel_params_default(None)            # a NULL output is ignored


def test_arguments_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD     # a NULL handle is looked at after the device
    p, h = capi.KhMapTravelParams(), C.c_void_p(1)
    L.kh_map_travel_params_default(C.byref(p))
    assert L.kh_map_travel_create(None, C.byref(p), None) == BAD
    assert L.kh_map_travel_create(None, C.byref(p), C.byref(h)) == BAD and h.value is None, "a refused create leaves NULL"
    h.value = 1
    assert L.kh_map_travel_create(None, None, C.byref(h)) == BAD and h.value is None
    L.kh_map_travel_destroy(None)
    assert L.kh_map_travel_recompute(None, None) == BAD
    st = capi.KhMapTravelStats()
    assert L.kh_map_travel_stats_get(None, None) == BAD and L.kh_map_travel_stats_get(None, C.byref(st)) == after
    xy = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    status = (C.c_int32 * 2)()
    assert L.kh_map_travel_solve(None, 0, xy, status) == BAD and L.kh_map_travel_solve(None, -1, xy, status) == BAD
    assert L.kh_map_travel_solve(None, 2, None, status) == BAD
    many = (C.c_double * (2 * 4097))()
    assert L.kh_map_travel_solve(None, 4097, many, None) == BAD and L.kh_map_travel_solve(None, 4096, many, None) == after
    assert L.kh_map_travel_solve(None, 2, xy, None) == after and L.kh_map_travel_solve(None, 2, xy, status) == after
    assert L.kh_map_travel_read(None, None, None) == after
    assert L.kh_map_travel_lookup(None, 0, xy, 0, None, None, None) == BAD and L.kh_map_travel_lookup(None, 2, None, 0, None, None, None) == BAD
    assert L.kh_map_travel_lookup(None, 2, xy, -1, None, None, None) == BAD and L.kh_map_travel_lookup(None, 2, xy, 17, None, None, None) == BAD
    assert L.kh_map_travel_lookup(None, 2, xy, 16, None, None, None) == after
    heads = (capi.KhTravelPath * 2)()
    assert L.kh_map_travel_paths(None, 0, xy, 0, 8, heads, None) == BAD and L.kh_map_travel_paths(None, 2, None, 0, 8, heads, None) == BAD
    assert L.kh_map_travel_paths(None, 2, xy, 17, 8, heads, None) == BAD and L.kh_map_travel_paths(None, 2, xy, 0, 8, None, None) == BAD
    assert L.kh_map_travel_paths(None, 2, xy, 0, 0, heads, None) == BAD and L.kh_map_travel_paths(None, 2, xy, 0, 65537, heads, None) == BAD
    assert L.kh_map_travel_paths(None, 2, xy, 0, 65536, heads, None) == after and L.kh_map_travel_paths(None, 1, xy, 0, 1, heads, None) == after
    big = (C.c_double * (2 * 257))()
    assert L.kh_map_travel_paths(None, 257, big, 0, 65536, heads, None) == BAD, "n * max_cells above 2^24"
    for call in (lambda b: L.kh_map_travel_solve(None, 2, b, None), lambda b: L.kh_map_travel_lookup(None, 2, b, 0, None, None, None),
                 lambda b: L.kh_map_travel_paths(None, 2, b, 0, 8, heads, None)):
        for k, value in ((0, math.nan), (3, math.inf), (2, -math.inf)):
            bad = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
            bad[k] = value
            assert call(bad) == BAD, (k, value)
    assert L.kh_map_travel_set_rounds_per_check(None, -1) == BAD and L.kh_map_travel_set_rounds_per_check(None, 65) == BAD
    assert L.kh_map_travel_set_rounds_per_check(None, 0) == after and L.kh_map_travel_set_rounds_per_check(None, 64) == after
