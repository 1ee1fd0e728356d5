"""CPU: the ABI of a field that follows its map -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes,
the layout of kh_field_update, and the argument checks that come before a device is looked for (then KH_ERR_NO_DEVICE on a machine
without one).  The lattice test needs a handle, which needs a device: its order is tests/test_map_field_update_plan.py's."""
import ctypes as C
import math
import os
import re

from slam_toolbox_amd import capi
from test_map_localize_abi import MALFORMED, _header_layout, _layout, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_field_update", "kh_map_field_set_band_rows", "kh_map_field_read_rect", "kh_map_field_costs_rect", "kh_live_map_field_create",
         "kh_live_map_field_sync"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    sources = __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "occupancy_field_update.hip" in sources
    assert os.path.exists(os.path.join(ROOT, "slam_toolbox_amd", "csrc", "map_field_update_plan.hpp"))


def test_layout_matches_the_header():
    want, size = _header_layout("kh_field_update", {})
    assert _layout(capi.KhFieldUpdate) == want
    assert C.sizeof(capi.KhFieldUpdate) == size == 88
    assert capi.KhFieldUpdate.values_box.offset == 16 and capi.KhFieldUpdate.rebuilt.offset == 32 and capi.KhFieldUpdate.cells_compared.offset == 40
    assert capi.KhFieldUpdate.times_ms.offset == 56


def test_update_arguments(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD     # a NULL handle is looked at after the device
    v, u = _view(), capi.KhFieldUpdate()
    u.rebuilt, u.cells_compared = 7, 7
    assert L.kh_map_field_update(None, None, None, C.byref(u)) == BAD
    assert (u.rebuilt, u.cells_compared) == (0, 0), "a refused update leaves zeros"
    for field, value in MALFORMED:
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        assert L.kh_map_field_update(None, C.byref(w), None, C.byref(u)) == BAD, field
    rect = (C.c_int32 * 4)(0, 0, 5, 5)
    assert L.kh_map_field_update(None, C.byref(v), None, None) == after
    assert L.kh_map_field_update(None, C.byref(v), rect, C.byref(u)) == after
    assert L.kh_map_field_set_band_rows(None, -1) == BAD and L.kh_map_field_set_band_rows(None, 0) == after and L.kh_map_field_set_band_rows(None, 5) == after


def test_rect_reader_arguments(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD
    values, costs = (C.c_uint32 * 4)(), (C.c_uint8 * 4)()
    assert L.kh_map_field_read_rect(None, 0, 0, 2, 2, None) == BAD
    for w, h in ((0, 2), (2, 0), (-1, 2), (2, -2)):
        assert L.kh_map_field_read_rect(None, 0, 0, w, h, values) == BAD, (w, h)
    assert L.kh_map_field_read_rect(None, 0, 0, 2, 2, values) == after
    p = capi.KhInflationParams()
    L.kh_inflation_params_default(C.byref(p))
    assert L.kh_map_field_costs_rect(None, None, 0, 0, 2, 2, costs) == BAD and L.kh_map_field_costs_rect(None, C.byref(p), 0, 0, 2, 2, None) == BAD
    for w, h in ((0, 2), (2, 0), (-1, 2), (2, -2)):
        assert L.kh_map_field_costs_rect(None, C.byref(p), 0, 0, w, h, costs) == BAD, (w, h)
    for field, value in (("inscribed_radius", 0.6), ("inscribed_radius", -1.0), ("inflation_radius", math.nan), ("inflation_radius", math.inf),
                         ("cost_scaling_factor", -1.0), ("cost_scaling_factor", math.nan), ("track_unknown", 2), ("inflate_unknown", -1)):
        q = capi.KhInflationParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert L.kh_map_field_costs_rect(None, C.byref(q), 0, 0, 2, 2, costs) == BAD, (field, value)
    assert L.kh_map_field_costs_rect(None, C.byref(p), 0, 0, 2, 2, costs) == after


def test_live_binding_arguments(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD
    p, h, u = capi.KhMapFieldParams(), C.c_void_p(1), capi.KhFieldUpdate()
    L.kh_map_field_params_default(C.byref(p))
    assert L.kh_live_map_field_create(None, C.byref(p), None) == BAD
    assert L.kh_live_map_field_create(None, None, C.byref(h)) == BAD and h.value is None, "a refused create leaves NULL"
    h.value = 1
    assert L.kh_live_map_field_create(None, C.byref(p), C.byref(h)) == after and h.value is None
    u.relayout = 3
    assert L.kh_live_map_field_sync(None, C.byref(u)) == after and u.relayout == 0
    assert L.kh_live_map_field_sync(None, None) == after
