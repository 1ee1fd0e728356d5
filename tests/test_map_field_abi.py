"""CPU: the ABI of the distance field -- the new names in include/karto_hip.h, in capi.SYMBOLS and exported with prototypes, the layout
of the new structs, the codes, the defaults, the host-only cost table, and the argument checks that come before a device is looked
for (then KH_ERR_NO_DEVICE on a machine without one)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import map_field_rule as rule
from slam_toolbox_amd import capi
from test_map_localize_abi import MALFORMED, _header_layout, _laser, _layout, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_map_field_params_default", "kh_map_field_create", "kh_map_field_destroy", "kh_map_field_stats_get", "kh_map_field_read",
         "kh_inflation_params_default", "kh_inflation_table", "kh_map_field_costs", "kh_map_field_clearance", "kh_map_field_score",
         "kh_field_refine_params_default", "kh_map_field_refine"]
BAD, NO_DEVICE = capi.KH_ERR_INVALID_ARG, capi.KH_ERR_NO_DEVICE


def test_names_are_declared_bound_and_exported(kartohip_lib):
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    for name in NAMES:
        assert re.search(r"KH_API \w+ " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"
    sources = __import__("slam_toolbox_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "map_field.cpp" in sources and "occupancy_field.hip" in sources


def test_layouts_and_codes_match_the_header():
    ints = {"uint64_t": (8, 8), "uint32_t": (4, 4)}
    for name, struct, want_size in (("kh_map_field_params", capi.KhMapFieldParams, 16), ("kh_map_field_stats", capi.KhMapFieldStats, 64),
                                    ("kh_inflation_params", capi.KhInflationParams, 32), ("kh_field_score", capi.KhFieldScore, 40),
                                    ("kh_field_refine_params", capi.KhFieldRefineParams, 32), ("kh_field_refined", capi.KhFieldRefined, 56)):
        want, size = _header_layout(name, ints)
        assert _layout(struct) == want, name
        assert C.sizeof(struct) == size == want_size, name
    assert capi.KhMapFieldStats.max_d2.offset == 20 and capi.KhMapFieldStats.n_obstacles.offset == 24 and capi.KhMapFieldStats.times_ms.offset == 40
    assert capi.KhFieldScore.sum_d2.offset == 16 and capi.KhFieldScore.score.offset == 32
    assert capi.KhFieldRefined.cost_start.offset == 24 and capi.KhFieldRefined.status.offset == 52
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    assert int(re.search(r"#define KH_FIELD_FAR (0x[0-9A-Fa-f]+)u", header).group(1), 16) == capi.KH_FIELD_FAR == rule.FAR
    for prefix, names in (("KH_FIELD_OBSTACLE_", ("OCCUPIED", "NOT_FREE")), ("KH_CLEAR_", ("OK", "FAR", "OUTSIDE")),
                          ("KH_REFINE_", ("CONVERGED", "MAX_ROUNDS", "LEFT_LATTICE"))):
        for k, name in enumerate(names):
            assert int(re.search(prefix + name + r" = (\d+)", header).group(1)) == getattr(capi, prefix + name) == k, name


def test_defaults(kartohip_lib):
    L = kartohip_lib
    p = capi.KhMapFieldParams(7.0, 1, 9)
    L.kh_map_field_params_default(C.byref(p))
    assert (p.max_distance, p.obstacles, p.pad) == (2.0, capi.KH_FIELD_OBSTACLE_OCCUPIED, 0)
    q = capi.KhInflationParams(1.0, 2.0, 3.0, 0, 1)
    L.kh_inflation_params_default(C.byref(q))
    assert {k: getattr(q, k) for k, _ in capi.KhInflationParams._fields_} == rule.INFLATION
    r = capi.KhFieldRefineParams(1.0, 1.0, 1, 1, 1, 1)
    L.kh_field_refine_params_default(C.byref(r), 20.0)
    assert (r.step_xy, r.step_heading, r.n_halvings, r.max_rounds, r.truncate_cells, r.pad) == (2.0 / 20.0, 0.02, 4, 64, 0, 0)
    assert dict(rule.REFINE, step_xy=0.1) == {k: getattr(r, k) for k, _ in capi.KhFieldRefineParams._fields_ if k != "pad"}
    L.kh_map_field_params_default(None); L.kh_inflation_params_default(None); L.kh_field_refine_params_default(None, 20.0)      # NULL outputs are ignored


def test_inflation_table_is_the_rule_s(kartohip_lib):
    """host only: it answers on a machine without a device"""
    from slam_toolbox_amd.map_field import inflation_table
    from test_map_field_plan import BAD_TABLES, TABLES
    for kw in TABLES:
        assert np.array_equal(inflation_table(**kw), rule.cost_table(**kw)), kw
    for kw in BAD_TABLES:
        with pytest.raises(capi.KartoHipError) as e:
            inflation_table(**kw)
        assert e.value.code == BAD, kw
    L = kartohip_lib
    p, n, buf = capi.KhInflationParams(), C.c_int32(-1), (C.c_uint8 * 200)()
    L.kh_inflation_params_default(C.byref(p))
    assert L.kh_inflation_table(C.byref(p), 20.0, None, 0, C.byref(n)) == capi.KH_OK and n.value == 122
    assert L.kh_inflation_table(C.byref(p), 20.0, buf, 121, C.byref(n)) == BAD and n.value == 122, "a table too small is refused, its size still told"
    assert L.kh_inflation_table(C.byref(p), 20.0, buf, 200, C.byref(n)) == capi.KH_OK and list(buf[:122]) == rule.cost_table(20.0).tolist() and buf[122] == 0
    assert L.kh_inflation_table(None, 20.0, buf, 200, C.byref(n)) == BAD and L.kh_inflation_table(C.byref(p), 20.0, buf, 200, None) == BAD
    assert L.kh_inflation_table(C.byref(p), 20.0, None, 200, C.byref(n)) == BAD and L.kh_inflation_table(C.byref(p), 20.0, buf, -1, C.byref(n)) == BAD


def test_create_arguments(kartohip_lib):
    L = kartohip_lib
    v, p, h = _view(), capi.KhMapFieldParams(), C.c_void_p(1)
    L.kh_map_field_params_default(C.byref(p))
    call = lambda **kw: L.kh_map_field_create(kw.get("view", C.byref(v)), kw.get("params", C.byref(p)), kw.get("out", C.byref(h)))  # noqa: E731
    for kw in (dict(view=None), dict(params=None)):
        h.value = 1
        assert call(**kw) == BAD, kw
        assert h.value is None, "a refused create leaves NULL"
    assert call(out=None) == BAD
    for field, value in MALFORMED:
        w = capi.KhMapView.from_buffer_copy(v)
        setattr(w, field, value)
        assert call(view=C.byref(w)) == BAD, field
    for field, value in (("max_distance", math.nan), ("max_distance", math.inf), ("max_distance", -0.5), ("max_distance", 51.3), ("obstacles", -1), ("obstacles", 2)):
        q = capi.KhMapFieldParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert call(params=C.byref(q)) == BAD, (field, value)
    uncapped = capi.KhMapFieldParams(0.0, 0, 0)
    for width, height, params in ((32769, 1, p), (1, 32769, p), (32768, 8193, p), (4097, 8, uncapped), (8, 4097, uncapped)):
        w = capi.KhMapView.from_buffer_copy(v)
        w.width, w.height, w.width_step = width, height, width
        assert call(view=C.byref(w), params=C.byref(params)) == BAD, (width, height)
    if L.kh_device_count() == 0:
        assert call() == NO_DEVICE and h.value is None
        w = capi.KhMapView.from_buffer_copy(v)
        w.width, w.height, w.width_step = 4096, 4096, 4096
        assert call(view=C.byref(w), params=C.byref(uncapped)) == NO_DEVICE
        w.width, w.height, w.width_step = 32768, 8192, 32768
        assert call(view=C.byref(w)) == NO_DEVICE
        assert call(params=C.byref(capi.KhMapFieldParams(51.2, 1, 0))) == NO_DEVICE


def test_handle_calls(kartohip_lib):
    L = kartohip_lib
    after = NO_DEVICE if L.kh_device_count() == 0 else BAD     # a NULL handle is looked at after the device
    L.kh_map_field_destroy(None)
    st = capi.KhMapFieldStats()
    assert L.kh_map_field_stats_get(None, None) == BAD and L.kh_map_field_stats_get(None, C.byref(st)) == after
    assert L.kh_map_field_read(None, None, None) == after
    # costs
    p, out = capi.KhInflationParams(), (C.c_uint8 * 4)()
    L.kh_inflation_params_default(C.byref(p))
    assert L.kh_map_field_costs(None, None, out) == BAD and L.kh_map_field_costs(None, C.byref(p), None) == BAD
    for field, value in (("inscribed_radius", 0.6), ("inscribed_radius", -1.0), ("inflation_radius", math.nan), ("inflation_radius", math.inf),
                         ("cost_scaling_factor", -1.0), ("cost_scaling_factor", math.nan), ("track_unknown", 2), ("inflate_unknown", -1)):
        q = capi.KhInflationParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert L.kh_map_field_costs(None, C.byref(q), out) == BAD, (field, value)
    assert L.kh_map_field_costs(None, C.byref(p), out) == after
    # clearance
    xy = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    assert L.kh_map_field_clearance(None, 0, xy, None, None, None) == BAD and L.kh_map_field_clearance(None, 2, None, None, None, None) == BAD
    for k, value in ((0, math.nan), (3, math.inf), (2, -math.inf)):
        bad = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
        bad[k] = value
        assert L.kh_map_field_clearance(None, 2, bad, None, None, None) == BAD, (k, value)
    assert L.kh_map_field_clearance(None, 2, xy, None, None, None) == after
    # score and refinement
    laser, ranges, poses = _laser(), (C.c_double * 8)(*([2.0] * 8)), (C.c_double * 3)(0.0, 0.0, 0.0)
    score, refined = (capi.KhFieldScore * 1)(), (capi.KhFieldRefined * 1)()
    sc = lambda **kw: L.kh_map_field_score(None, kw.get("laser", C.byref(laser)), kw.get("ranges", ranges), kw.get("n", 1), kw.get("poses", poses),  # noqa: E731
                                           kw.get("t", 0), kw.get("out", score))
    none = capi.KhLaser.from_buffer_copy(laser)
    none.n_beams = 0
    for kw in (dict(laser=None), dict(ranges=None), dict(poses=None), dict(out=None), dict(n=0), dict(t=-1), dict(t=1025), dict(laser=C.byref(none))):
        assert sc(**kw) == BAD, kw
    assert sc() == after and sc(t=1024) == after
    rp = capi.KhFieldRefineParams()
    L.kh_field_refine_params_default(C.byref(rp), 20.0)
    rf = lambda **kw: L.kh_map_field_refine(None, kw.get("laser", C.byref(laser)), kw.get("ranges", ranges), kw.get("n", 1), kw.get("poses", poses),  # noqa: E731
                                            kw.get("params", C.byref(rp)), kw.get("out", refined), None)
    for kw in (dict(laser=None), dict(ranges=None), dict(poses=None), dict(out=None), dict(n=0), dict(params=None)):
        assert rf(**kw) == BAD, kw
    for field, value in (("step_xy", 0.0), ("step_xy", math.nan), ("step_heading", -1.0), ("step_heading", math.inf), ("n_halvings", -1), ("n_halvings", 33),
                         ("max_rounds", 0), ("max_rounds", 4097), ("truncate_cells", -1), ("truncate_cells", 1025)):
        q = capi.KhFieldRefineParams.from_buffer_copy(rp)
        setattr(q, field, value)
        assert rf(params=C.byref(q)) == BAD, (field, value)
    assert rf() == after
