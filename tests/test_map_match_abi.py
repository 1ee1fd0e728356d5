"""CPU: the ABI of the map entry points -- kh_map_view's layout as include/karto_hip.h declares it, the new names bound with
prototypes, and the argument checks that need no device."""
import ctypes as C
import os
import re

import numpy as np

from slam_toolbox_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_occupancy_view", "kh_occupancy_write_nav", "kh_live_map_view", "kh_matcher_add_map", "kh_matcher_match_map",
         "kh_matcher_match_map_batch"]


def test_names_are_bound(kartohip_lib):
    for name in NAMES:
        assert name in capi.SYMBOLS
        assert getattr(kartohip_lib, name).argtypes, f"{name} has no prototype"


def test_view_layout_matches_the_header():
    header = open(os.path.join(ROOT, "include", "karto_hip.h")).read()
    body = re.search(r"typedef struct kh_map_view \{(.*?)\} kh_map_view;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"const uint8_t *": 8, "int32_t": 4, "double": 8}
    want, at = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype = next(t for t in sizes if decl.startswith(t))
        for name in decl[len(ctype):].split(","):
            name = name.strip()
            count = 1
            m = re.match(r"(\w+)\[(\d+)\]", name)
            if m:
                name, count = m.group(1), int(m.group(2))
            at = (at + sizes[ctype] - 1) // sizes[ctype] * sizes[ctype]
            want.append((name, at, sizes[ctype] * count))
            at += sizes[ctype] * count
    got = [(name, getattr(capi.KhMapView, name).offset, getattr(capi.KhMapView, name).size) for name, _ in capi.KhMapView._fields_]
    assert got == want
    assert [n for n, _, _ in want] == ["device_cells", "device", "width", "height", "width_step", "ox", "oy", "anchor", "scale"]
    assert C.sizeof(capi.KhMapView) == 56 and capi.KhMapView.anchor.offset == 32 and capi.KhMapView.scale.offset == 48


def test_null_arguments_are_refused_without_a_device(kartohip_lib):
    L = kartohip_lib
    v = capi.KhMapView()
    scan = capi.KhScan()
    mean, cov, resp, status = np.zeros(3), np.zeros(9), C.c_double(), np.zeros(1, dtype=np.int32)
    bad = capi.KH_ERR_INVALID_ARG
    assert L.kh_occupancy_view(None, C.byref(v)) == bad
    assert L.kh_occupancy_write_nav(None, None) == bad
    assert L.kh_live_map_view(None, C.byref(v)) == bad
    assert L.kh_matcher_add_map(None, 0, C.byref(scan), C.byref(v)) == bad
    assert L.kh_matcher_add_map(None, 0, C.byref(scan), None) == bad
    assert L.kh_matcher_match_map(None, C.byref(scan), C.byref(v), 1, 1, mean, cov, C.byref(resp)) == bad
    assert L.kh_matcher_match_map(None, C.byref(scan), None, 1, 1, mean, cov, C.byref(resp)) == bad
    assert L.kh_matcher_match_map_batch(None, 1, C.byref(scan), C.byref(v), 1, 1, mean, cov, np.zeros(1), status) == bad
    assert L.kh_matcher_match_map_batch(None, 1, C.byref(scan), None, 1, 1, mean, cov, np.zeros(1), status) == bad
