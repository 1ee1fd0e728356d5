"""GPU: kh_map_seeds (k_map_seeds in csrc/occupancy_map.hip) against tests/map_localize_rule.py on the hand-made views of
tests/map_localize_cases.py, uploaded through kh_device_upload, and on the views the library itself hands out (kh_occupancy_view,
kh_live_map_view after a growth).  Cells and world points are compared exactly."""
import ctypes as C
import math

import numpy as np
import pytest

import map_localize_cases as cases
import map_localize_rule as rule
import map_match_rule as mr
from common import bits
from slam_toolbox_amd import capi, synth
from slam_toolbox_amd.map_localizer import map_seeds

pytestmark = pytest.mark.gpu

SEED_CASES = cases.seed_cases()


class DeviceView:
    """a view dict's cells in device memory of the caller's own, as a capi.KhMapView (`.v`)"""

    def __init__(self, view, device=0):
        L = capi.lib()
        cells = np.ascontiguousarray(view["cells"])
        self.buf = C.c_void_p()
        capi.check(L.kh_device_malloc(device, cells.size, C.byref(self.buf)), "kh_device_malloc")
        capi.check(L.kh_device_upload(self.buf, cells.ctypes.data, cells.size), "kh_device_upload")
        self.size = cells.size
        v = capi.KhMapView()
        v.device_cells, v.device, v.width, v.height, v.width_step = self.buf.value, device, view["width"], view["height"], cells.shape[1]
        v.ox, v.oy, v.anchor[0], v.anchor[1], v.scale = view["ox"], view["oy"], view["anchor"][0], view["anchor"][1], view["scale"]
        self.v = v

    def upload(self, view):
        """another view dict's cells into the same memory (the same window and stride)"""
        cells = np.ascontiguousarray(view["cells"])
        assert cells.size == self.size
        capi.check(capi.lib().kh_device_upload(self.buf, cells.ctypes.data, cells.size), "kh_device_upload")

    def download(self):
        out = np.zeros(self.size, dtype=np.uint8)
        capi.check(capi.lib().kh_device_download(out.ctypes.data, self.buf, self.size), "kh_device_download")
        return out

    def close(self):
        if self.buf:
            capi.lib().kh_device_free(self.buf)
            self.buf = C.c_void_p()


def same_seeds(got, want):
    assert np.array_equal(got[0], want[0]), (got[0].tolist(), want[0].tolist())
    assert np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("case", SEED_CASES, ids=[c.name for c in SEED_CASES])
def test_seed_cases(kartohip_lib, case):
    d = DeviceView(case.view)
    got = map_seeds(d.v, case.spacing, case.center, case.radius)
    want = rule.seeds(case.view, case.spacing, case.center, case.radius)
    same_seeds(got, want)
    case.check(got[0].astype(np.int64), got[1])
    assert np.array_equal(d.download(), case.view["cells"].ravel()), "the view's cells were written"
    d.close()


def test_cap_and_total(kartohip_lib):
    case = next(c for c in SEED_CASES if c.name.startswith("negative origin"))
    want_cells, want_xy = rule.seeds(case.view, case.spacing)
    d = DeviceView(case.view)
    L = kartohip_lib
    for cap in (0, 1, 5, 16, 40):
        cells, xy, n = np.full((40, 2), -7, dtype=np.int32), np.full((40, 2), -7.0), C.c_int32()
        capi.check(L.kh_map_seeds(C.byref(d.v), case.spacing, None, 0.0, cells.ctypes.data, xy.ctypes.data, cap, C.byref(n)), "kh_map_seeds")
        assert n.value == 16, "the total, also beyond cap"
        k = min(cap, 16)
        assert np.array_equal(cells[:k], want_cells[:k]) and np.array_equal(xy[:k], want_xy[:k])
        assert (cells[k:] == -7).all() and (xy[k:] == -7.0).all(), "nothing is written beyond cap"
    n = C.c_int32()
    capi.check(L.kh_map_seeds(C.byref(d.v), case.spacing, None, 0.0, None, None, 16, C.byref(n)), "kh_map_seeds")      # either output may be NULL
    assert n.value == 16
    assert L.kh_map_seeds(C.byref(d.v), 4096.6 / case.view["scale"], None, 0.0, None, None, 0, C.byref(n)) == capi.KH_ERR_INVALID_ARG
    w = capi.KhMapView.from_buffer_copy(d.v)
    w.device = 1 << 20
    assert L.kh_map_seeds(C.byref(w), case.spacing, None, 0.0, None, None, 0, C.byref(n)) == capi.KH_ERR_NO_DEVICE
    d.close()


def test_occupancy_view(kartohip_lib):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    rng = np.random.default_rng(31)
    nav = rng.choice(np.array([-1, 100, 0], dtype=np.int8), size=(90, 131), p=[0.5, 0.1, 0.4])
    g = OccupancyGrid.from_nav(nav, (-3.2, 1.7), 0.05)
    view = mr.view_dict(g.cells(), (-3.2, 1.7), g.view().scale, 0, 0, 131)
    for spacing, center, radius in ((1.05, None, 0.0), (0.55, (0.0, 4.0), 1.5)):
        same_seeds(map_seeds(g, spacing, center, radius), rule.seeds(view, spacing, center, radius))
    assert len(map_seeds(g, 1.05)[0]) == 7 * 5
    g.close()


def test_live_map_view_after_growth(kartohip_lib):
    """the blocks are floor quotients of the lattice index: a seed block stays where it is when the window grows to the lower left"""
    from test_live_map_edges_gpu import _place, _synthetic, placing_mapper
    laser = synth.Laser()
    poses, ranges = _synthetic(6, 3)
    poses[:3, :2] = [(26.0, 24.0), (26.5, 24.5), (27.0, 24.2)]
    poses[3:, :2] = [(10.0, 10.0), (10.5, 10.2), (11.0, 10.1)]
    m = placing_mapper(laser)
    live = m.live_map(0.05, np.array([16.0, 16.0]), math.inf)     # an anchor inside the map: negative lattice cells after the growth
    for k in range(3):
        _place(m, ranges[k], poses[k], k)
    live.update()
    first = live.info()
    spacing = 1.55
    view = mr.view_dict(live.cells(), (16.0, 16.0), live.view().scale, first["ox"], first["oy"], first["width"])
    before = map_seeds(live, spacing)
    same_seeds(before, rule.seeds(view, spacing))
    for k in range(3, 6):
        _place(m, ranges[k], poses[k], k)
    assert live.update()["relayouts"] == 1, "the window did not grow"
    info = live.info()
    assert info["ox"] < first["ox"] and info["oy"] < first["oy"] and info["ox"] < 0
    view = mr.view_dict(live.cells(), (16.0, 16.0), live.view().scale, info["ox"], info["oy"], info["width"])
    after = map_seeds(live, spacing)
    same_seeds(after, rule.seeds(view, spacing))
    p = rule.pitch_of(spacing, view["scale"])
    blocks = lambda c: {(int(i) // p, int(j) // p) for i, j in c}      # noqa: E731
    assert blocks(before[0]) <= blocks(after[0]) and len(after[0]) > len(before[0]) > 0
    live.close(); m.close()
