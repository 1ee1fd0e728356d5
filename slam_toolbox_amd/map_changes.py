"""The map change layer over the C ABI (kh_map_changes_*; include/karto_hip.h): where the scans of a robot that
holds only a map contradict that map, and the map with what was observed laid over it.

    layer = MapChanges(grid)                                # an OccupancyGrid, a LiveMap or a capi.KhMapView
    labels = layer.observe(laser, ranges, sensor_pose)      # per beam: (class, blocked); capi.KH_BEAM_*
    d = layer.diff()                                        # per cell: codes, counts, the changed cells; capi.KH_CELL_*
    localizer.set_map(layer.view())                         # the patched map, on the device
    nav = layer.nav()                                       # ... and as nav_msgs/OccupancyGrid values

Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .map_localizer import _laser_of, _view_of

COUNTS = ("n_unobserved", "n_confirmed", "n_appeared", "n_vanished", "n_discovered_occupied", "n_discovered_free")


def _as_laser(laser):
    return laser if isinstance(laser, capi.KhLaser) else _laser_of(laser)


class MapChanges:
    def __init__(self, source):
        """kh_map_changes_create.  The view is borrowed and the window fixed: keep the source alive and as it is (the layer holds a
        reference to what it was given)."""
        v = _view_of(source)
        self._source = source
        self.width, self.height, self.width_step = v.width, v.height, v.width_step
        self._h = C.c_void_p()
        capi.check(capi.lib().kh_map_changes_create(C.byref(v), C.byref(self._h)), "kh_map_changes_create")

    def observe(self, laser, ranges, sensor_poses, end_tolerance: int = 1):
        """kh_map_changes_observe: one scan (ranges (n_beams,), a pose (3,)) or several ((n, n_beams), (n, 3)).
        -> labels int32 (n_beams, 2) or (n, n_beams, 2): the KH_BEAM_ class and `blocked` of every beam"""
        L = _as_laser(laser)
        poses = np.ascontiguousarray(sensor_poses, dtype=np.float64)
        single = poses.ndim == 1
        poses = poses.reshape(-1, 3)
        ranges = np.ascontiguousarray(ranges, dtype=np.float64).reshape(-1, L.n_beams)
        assert ranges.shape[0] == poses.shape[0], "one pose per scan"
        labels = np.zeros((poses.shape[0], L.n_beams, 2), dtype=np.int32)
        capi.check(capi.lib().kh_map_changes_observe(self._h, C.byref(L), poses.shape[0], ranges.ctypes.data, poses.ctypes.data,
                                                     int(end_tolerance), labels.ctypes.data), "kh_map_changes_observe")
        return labels[0] if single else labels

    def diff(self, min_pass_through: int = 2, occupancy_threshold: float = 0.1, cap=None) -> dict:
        """kh_map_changes_diff -> the summary's fields, `counts` (the six counts by code) and `cells` (n_listed, 3) int32: lattice i,
        lattice j, code of the changed cells in row-major order.  cap None: all of them (a second call where the first guess of 65536
        was short)."""
        room = min(self.width * self.height, 65536) if cap is None else int(cap)
        while True:
            cells = np.zeros((max(1, room), 3), dtype=np.int32)
            s = capi.KhMapChangesSummary()
            capi.check(capi.lib().kh_map_changes_diff(self._h, int(min_pass_through), float(occupancy_threshold), cells.ctypes.data, room,
                                                      C.byref(s)), "kh_map_changes_diff")
            if cap is not None or s.n_changed <= room:
                break
            room = int(s.n_changed)
        out = {k: getattr(s, k) for k, _ in capi.KhMapChangesSummary._fields_}
        out["counts"] = np.array([getattr(s, k) for k in COUNTS], dtype=np.int64)
        out["cells"] = cells[:s.n_listed].copy()
        return out

    def decay(self, shift: int = 1):
        capi.check(capi.lib().kh_map_changes_decay(self._h, int(shift)), "kh_map_changes_decay")

    def clear(self):
        capi.check(capi.lib().kh_map_changes_clear(self._h), "kh_map_changes_clear")

    def read(self) -> dict:
        """kh_map_changes_read: pass, hits (uint32), codes, patched (uint8), each (height, width_step)"""
        shape = (self.height, self.width_step)
        out = dict(passes=np.zeros(shape, dtype=np.uint32), hits=np.zeros(shape, dtype=np.uint32), codes=np.zeros(shape, dtype=np.uint8),
                   patched=np.zeros(shape, dtype=np.uint8))
        capi.check(capi.lib().kh_map_changes_read(self._h, out["passes"].ctypes.data, out["hits"].ctypes.data, out["codes"].ctypes.data,
                                                  out["patched"].ctypes.data), "kh_map_changes_read")
        return out

    def view(self) -> capi.KhMapView:
        """kh_map_changes_view: the patched cells of the last diff, borrowed until the next diff or close"""
        v = capi.KhMapView()
        capi.check(capi.lib().kh_map_changes_view(self._h, C.byref(v)), "kh_map_changes_view")
        return v

    def nav(self):
        """kh_map_changes_read_nav: the patched cells as (height, width) int8 nav values"""
        out = np.zeros((self.height, self.width), dtype=np.int8)
        capi.check(capi.lib().kh_map_changes_read_nav(self._h, out.ctypes.data), "kh_map_changes_read_nav")
        return out

    def close(self):
        if self._h:
            capi.lib().kh_map_changes_destroy(self._h)
            self._h = C.c_void_p()
        self._source = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
