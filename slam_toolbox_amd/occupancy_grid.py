"""Python mirror of karto::OccupancyGrid (Karto.h:5880-6330) over the C ABI (kh_occupancy_*): same method
names and argument meaning as the reference -- CreateFromScans(scans, resolution), GetWidth/GetHeight,
cell states 0 unknown / 100 occupied / 255 free."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .scan_matcher import _scan_array

GridStates_Unknown, GridStates_Occupied, GridStates_Free = 0, 100, 255      # Karto.h:4379-4381


def compute_dimensions(scans, min_range, range_threshold, resolution):
    """OccupancyGrid::ComputeDimensions (Karto.h:6086-6112) -> (width, height, offset (2,))."""
    w, h = C.c_int32(), C.c_int32()
    off = np.zeros(2)
    capi.check(capi.lib().kh_occupancy_compute_dimensions(len(scans), _scan_array(scans), float(min_range),
                                                          float(range_threshold), float(resolution), C.byref(w),
                                                          C.byref(h), off), "kh_occupancy_compute_dimensions")
    return w.value, h.value, off


class OccupancyGrid:
    def __init__(self, width, height, offset, resolution, device: int = 0):
        h = C.c_void_p()
        capi.check(capi.lib().kh_occupancy_create(int(width), int(height), float(offset[0]), float(offset[1]),
                                                  float(resolution), device, C.byref(h)), "kh_occupancy_create")
        self._h = h
        self.width, self.height, self.width_step = int(width), int(height), (int(width) + 7) & ~7
        self.offset = np.asarray(offset, dtype=np.float64).copy()
        self.resolution = float(resolution)

    @classmethod
    def from_handle(cls, handle, resolution):
        """wraps a kh_occupancy the library made (kh_mapper_build_map); the grid owns it from here on"""
        g = cls.__new__(cls)
        g._h = handle
        w, h, ws = C.c_int32(), C.c_int32(), C.c_int32()
        capi.check(capi.lib().kh_occupancy_info(handle, C.byref(w), C.byref(h), C.byref(ws), None, None), "kh_occupancy_info")
        g.width, g.height, g.width_step = w.value, h.value, ws.value
        g.offset = np.zeros(2)
        capi.check(capi.lib().kh_occupancy_geometry(handle, g.offset, None), "kh_occupancy_geometry")
        g.resolution = float(resolution)
        return g

    @staticmethod
    def CreateFromScans(scans, resolution, laser, device: int = 0, min_pass_through=2, occupancy_threshold=0.1):
        """OccupancyGrid::CreateFromScans (Karto.h:5947-5962); `laser` supplies GetRangeThreshold / GetMinimumRange /
        GetMaximumRange of the scans' LaserRangeFinder.  Returns None for an empty scan list like the reference."""
        if not scans:
            return None
        w, h, off = compute_dimensions(scans, laser.min_range, laser.range_threshold, resolution)
        g = OccupancyGrid(w, h, off, resolution, device)
        g.AddScans(scans, laser)
        g.Update(min_pass_through, occupancy_threshold)
        return g

    def AddScans(self, scans, laser):
        capi.check(capi.lib().kh_occupancy_add_scans(self._h, len(scans), _scan_array(scans), float(laser.range_threshold),
                                                     float(laser.min_range), float(laser.max_range)), "kh_occupancy_add_scans")

    def Update(self, min_pass_through=2, occupancy_threshold=0.1):
        capi.check(capi.lib().kh_occupancy_update(self._h, int(min_pass_through), float(occupancy_threshold)), "kh_occupancy_update")

    def Clear(self):
        capi.check(capi.lib().kh_occupancy_clear(self._h), "kh_occupancy_clear")

    def GetWidth(self):
        return self.width

    def GetHeight(self):
        return self.height

    def cells(self):
        out = np.zeros(self.width_step * self.height, dtype=np.uint8)
        capi.check(capi.lib().kh_occupancy_read(self._h, out.ctypes.data, None, None), "kh_occupancy_read")
        return out.reshape(self.height, self.width_step)

    def nav(self):
        """kh_occupancy_read_nav: (height, width) int8 without row padding, the data of a nav_msgs/OccupancyGrid (vis_utils::toNavMap):
        -1 unknown, 100 occupied, 0 free"""
        out = np.zeros((self.height, self.width), dtype=np.int8)
        capi.check(capi.lib().kh_occupancy_read_nav(self._h, out.ctypes.data), "kh_occupancy_read_nav")
        return out

    def view(self) -> capi.KhMapView:
        """kh_occupancy_view: the cell states where they lie on the device, for ScanMatcher.AddMap / MatchScanMap*.  Borrowed:
        valid until the grid is next updated, cleared, written or closed."""
        v = capi.KhMapView()
        capi.check(capi.lib().kh_occupancy_view(self._h, C.byref(v)), "kh_occupancy_view")
        return v

    @staticmethod
    def from_nav(nav, offset, resolution, device: int = 0):
        """A grid from the data of a nav_msgs/OccupancyGrid or a map image turned into its values: nav is (height, width) int8 of
        -1 unknown / 100 occupied / 0 free (kh_occupancy_write_nav, the inverse of nav()); any other value raises.  The counters
        are zero: Update() would recompute the cells from them."""
        nav = np.ascontiguousarray(nav, dtype=np.int8)
        if nav.ndim != 2:
            raise ValueError("nav must be (height, width)")
        g = OccupancyGrid(nav.shape[1], nav.shape[0], offset, resolution, device)
        g.write_nav(nav)
        return g

    def write_nav(self, nav):
        nav = np.ascontiguousarray(nav, dtype=np.int8)
        if nav.shape != (self.height, self.width):
            raise ValueError("nav must be (height, width) of this grid")
        capi.check(capi.lib().kh_occupancy_write_nav(self._h, nav.ctypes.data), "kh_occupancy_write_nav")

    def counters(self):
        p = np.zeros(self.width_step * self.height, dtype=np.uint32)
        h = np.zeros(self.width_step * self.height, dtype=np.uint32)
        capi.check(capi.lib().kh_occupancy_read(self._h, None, p.ctypes.data, h.ctypes.data), "kh_occupancy_read")
        return p.reshape(self.height, self.width_step), h.reshape(self.height, self.width_step)

    def stats(self):
        ms, beams = C.c_double(), C.c_int64()
        capi.check(capi.lib().kh_occupancy_info(self._h, None, None, None, C.byref(ms), C.byref(beams)), "kh_occupancy_info")
        return {"trace_ms": ms.value, "beams": beams.value}

    def close(self):
        if self._h:
            capi.lib().kh_occupancy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
