"""Two finished maps merged into one over the C ABI (kh_map_merge_*; include/karto_hip.h): the map `moving`
warped through a rigid correction onto the lattice of the map `target`, the two composed cell by cell, the overlap counted.

    candidates, _ = localizer.align(other_map)              # where the other map lies in the localizer's (kh_map_align)
    merged = localizer.merge(other_map, candidates[0].correction)
    merged.stats["agreement"]                               # a dense second opinion on the alignment
    localizer.set_map(merged.view)                          # the merged map, on the device, on the target's lattice
    nav = merged.nav()                                      # ... and as nav_msgs/OccupancyGrid values

Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .map_localizer import _view_of

CONFLICTS = dict(target=capi.KH_MERGE_CONFLICT_TARGET, moving=capi.KH_MERGE_CONFLICT_MOVING, occupied=capi.KH_MERGE_CONFLICT_OCCUPIED,
                 unknown=capi.KH_MERGE_CONFLICT_UNKNOWN)


class MapMerge:
    def __init__(self, target, moving, correction, footprint: int = 0, conflict=capi.KH_MERGE_CONFLICT_OCCUPIED, grow: int = 1):
        """kh_map_merge_create.  target, moving: a capi.KhMapView, an OccupancyGrid, a LiveMap, or another MapMerge (its merged map);
        correction (x, y, yaw): moving map -> target map, what AlignCandidate.correction holds.  footprint 0: the default for the two
        resolutions; conflict: a KH_MERGE_CONFLICT_ value or one of "target", "moving", "occupied", "unknown".  Both inputs are only
        read and may go once this returns: the merged map is the handle's own."""
        self._h = C.c_void_p()
        t, m = _view_of(target), _view_of(moving)
        p = capi.KhMapMergeParams()
        capi.lib().kh_map_merge_params_default(C.byref(p))
        p.correction[0], p.correction[1], p.correction[2] = (float(v) for v in correction)
        p.footprint, p.conflict, p.grow = int(footprint), int(CONFLICTS.get(conflict, conflict)), int(grow)
        capi.check(capi.lib().kh_map_merge_create(C.byref(t), C.byref(m), C.byref(p), C.byref(self._h)), "kh_map_merge_create")
        st = capi.KhMapMergeStats()
        capi.check(capi.lib().kh_map_merge_stats_get(self._h, C.byref(st)), "kh_map_merge_stats_get")
        self.stats = {k: (list(getattr(st, k)) if k in ("known_box", "times_ms") else getattr(st, k)) for k, _ in capi.KhMapMergeStats._fields_}
        self.width, self.height, self.width_step = st.width, st.height, st.width_step
        self.view = capi.KhMapView()
        capi.check(capi.lib().kh_map_merge_view(self._h, C.byref(self.view)), "kh_map_merge_view")

    def _read(self, which):
        out = np.zeros((self.height, self.width_step), dtype=np.uint8)
        args = (out.ctypes.data, None) if which == 0 else (None, out.ctypes.data)
        capi.check(capi.lib().kh_map_merge_read(self._h, *args), "kh_map_merge_read")
        return out

    def cells(self):
        """the merged cell states (0 unknown, 100 occupied, 255 free), (height, width_step) uint8, the padding 0"""
        return self._read(0)

    def codes(self):
        """the KH_MERGED_ code of every cell, (height, width_step) uint8"""
        return self._read(1)

    def nav(self):
        """kh_map_merge_read_nav: the merged cells as (height, width) int8 nav values"""
        out = np.zeros((self.height, self.width), dtype=np.int8)
        capi.check(capi.lib().kh_map_merge_read_nav(self._h, out.ctypes.data), "kh_map_merge_read_nav")
        return out

    def close(self):
        if self._h:
            capi.lib().kh_map_merge_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
