"""The live occupancy map of a mapper over the C ABI (kh_live_map_*): pass / hit / cell grids that stay on the mapper's device and
are brought up to date by the difference since the last update (include/karto_hip.h).

    live = mapper.live_map(resolution=0.05)
    ... mapper.Process(...) ...
    live.update()                      # every map_update_interval
    cells = live.cells()               # (height, width_step) uint8: 0 unknown, 100 occupied, 255 free
    live.close()                       # before mapper.close()

Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class LiveMap:
    def __init__(self, mapper, resolution: float = 0.05, anchor=None, rebuild_fraction: float = None):
        self._mapper = mapper              # the live map borrows the mapper: keep it alive
        self._h = C.c_void_p()
        a = None if anchor is None else np.ascontiguousarray(anchor, dtype=np.float64).copy()
        capi.check(capi.lib().kh_live_map_create(mapper._h, float(resolution), None if a is None else a.ctypes.data,
                                                 -1.0 if rebuild_fraction is None else float(rebuild_fraction), C.byref(self._h)),
                   "kh_live_map_create")

    def update(self, min_pass_through: int = 2, occupancy_threshold: float = 0.1) -> dict:
        """kh_live_map_update; returns the counters of this update (stats()["last"])"""
        capi.check(capi.lib().kh_live_map_update(self._h, int(min_pass_through), float(occupancy_threshold)), "kh_live_map_update")
        return self.stats()["last"]

    def info(self) -> dict:
        i = capi.KhLiveMapInfo()
        capi.check(capi.lib().kh_live_map_info(self._h, C.byref(i)), "kh_live_map_info")
        out = {k: getattr(i, k) for k in ("resolution", "rebuild_fraction", "ox", "oy", "width", "height", "width_step", "reach")}
        out["anchor"] = np.array(i.anchor[:])
        return out

    def _read(self, dtype):
        i = self.info()
        return np.zeros(i["width_step"] * i["height"], dtype=dtype), (i["height"], i["width_step"])

    def cells(self) -> np.ndarray:
        out, shape = self._read(np.uint8)
        capi.check(capi.lib().kh_live_map_read(self._h, out.ctypes.data, None, None), "kh_live_map_read")
        return out.reshape(shape)

    def counters(self):
        """(pass, hits), each (height, width_step) uint32"""
        p, shape = self._read(np.uint32)
        h = np.zeros_like(p)
        capi.check(capi.lib().kh_live_map_read(self._h, None, p.ctypes.data, h.ctypes.data), "kh_live_map_read")
        return p.reshape(shape), h.reshape(shape)

    def stats(self) -> dict:
        st = capi.KhLiveMapStats()
        capi.check(capi.lib().kh_live_map_stats(self._h, C.byref(st)), "kh_live_map_stats")
        counts = lambda c: {k: getattr(c, k) for k, _ in capi.KhLiveMapCounts._fields_}
        return {"last": counts(st.last), "total": counts(st.total), "updates": st.updates, "scans_in_map": st.scans_in_map,
                "log_bytes": st.log_bytes}

    def close(self):
        if self._h:
            capi.lib().kh_live_map_destroy(self._h)
            self._h = C.c_void_p()
        self._mapper = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
