"""The live occupancy map of a mapper over the C ABI (kh_live_map_*): pass / hit / cell grids that stay on the mapper's device and
are brought up to date by the difference since the last update (include/karto_hip.h).

    live = mapper.live_map(resolution=0.05)
    ... mapper.Process(...) ...
    live.update()                      # every map_update_interval
    cells = live.cells()               # (height, width_step) uint8: 0 unknown, 100 occupied, 255 free
    live.close()                       # before mapper.close()

The way out for a consumer that wants nav_msgs/OccupancyGrid values and only what changed (kh_map_feed_*):

    feed = live.feed()                 # one per consumer
    delta, tile_xy, data = feed.poll() # after live.update(): the 16 x 16 tiles whose values changed since the last poll
    full = feed.read(x, y, w, h)       # any lattice rectangle of what the consumer has been told, -1 outside
    feed.close()                       # before live.close()

A distance field that follows the map (kh_live_map_field_*; slam_toolbox_amd.map_field.MapField):

    field = live.field(max_distance=2.0)
    u = field.sync()                   # after live.update(): what the updates changed since the last sync, recomputed exactly

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

    def view(self) -> capi.KhMapView:
        """kh_live_map_view: the window's cell states where they lie on the device, for ScanMatcher.AddMap / MatchScanMap*.
        Borrowed: valid until the next update(); raises (KH_ERR_NOT_FOUND) before the first scan."""
        v = capi.KhMapView()
        capi.check(capi.lib().kh_live_map_view(self._h, C.byref(v)), "kh_live_map_view")
        return v

    def stats(self) -> dict:
        st = capi.KhLiveMapStats()
        capi.check(capi.lib().kh_live_map_stats(self._h, C.byref(st)), "kh_live_map_stats")
        counts = lambda c: {k: getattr(c, k) for k, _ in capi.KhLiveMapCounts._fields_}
        return {"last": counts(st.last), "total": counts(st.total), "updates": st.updates, "scans_in_map": st.scans_in_map,
                "log_bytes": st.log_bytes}

    def feed(self) -> "MapFeed":
        """kh_map_feed_create: a feed of changed tiles for one consumer.  Close it before the live map."""
        return MapFeed(self)

    def field(self, max_distance: float = 2.0, obstacles=capi.KH_FIELD_OBSTACLE_OCCUPIED):
        """kh_live_map_field_create: a MapField of the current window that follows this map through its .sync().  Raises
        (KH_ERR_NOT_FOUND) before the first scan."""
        from .map_field import MapField
        return MapField._following(self, max_distance, obstacles)

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


class MapFeed:
    def __init__(self, live: LiveMap):
        self._live = live                  # the feed borrows the live map: keep it alive
        self._h = C.c_void_p()
        capi.check(capi.lib().kh_map_feed_create(live._h, C.byref(self._h)), "kh_map_feed_create")

    def poll(self):
        """kh_map_feed_poll + kh_map_feed_tiles -> (delta dict, tile_xy (n, 2) int32 of (tx, ty), data (n, 16, 16) int8), the tiles
        in ascending (ty, tx) order"""
        d = capi.KhMapFeedDelta()
        capi.check(capi.lib().kh_map_feed_poll(self._h, C.byref(d)), "kh_map_feed_poll")
        delta = {k: getattr(d, k) for k, _ in capi.KhMapFeedDelta._fields_}
        t = capi.KH_MAP_TILE
        xy, data = np.zeros((d.n_tiles, 2), dtype=np.int32), np.zeros((d.n_tiles, t, t), dtype=np.int8)
        capi.check(capi.lib().kh_map_feed_tiles(self._h, xy.ctypes.data, data.ctypes.data), "kh_map_feed_tiles")
        return delta, xy, data

    def read(self, x: int, y: int, w: int, h: int) -> np.ndarray:
        """kh_map_feed_read: lattice cells [x, x + w) x [y, y + h) of the published grid as (h, w) int8, -1 outside the window"""
        out = np.zeros((int(h), int(w)), dtype=np.int8)
        capi.check(capi.lib().kh_map_feed_read(self._h, int(x), int(y), int(w), int(h), out.ctypes.data), "kh_map_feed_read")
        return out

    def stats(self) -> dict:
        st = capi.KhMapFeedStats()
        capi.check(capi.lib().kh_map_feed_stats(self._h, C.byref(st)), "kh_map_feed_stats")
        return {k: getattr(st, k) for k, _ in capi.KhMapFeedStats._fields_}

    def close(self):
        if self._h:
            capi.lib().kh_map_feed_destroy(self._h)
            self._h = C.c_void_p()
        self._live = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
