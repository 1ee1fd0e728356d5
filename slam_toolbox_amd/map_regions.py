"""Map regions over the C ABI (kh_map_regions_*; include/karto_hip.h): the connected pieces of free space a
robot of a given radius can move in, and the frontier -- free cells next to unknown ones -- as clusters an explorer can drive to.

    field = MapField(grid, max_distance=2.0)
    regions = MapRegions(field, min_clearance=0.2)          # or field.regions(min_clearance=0.2)
    regions.region_ids                                      # (height, width) uint32: the kept id, KH_REGION_NONE, KH_REGION_DROPPED
    regions.regions[0]                                      # a record: root, n_cells, box, centroid, anchor_xy, n_other, link, ...
    regions.reachable(robot_xy, seed_xy)                    # are the two points in the same region?
    [f["anchor_xy"] for f in regions.frontiers if f["link"] == here]   # where to explore next from region `here`
    field.update(grid); regions.recompute(field)            # the map changed

Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

RECORD_FIELDS = tuple(k for k, _ in capi.KhRegion._fields_)


class MapRegions:
    def __init__(self, field, **params):
        """kh_map_regions_create.  field: a MapField; params: fields of kh_map_regions_params over its defaults.  The handle does
        not borrow the field."""
        self._h = C.c_void_p()
        p = capi.KhMapRegionsParams()
        capi.lib().kh_map_regions_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        capi.check(capi.lib().kh_map_regions_create(field._h, C.byref(p), C.byref(self._h)), "kh_map_regions_create")
        self._read_stats()

    def _read_stats(self):
        st = capi.KhMapRegionsStats()
        capi.check(capi.lib().kh_map_regions_stats_get(self._h, C.byref(st)), "kh_map_regions_stats_get")
        self.stats = {k: (list(getattr(st, k)) if k in ("n_total", "n_kept", "truncated", "times_ms") else getattr(st, k))
                      for k, _ in capi.KhMapRegionsStats._fields_}
        self.width, self.height = st.width, st.height

    def recompute(self, field):
        """kh_map_regions_recompute: the whole analysis again, of `field` as it stands (the same lattice)"""
        capi.check(capi.lib().kh_map_regions_recompute(self._h, field._h), "kh_map_regions_recompute")
        self._read_stats()

    def _ids(self, which):
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        capi.check(capi.lib().kh_map_regions_read(self._h, which, out.ctypes.data), "kh_map_regions_read")
        return out

    def _records(self, which):
        n = C.c_int32()
        capi.check(capi.lib().kh_map_regions_get(self._h, which, None, 0, C.byref(n)), "kh_map_regions_get")
        out = (capi.KhRegion * max(1, n.value))()
        capi.check(capi.lib().kh_map_regions_get(self._h, which, out, n.value, C.byref(n)), "kh_map_regions_get")
        return [{k: (tuple(getattr(r, k)) if k in ("box", "centroid", "anchor_xy") else getattr(r, k)) for k in RECORD_FIELDS} for r in out[:n.value]]

    @property
    def region_ids(self):
        """(height, width) uint32: the kept region id of every cell, capi.KH_REGION_NONE / KH_REGION_DROPPED"""
        return self._ids(capi.KH_REGIONS)

    @property
    def frontier_ids(self):
        return self._ids(capi.KH_FRONTIERS)

    @property
    def regions(self):
        """the kept regions in id order: a list of dicts, kh_region's fields"""
        return self._records(capi.KH_REGIONS)

    @property
    def frontiers(self):
        return self._records(capi.KH_FRONTIERS)

    def lookup(self, xy):
        """kh_map_regions_lookup of (n, 2) world points -> (status (n,) int32 KH_REGION_AT_ / KH_REGION_OUTSIDE, id (n,) uint32)"""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        status, ids = np.zeros(max(1, n), dtype=np.int32), np.zeros(max(1, n), dtype=np.uint32)
        capi.check(capi.lib().kh_map_regions_lookup(self._h, n, xy.ctypes.data, status.ctypes.data, ids.ctypes.data), "kh_map_regions_lookup")
        return status[:n], ids[:n]

    def reachable(self, a, b) -> bool:
        """can a robot of the analysed clearance get from world point a to world point b?"""
        status, ids = self.lookup([a, b])
        return bool(status[0] == capi.KH_REGION_AT_OK and status[1] == capi.KH_REGION_AT_OK and ids[0] == ids[1])

    def close(self):
        if self._h:
            capi.lib().kh_map_regions_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
