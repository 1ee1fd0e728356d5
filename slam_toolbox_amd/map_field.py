"""The distance field of a map over the C ABI (kh_map_field_*; include/karto_hip.h): how far every cell lies
from the nearest obstacle, and what reads that -- costmap values, clearance at world points, the endpoint score of a scan at many
poses and the pose refinement built on it.

    field = MapField(grid, max_distance=2.0)                # a snapshot: the grid may change or go afterwards
    field.metres                                            # (height, width) float64, +inf beyond max_distance
    costs = field.costs(inflation_radius=0.55)              # (height, width) uint8 costmap values
    metres, status, d2 = field.clearance([[1.0, 2.0]])      # how much room is there at (x, y)?
    refined = field.refine(ranges, [sensor_pose], laser)    # descend the endpoint cost from a candidate pose

A field can follow its map: the part of the map that changed is compared and recomputed, exact to the bit.

    u = field.update(grid, rect=(x, y, w, h))               # the caller knows where the map changed (None: compare everything)
    field = live.field(max_distance=2.0); u = field.sync()  # or the live map does: after every live.update()
    box = u["values_box"]; field.costs_rect(*box)           # the costs of what changed: a map_msgs/OccupancyGridUpdate

Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import capi
from .map_localizer import _laser_of, _view_of

OBSTACLES = dict(occupied=capi.KH_FIELD_OBSTACLE_OCCUPIED, not_free=capi.KH_FIELD_OBSTACLE_NOT_FREE)
SCORE_FIELDS = tuple(k for k, _ in capi.KhFieldScore._fields_)
Refined = namedtuple("Refined", "pose cost_start cost n_hit rounds halvings status")


def inflation_table(scale, **params):
    """kh_inflation_table: the costs by squared distance in cells, (Rt * Rt + 1,) uint8.  params: fields of kh_inflation_params"""
    p = _inflation(params)
    n = C.c_int32()
    capi.check(capi.lib().kh_inflation_table(C.byref(p), float(scale), None, 0, C.byref(n)), "kh_inflation_table")
    table = np.zeros(n.value, dtype=np.uint8)
    capi.check(capi.lib().kh_inflation_table(C.byref(p), float(scale), table.ctypes.data, n.value, C.byref(n)), "kh_inflation_table")
    return table


def _inflation(params):
    p = capi.KhInflationParams()
    capi.lib().kh_inflation_params_default(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class MapField:
    def __init__(self, view, max_distance: float = 2.0, obstacles=capi.KH_FIELD_OBSTACLE_OCCUPIED):
        """kh_map_field_create.  view: a capi.KhMapView or anything that has one (an OccupancyGrid, a LiveMap, a MapChanges, a
        MapMerge).  max_distance in metres, 0: uncapped; obstacles: a KH_FIELD_OBSTACLE_ value or "occupied" / "not_free".  The
        field is a snapshot: no reference to the view's owner is kept once this returns."""
        self._h = C.c_void_p()
        v = _view_of(view)
        p = capi.KhMapFieldParams()
        capi.lib().kh_map_field_params_default(C.byref(p))
        p.max_distance, p.obstacles = float(max_distance), int(OBSTACLES.get(obstacles, obstacles))
        capi.check(capi.lib().kh_map_field_create(C.byref(v), C.byref(p), C.byref(self._h)), "kh_map_field_create")
        self._live = None
        self.scale, self.anchor = v.scale, (v.anchor[0], v.anchor[1])
        self._read_stats()

    @classmethod
    def _following(cls, live, max_distance, obstacles):
        """kh_live_map_field_create (LiveMap.field)"""
        self = cls.__new__(cls)
        self._h, self._live = C.c_void_p(), live     # the field borrows the live map: keep it alive
        p = capi.KhMapFieldParams()
        capi.lib().kh_map_field_params_default(C.byref(p))
        p.max_distance, p.obstacles = float(max_distance), int(OBSTACLES.get(obstacles, obstacles))
        capi.check(capi.lib().kh_live_map_field_create(live._h, C.byref(p), C.byref(self._h)), "kh_live_map_field_create")
        v = live.view()
        self.scale, self.anchor = v.scale, (v.anchor[0], v.anchor[1])
        self._read_stats()
        return self

    def _read_stats(self):
        """kh_map_field_stats_get -> .stats, .width, .height (after an update the library recounts the three counters here)"""
        st = capi.KhMapFieldStats()
        capi.check(capi.lib().kh_map_field_stats_get(self._h, C.byref(st)), "kh_map_field_stats_get")
        self.stats = {k: (list(getattr(st, k)) if k == "times_ms" else getattr(st, k)) for k, _ in capi.KhMapFieldStats._fields_}
        self.width, self.height = st.width, st.height

    def _updated(self, u, stats):
        if stats:
            self._read_stats()
        out = {k: getattr(u, k) for k, _ in capi.KhFieldUpdate._fields_}
        out.update(cells_box=tuple(u.cells_box), values_box=tuple(u.values_box), times_ms=list(u.times_ms))
        return out

    def update(self, view, rect=None, stats=True) -> dict:
        """kh_map_field_update: the field follows `view` (on the same lattice); rect = (x, y, w, h) in lattice cells is where the
        map may have changed, None: anywhere.  -> kh_field_update's fields.  stats=False leaves .stats as it was (and the recount
        to the next reader of the statistics)."""
        v = _view_of(view)
        r = None if rect is None else (C.c_int32 * 4)(*(int(k) for k in rect))
        u = capi.KhFieldUpdate()
        capi.check(capi.lib().kh_map_field_update(self._h, C.byref(v), r, C.byref(u)), "kh_map_field_update")
        return self._updated(u, stats)

    def sync(self, stats=True) -> dict:
        """kh_live_map_field_sync: a field made by LiveMap.field() takes what the live map's updates changed since the last sync"""
        u = capi.KhFieldUpdate()
        capi.check(capi.lib().kh_live_map_field_sync(self._h, C.byref(u)), "kh_live_map_field_sync")
        return self._updated(u, stats)

    def set_band_rows(self, n: int):
        """kh_map_field_set_band_rows (debugging): the band height of an update's column pass, 0: the library's choice"""
        capi.check(capi.lib().kh_map_field_set_band_rows(self._h, int(n)), "kh_map_field_set_band_rows")

    def read_rect(self, x: int, y: int, w: int, h: int):
        """kh_map_field_read_rect: the values of lattice cells [x, x + w) x [y, y + h), (h, w) uint32"""
        out = np.zeros((max(0, int(h)), max(0, int(w))), dtype=np.uint32)
        capi.check(capi.lib().kh_map_field_read_rect(self._h, int(x), int(y), int(w), int(h), out.ctypes.data), "kh_map_field_read_rect")
        return out

    def costs_rect(self, x: int, y: int, w: int, h: int, **params):
        """kh_map_field_costs_rect: the costs of lattice cells [x, x + w) x [y, y + h), (h, w) uint8"""
        p = _inflation(params)
        out = np.zeros((max(0, int(h)), max(0, int(w))), dtype=np.uint8)
        capi.check(capi.lib().kh_map_field_costs_rect(self._h, C.byref(p), int(x), int(y), int(w), int(h), out.ctypes.data), "kh_map_field_costs_rect")
        return out

    @property
    def d2(self):
        """the squared distances in cells, (height, width) uint32, capi.KH_FIELD_FAR beyond the radius"""
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        capi.check(capi.lib().kh_map_field_read(self._h, out.ctypes.data, None), "kh_map_field_read")
        return out

    @property
    def metres(self):
        """the distances in metres, (height, width) float64, +inf beyond the radius"""
        out = np.zeros((self.height, self.width), dtype=np.float64)
        capi.check(capi.lib().kh_map_field_read(self._h, None, out.ctypes.data), "kh_map_field_read")
        return out

    def costs(self, **params):
        """kh_map_field_costs: (height, width) uint8 costmap values.  params: fields of kh_inflation_params over its defaults"""
        p = _inflation(params)
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        capi.check(capi.lib().kh_map_field_costs(self._h, C.byref(p), out.ctypes.data), "kh_map_field_costs")
        return out

    def clearance(self, xy):
        """kh_map_field_clearance of (n, 2) world points -> (metres (n,) float64, status (n,) int32 KH_CLEAR_, d2 (n,) uint32)"""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        metres, status, d2 = np.zeros(max(1, n)), np.zeros(max(1, n), dtype=np.int32), np.zeros(max(1, n), dtype=np.uint32)
        capi.check(capi.lib().kh_map_field_clearance(self._h, n, xy.ctypes.data, metres.ctypes.data, status.ctypes.data, d2.ctypes.data),
                   "kh_map_field_clearance")
        return metres[:n], status[:n], d2[:n]

    def score(self, ranges, poses, laser, truncate_cells: int = 0):
        """kh_map_field_score: one scan's readings at each of `poses` (n, 3) sensor poses -> list of n dicts (kh_field_score's fields)"""
        L = laser if isinstance(laser, capi.KhLaser) else _laser_of(laser)
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        assert ranges.shape == (L.n_beams,)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        out = (capi.KhFieldScore * max(1, len(poses)))()
        capi.check(capi.lib().kh_map_field_score(self._h, C.byref(L), ranges.ctypes.data, len(poses), poses.ctypes.data, int(truncate_cells), out),
                   "kh_map_field_score")
        return [{k: getattr(out[i], k) for k in SCORE_FIELDS} for i in range(len(poses))]

    def refine(self, ranges, poses, laser, **params):
        """kh_map_field_refine from each of `poses` (n, 3) sensor poses.  params: fields of kh_field_refine_params over its defaults
        for this field's scale.  -> (list of n Refined records, times_ms: the kernels, the call)"""
        L = laser if isinstance(laser, capi.KhLaser) else _laser_of(laser)
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        assert ranges.shape == (L.n_beams,)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        p = capi.KhFieldRefineParams()
        capi.lib().kh_field_refine_params_default(C.byref(p), self.scale)
        for k, v in params.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        out, times = (capi.KhFieldRefined * max(1, len(poses)))(), np.zeros(2)
        capi.check(capi.lib().kh_map_field_refine(self._h, C.byref(L), ranges.ctypes.data, len(poses), poses.ctypes.data, C.byref(p), out,
                                                  times.ctypes.data), "kh_map_field_refine")
        return [Refined(np.array(r.pose), r.cost_start, r.cost, r.n_hit, r.rounds, r.halvings, r.status) for r in out[:len(poses)]], times

    def regions(self, **params):
        """kh_map_regions_create on this field: connected free space by clearance and frontier clusters.
        params: fields of kh_map_regions_params.  -> map_regions.MapRegions, which does not borrow the field"""
        from .map_regions import MapRegions
        return MapRegions(self, **params)

    def travel(self, **params):
        """kh_map_travel_create on this field: travel costs to goal points, paths, lookups.  params: fields of
        kh_map_travel_params and of its kh_inflation_params.  -> map_travel.MapTravel, which does not borrow the field"""
        from .map_travel import MapTravel
        return MapTravel(self, **params)

    def footprint(self, vertices):
        """kh_map_footprint_create on this field: a convex polygon checked at poses and by heading.  vertices:
        (n, 2) metres in the robot frame.  -> map_footprint.MapFootprint, which does not borrow the field"""
        from .map_footprint import MapFootprint
        return MapFootprint(self, vertices)

    def close(self):
        if self._h:
            capi.lib().kh_map_field_destroy(self._h)
            self._h = C.c_void_p()
        self._live = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
