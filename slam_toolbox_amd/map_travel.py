"""Travel costs on a map over the C ABI (kh_map_travel_*; include/karto_hip.h): for a set of goal points the
least cost of travelling from every traversable cell to the nearest goal, over the 4 or 8 neighbours, weighted by the inflation cost
of the cells passed -- and its readers: the cost at world points, the path of cells from a start, a ranking of frontier clusters.

    field = MapField(grid, max_distance=2.0)
    travel = MapTravel(field, min_clearance=0.2)            # or field.travel(min_clearance=0.2)
    travel.solve([dock_xy])                                 # -> the goals' KH_TRAVEL_GOAL_ statuses
    travel.values                                           # (height, width) uint32, KH_TRAVEL_FAR where no goal is reached
    travel.lookup([robot_xy], snap_cells=2)                 # -> statuses, values, lattice cells
    travel.paths([robot_xy], max_cells=4096)[0].xy          # the world points of the path to the dock
    travel.rank(regions.frontiers, snap_cells=1)            # frontier clusters, cheapest to reach first (solve from the robot)
    field.update(grid); travel.recompute(field)             # the map changed: the solution is dropped

Nothing here computes but `rank`, which sorts: every other call lands in the library."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import capi

Path = namedtuple("Path", "status cost start_cell cells xy")
_INFLATION = tuple(k for k, _ in capi.KhInflationParams._fields_)


def _params(params):
    p = capi.KhMapTravelParams()
    capi.lib().kh_map_travel_params_default(C.byref(p))
    for k, v in params.items():
        if k in _INFLATION:
            setattr(p.inflation, k, v)
        elif hasattr(p, k) and k != "inflation":
            setattr(p, k, v)
        else:
            raise KeyError(k)
    return p


def reach_of(params) -> float:
    """the distance in metres a field must reach for these parameters: min_clearance and, with a cost_weight above 0, the inflation
    radius (MapLocalizer.travel sizes its field by it)"""
    p = _params(params)
    return max(float(p.min_clearance), float(p.inflation.inflation_radius) if p.cost_weight > 0 else 0.0)


class MapTravel:
    def __init__(self, field, **params):
        """kh_map_travel_create.  field: a MapField; params: fields of kh_map_travel_params, and of its kh_inflation_params by their
        own names, over the defaults.  The handle does not borrow the field."""
        self._h = C.c_void_p()
        p = _params(params)
        capi.check(capi.lib().kh_map_travel_create(field._h, C.byref(p), C.byref(self._h)), "kh_map_travel_create")
        self.anchor, self.scale = tuple(field.anchor), float(field.scale)
        self._read_stats()

    def _read_stats(self):
        st = capi.KhMapTravelStats()
        capi.check(capi.lib().kh_map_travel_stats_get(self._h, C.byref(st)), "kh_map_travel_stats_get")
        self.stats = {k: (list(getattr(st, k)) if k == "times_ms" else getattr(st, k)) for k, _ in capi.KhMapTravelStats._fields_ if not k.startswith("pad")}
        self.width, self.height = st.width, st.height

    def recompute(self, field):
        """kh_map_travel_recompute: the weights again, of `field` as it stands (the same lattice); the solution is dropped"""
        capi.check(capi.lib().kh_map_travel_recompute(self._h, field._h), "kh_map_travel_recompute")
        self._read_stats()

    def set_rounds_per_check(self, k: int):
        """kh_map_travel_set_rounds_per_check (debugging): launches between two reads of the flag word, 0: the library's choice"""
        capi.check(capi.lib().kh_map_travel_set_rounds_per_check(self._h, int(k)), "kh_map_travel_set_rounds_per_check")

    def solve(self, goals):
        """kh_map_travel_solve from (n, 2) world points -> (n,) int32 KH_TRAVEL_GOAL_ statuses"""
        xy = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        status = np.zeros(max(1, len(xy)), dtype=np.int32)
        capi.check(capi.lib().kh_map_travel_solve(self._h, len(xy), xy.ctypes.data, status.ctypes.data), "kh_map_travel_solve")
        self._read_stats()
        return status[:len(xy)]

    def _read(self, dtype, which):
        out = np.zeros((self.height, self.width), dtype=dtype)
        args = (out.ctypes.data, None) if which == 0 else (None, out.ctypes.data)
        capi.check(capi.lib().kh_map_travel_read(self._h, *args), "kh_map_travel_read")
        return out

    @property
    def values(self):
        """(height, width) uint32: the travel cost of every cell, capi.KH_TRAVEL_FAR where no goal is reached"""
        return self._read(np.uint32, 0)

    @property
    def weights(self):
        """(height, width) uint16: q of every cell, 0 where it is not traversable"""
        return self._read(np.uint16, 1)

    def lookup(self, xy, snap_cells: int = 0):
        """kh_map_travel_lookup of (n, 2) world points -> (status (n,) int32 KH_TRAVEL_AT_, value (n,) uint32, cell (n, 2) int32)"""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        status, value, cell = np.zeros(max(1, n), dtype=np.int32), np.zeros(max(1, n), dtype=np.uint32), np.zeros((max(1, n), 2), dtype=np.int32)
        capi.check(capi.lib().kh_map_travel_lookup(self._h, n, xy.ctypes.data, int(snap_cells), status.ctypes.data, value.ctypes.data, cell.ctypes.data),
                   "kh_map_travel_lookup")
        return status[:n], value[:n], cell[:n]

    def cell_world(self, cells):
        """the world points of (n, 2) lattice cells by the view's rule: anchor + cell / scale"""
        cells = np.asarray(cells, dtype=np.int32).reshape(-1, 2)
        return np.stack([self.anchor[0] + cells[:, 0].astype(np.float64) / self.scale, self.anchor[1] + cells[:, 1].astype(np.float64) / self.scale], axis=1)

    def paths(self, starts, snap_cells: int = 0, max_cells: int = 4096):
        """kh_map_travel_paths from (n, 2) world points -> a list of Path(status, cost, start_cell, cells (k, 2) int32 lattice cells,
        xy (k, 2) their world points)"""
        xy = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        heads = (capi.KhTravelPath * max(1, n))()
        cells = np.zeros((max(1, n), int(max_cells), 2), dtype=np.int32)
        capi.check(capi.lib().kh_map_travel_paths(self._h, n, xy.ctypes.data, int(snap_cells), int(max_cells), heads, cells.ctypes.data), "kh_map_travel_paths")
        out = []
        for k in range(n):
            mine = cells[k, :heads[k].n_cells].copy()
            out.append(Path(heads[k].status, heads[k].cost, heads[k].start_cell, mine, self.cell_world(mine)))
        return out

    def rank(self, clusters, snap_cells: int = 0):
        """host only: frontier records (MapRegions.frontiers) ordered by (the value at their anchor_xy, id) -- the id is the record's
        place in `clusters` --, the unreached ones last in id order.  -> a list of (id, value, record); value None where unreached"""
        clusters = list(clusters)
        if not clusters:
            return []
        status, value, _ = self.lookup([c["anchor_xy"] for c in clusters], snap_cells)
        reached = sorted((int(value[k]), k) for k in range(len(clusters)) if status[k] == capi.KH_TRAVEL_AT_OK)
        rest = [k for k in range(len(clusters)) if status[k] != capi.KH_TRAVEL_AT_OK]
        return [(k, v, clusters[k]) for v, k in reached] + [(k, None, clusters[k]) for k in rest]

    def close(self):
        if self._h:
            capi.lib().kh_map_travel_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
