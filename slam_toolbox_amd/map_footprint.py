"""Footprints on a map over the C ABI (kh_map_footprint_*; include/karto_hip.h): does a robot that is not round
-- a convex polygon in its own frame -- fit at a pose, at a heading?  Many poses against one footprint, or every cell of the window
turned to each of a set of headings.

    field = MapField(grid, max_distance=2.0)
    fp = MapFootprint(field, [(0.5, 0.3), (-0.5, 0.3), (-0.5, -0.3), (0.5, -0.3)])      # or field.footprint(vertices)
    fp.check([(x, y, theta)])["status"]                     # KH_FOOTPRINT_FREE / _UNKNOWN / _OUTSIDE / _COLLISION / _LATTICE
    records, first = fp.check_path(travel.paths([robot_xy])[0].xy)       # the first pose of a path the robot does not fit at, or -1
    masks, summary = fp.layer(n_headings=16, max_status=0)  # (height, width) uint32: bit h set where heading h fits
    field.update(grid); fp.recompute(field)                 # the map changed

Nothing here computes but `check_path`, which turns consecutive points into headings: every other call lands in the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

FOOTPRINT_DTYPE = np.dtype([(k, np.int32 if k == "status" else np.uint32) for k, _ in capi.KhFootprint._fields_])


class MapFootprint:
    def __init__(self, field, vertices):
        """kh_map_footprint_create.  field: a MapField; vertices: (n, 2) metres in the robot frame, 3 .. 16 of them, strictly convex
        in either winding.  The handle does not borrow the field."""
        self._h = C.c_void_p()
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 2)
        capi.check(capi.lib().kh_map_footprint_create(field._h, len(v), v.ctypes.data, C.byref(self._h)), "kh_map_footprint_create")
        self.vertices = v.copy()
        self.width, self.height = self.stats["width"], self.stats["height"]

    @property
    def stats(self):
        st = capi.KhMapFootprintStats()
        capi.check(capi.lib().kh_map_footprint_stats_get(self._h, C.byref(st)), "kh_map_footprint_stats_get")
        return {k: (list(getattr(st, k)) if k == "times_ms" else getattr(st, k)) for k, _ in capi.KhMapFootprintStats._fields_ if k != "pad"}

    def recompute(self, field):
        """kh_map_footprint_recompute: the snapshot again, of `field` as it stands (the same lattice)"""
        capi.check(capi.lib().kh_map_footprint_recompute(self._h, field._h), "kh_map_footprint_recompute")
        self.width, self.height = self.stats["width"], self.stats["height"]

    def check(self, poses):
        """kh_map_footprint_check of (n, 3) poses (x, y, theta) -> (n,) records of FOOTPRINT_DTYPE (kh_footprint_t)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(max(1, len(poses)), dtype=FOOTPRINT_DTYPE)
        capi.check(capi.lib().kh_map_footprint_check(self._h, len(poses), poses.ctypes.data, out.ctypes.data), "kh_map_footprint_check")
        return out[:len(poses)]

    @staticmethod
    def path_poses(xy):
        """host only: (n, 2) world points -> (n, 3) poses whose heading points from each point to the next, the last heading repeated
        (0 for a single point)"""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        poses = np.zeros((len(xy), 3), dtype=np.float64)
        poses[:, :2] = xy
        if len(xy) > 1:
            d = xy[1:] - xy[:-1]
            poses[:-1, 2] = np.arctan2(d[:, 1], d[:, 0])
            poses[-1, 2] = poses[-2, 2]
        return poses

    def check_path(self, xy, level: int = capi.KH_FOOTPRINT_COLLISION):
        """host only, then `check`: the points of a path (MapTravel.paths(...)[k].xy as it is) as poses by `path_poses`
        -> (records, the first index whose status is at or above `level`, or -1)"""
        poses = self.path_poses(xy)
        if len(poses) == 0:
            return np.zeros(0, dtype=FOOTPRINT_DTYPE), -1
        records = self.check(poses)
        at = np.flatnonzero(records["status"] >= int(level))
        return records, (int(at[0]) if len(at) else -1)

    def layer(self, n_headings: int, max_status: int = capi.KH_FOOTPRINT_FREE, masks: bool = True):
        """kh_map_footprint_layer -> ((height, width) uint32 masks, bit h set where the footprint turned to heading 2 pi h / n_headings
        has a status <= max_status at the cell -- None with masks=False --, summary: n_fit (n_headings,), n_any, n_all)"""
        out = np.zeros((self.height, self.width), dtype=np.uint32) if masks else None
        s = capi.KhFootprintLayer()
        capi.check(capi.lib().kh_map_footprint_layer(self._h, int(n_headings), int(max_status), out.ctypes.data if masks else None, C.byref(s)),
                   "kh_map_footprint_layer")
        return out, {"n_fit": np.array(list(s.n_fit)[:int(n_headings)], dtype=np.uint64), "n_any": int(s.n_any), "n_all": int(s.n_all)}

    def close(self):
        if self._h:
            capi.lib().kh_map_footprint_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
