"""Visibility on a map over the C ABI (kh_map_visibility_*; include/karto_hip.h): the distinct cells a sensor
standing at a pose would see of a map, by state; those among them no committed viewpoint has seen; and a greedy choice of viewpoints.

    vis = MapVisibility(grid, laser, max_unknown=20)        # or localizer.visibility()
    vis.commit([where_the_robot_has_been])                  # the covered mask takes what was seen from there
    poses = vis.candidates(regions, n_headings=4)           # the frontier anchors as sensor poses
    vis.gain(poses)["gain"]                                 # what each would add
    picks, gains = vis.select(poses, k=3)                   # three viewpoints, each counted against the ones before it
    vis.mask                                                # (height, width) bool: what the commits and the picks cover

Nothing here computes but `candidates`, which lists poses: every other call lands in the library."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi

VISIBILITY_DTYPE = np.dtype([(k, np.uint32) for k, _ in capi.KhVisibility._fields_])


def _params(params):
    p = capi.KhVisibilityParams()
    capi.lib().kh_map_visibility_params_default(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, int(v))
    return p


def _poses(poses):
    return np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)


class MapVisibility:
    def __init__(self, view, laser, **params):
        """kh_map_visibility_create.  view: a capi.KhMapView, an OccupancyGrid or a LiveMap; laser: a capi.KhLaser or a laser record;
        params: fields of kh_visibility_params over the defaults.  The cells are borrowed: keep the source alive, and set the map
        again after it was updated."""
        from .map_localizer import _laser_of, _view_of
        self._h = C.c_void_p()
        self._source = view
        v = _view_of(view)
        L = laser if isinstance(laser, capi.KhLaser) else _laser_of(laser)
        p = _params(params)
        capi.check(capi.lib().kh_map_visibility_create(C.byref(v), C.byref(L), C.byref(p), C.byref(self._h)), "kh_map_visibility_create")
        self.width, self.height = v.width, v.height

    @property
    def stats(self):
        st = capi.KhMapVisibilityStats()
        capi.check(capi.lib().kh_map_visibility_stats_get(self._h, C.byref(st)), "kh_map_visibility_stats_get")
        return {k: getattr(st, k) for k, _ in capi.KhMapVisibilityStats._fields_ if k != "pad"}

    def set_map(self, view):
        """kh_map_visibility_set_map: another view of the same window and lattice; the mask is kept"""
        from .map_localizer import _view_of
        v = _view_of(view)
        capi.check(capi.lib().kh_map_visibility_set_map(self._h, C.byref(v)), "kh_map_visibility_set_map")
        self._source = view
        return self

    def set_skip(self, skip: bool):
        """kh_map_visibility_set_skip (measuring): read a bitmap word before the OR, or always OR"""
        capi.check(capi.lib().kh_map_visibility_set_skip(self._h, int(bool(skip))), "kh_map_visibility_set_skip")

    def clear(self):
        capi.check(capi.lib().kh_map_visibility_clear(self._h), "kh_map_visibility_clear")

    def commit(self, poses):
        """kh_map_visibility_commit of (n, 3) sensor poses: what they see joins the covered mask"""
        poses = _poses(poses)
        capi.check(capi.lib().kh_map_visibility_commit(self._h, len(poses), poses.ctypes.data), "kh_map_visibility_commit")

    def gain(self, poses):
        """kh_map_visibility_gain of (n, 3) sensor poses -> (n,) records of VISIBILITY_DTYPE (kh_visibility_t)"""
        poses = _poses(poses)
        out = np.zeros(max(1, len(poses)), dtype=VISIBILITY_DTYPE)
        ms = C.c_double()
        capi.check(capi.lib().kh_map_visibility_gain(self._h, len(poses), poses.ctypes.data, out.ctypes.data, C.byref(ms)), "kh_map_visibility_gain")
        self.kernel_ms = ms.value
        return out[:len(poses)]

    def select(self, poses, k: int, min_gain: int = 1):
        """kh_map_visibility_select among (n, 3) sensor poses -> (indices (m,) int32, gains (m,) uint32), m <= k picks in pick order.
        The mask is not cleared first, and is left holding the picks."""
        poses = _poses(poses)
        picks, gains = np.zeros(max(1, int(k)), dtype=np.int32), np.zeros(max(1, int(k)), dtype=np.uint32)
        n = C.c_int32()
        capi.check(capi.lib().kh_map_visibility_select(self._h, len(poses), poses.ctypes.data, int(k), int(min_gain), picks.ctypes.data, gains.ctypes.data,
                                                       C.byref(n)), "kh_map_visibility_select")
        return picks[:n.value].copy(), gains[:n.value].copy()

    @property
    def mask(self):
        """(height, width) bool: the covered mask"""
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        capi.check(capi.lib().kh_map_visibility_read_mask(self._h, out.ctypes.data), "kh_map_visibility_read_mask")
        return out.astype(bool)

    @staticmethod
    def candidates(regions, n_headings: int = 1):
        """host only: the frontier records' anchor_xy (a MapRegions, or a list of its frontier records) as sensor poses, n_headings
        evenly spaced from 0 at each -> (n_frontiers * n_headings, 3) float64, frontier-major"""
        records = regions.frontiers if hasattr(regions, "frontiers") else regions
        n_headings = max(1, int(n_headings))
        out = [(float(r["anchor_xy"][0]), float(r["anchor_xy"][1]), h * (2.0 * math.pi / n_headings)) for r in records for h in range(n_headings)]
        return np.asarray(out, dtype=np.float64).reshape(-1, 3)

    def close(self):
        if self._h:
            capi.lib().kh_map_visibility_destroy(self._h)
            self._h = C.c_void_p()
        self._source = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
