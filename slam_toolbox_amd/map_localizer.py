"""Localizing in a map alone over the C ABI (kh_map_seeds, kh_map_fit, kh_map_localizer_*; include/karto_hip.h):
the map is a device view of cell states -- an OccupancyGrid (built, merged, or from_nav of a shipped nav_msgs/OccupancyGrid), a
LiveMap, or a hand-filled capi.KhMapView -- and nothing else: no scans, no pose graph.

    loc = MapLocalizer(dict(loop_search_space_dimension=4.0), laser)
    loc.set_map(OccupancyGrid.from_nav(nav, origin, resolution))
    hyps, summary = loc.relocalize(ranges)                 # where was this scan taken?
    loc.set_pose(hyps[0].robot_pose, odometric_pose)
    step = loc.process(next_ranges, next_odometric_pose)   # ... and from there on, scan by scan

Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import capi

FIT_FIELDS = tuple(k for k, _ in capi.KhMergeFit._fields_)
MapHypothesis = namedtuple("MapHypothesis", "index seed_cell heading coarse_mean coarse_cov coarse_response fine_mean fine_cov fine_response "
                                            "robot_pose fit")
TrackStep = namedtuple("TrackStep", "predicted_pose robot_pose sensor_pose covariance response fit")
TrackStepObserved = namedtuple("TrackStepObserved", TrackStep._fields + ("labels",))      # process(..., changes=layer)


def _fit_dict(f):
    return {k: getattr(f, k) for k in FIT_FIELDS}


def _view_of(source):
    """a capi.KhMapView, or anything with .view() (OccupancyGrid, LiveMap)"""
    return source if isinstance(source, capi.KhMapView) else source.view()


def _laser_of(laser):
    off = tuple(getattr(laser, "offset", (0.0, 0.0, 0.0)))
    return capi.KhLaser(laser.n_beams, laser.min_angle, laser.ang_res, laser.min_range, laser.max_range, laser.range_threshold,
                        off[0], off[1], off[2])


def map_seeds(view, seed_spacing, center_xy=None, radius=0.0):
    """kh_map_seeds: where a robot can stand in the map -- one free cell per block of the seed lattice.
    -> (cells (n, 2) int32 lattice i, j; xy (n, 2) float64), in ascending (block row, block column)"""
    v = _view_of(view)
    c = None if center_xy is None else np.ascontiguousarray(center_xy, dtype=np.float64).copy()
    n = C.c_int32()
    args = (C.byref(v), float(seed_spacing), None if c is None else c.ctypes.data, float(radius))
    capi.check(capi.lib().kh_map_seeds(*args, None, None, 0, C.byref(n)), "kh_map_seeds")
    cells, xy = np.zeros((n.value, 2), dtype=np.int32), np.zeros((n.value, 2))
    if n.value:
        capi.check(capi.lib().kh_map_seeds(*args, cells.ctypes.data, xy.ctypes.data, n.value, C.byref(n)), "kh_map_seeds")
    return cells, xy


def map_fit(view, laser, ranges, poses):
    """kh_map_fit: the ray-consistency counters of one scan's readings at each of `poses` (n, 3) sensor poses -> list of n dicts
    (the fields of kh_merge_fit_t)"""
    v = _view_of(view)
    ranges = np.ascontiguousarray(ranges, dtype=np.float64)
    assert ranges.shape == (laser.n_beams,)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    out = (capi.KhMergeFit * max(1, len(poses)))()
    L = _laser_of(laser)
    capi.check(capi.lib().kh_map_fit(C.byref(v), C.byref(L), ranges.ctypes.data, len(poses), poses.ctypes.data, out), "kh_map_fit")
    return [_fit_dict(out[k]) for k in range(len(poses))]


class MapLocalizer:
    def __init__(self, params, laser, device: int = 0, max_batch: int = 32):
        """params: a dict of the fields of kh_mapper_params to override (AS STORED by karto::Mapper: variances squared), or None;
        laser: anything with n_beams, min_angle, ang_res, min_range, max_range, range_threshold (synth.Laser)"""
        p = capi.KhMapperParams()
        capi.lib().kh_mapper_params_default(C.byref(p))
        match_fields = {k for k, _ in capi.KhMatchParams._fields_}
        for k, v in (params or {}).items():
            if k in match_fields:
                setattr(p.match, k, v)
            elif hasattr(p, k):
                setattr(p, k, v)
            else:
                raise KeyError(k)
        self._params = p
        self._laser = _laser_of(laser)
        self.n_beams = laser.n_beams
        self._map = None
        self._h = C.c_void_p()
        capi.check(capi.lib().kh_map_localizer_create(C.byref(p), C.byref(self._laser), device, int(max_batch), C.byref(self._h)),
                   "kh_map_localizer_create")

    def set_map(self, source):
        """kh_map_localizer_set_map: a capi.KhMapView, an OccupancyGrid or a LiveMap.  The view is borrowed: set the map again after
        its source was updated, and keep the source alive (the localizer holds a reference to what it was given)."""
        v = _view_of(source)
        capi.check(capi.lib().kh_map_localizer_set_map(self._h, C.byref(v)), "kh_map_localizer_set_map")
        self._map = source
        return self

    def _ranges(self, ranges):
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        assert ranges.shape == (self.n_beams,)
        return ranges

    def relocalize(self, ranges, cap: int = 64, **params):
        """kh_map_localizer_relocalize.  params: fields of kh_map_relocalize_params over the defaults of this localizer's mapper
        parameters.  -> (hypotheses best first as MapHypothesis records, the summary as a dict)"""
        ranges = self._ranges(ranges)
        p = capi.KhMapRelocalizeParams()
        capi.lib().kh_map_relocalize_params_default(C.byref(self._params), C.byref(p))
        for k, v in params.items():
            if k == "center_xy":
                p.center_xy[0], p.center_xy[1] = float(v[0]), float(v[1])
            elif hasattr(p, k):
                setattr(p, k, v)
            else:
                raise KeyError(k)
        out = (capi.KhMapHyp * max(1, int(cap)))()
        summary = capi.KhMapRelocalizeSummary()
        capi.check(capi.lib().kh_map_localizer_relocalize(self._h, ranges.ctypes.data, C.byref(p), out, int(cap), C.byref(summary)),
                   "kh_map_localizer_relocalize")
        hyps = [MapHypothesis(h.index, (h.seed_cell[0], h.seed_cell[1]), h.heading, np.array(h.coarse_mean), np.array(h.coarse_cov).reshape(3, 3),
                              h.coarse_response, np.array(h.fine_mean), np.array(h.fine_cov).reshape(3, 3), h.fine_response,
                              np.array(h.robot_pose), _fit_dict(h.fit)) for h in out[:summary.n_returned]]
        return hyps, {k: getattr(summary, k) for k, _ in capi.KhMapRelocalizeSummary._fields_}

    def set_pose(self, robot_pose, odometric_pose=None):
        """kh_map_localizer_set_pose: the robot pose to track from, and the odometric pose it belongs to (default: the same)"""
        robot = np.ascontiguousarray(robot_pose, dtype=np.float64).copy()
        odom = robot if odometric_pose is None else np.ascontiguousarray(odometric_pose, dtype=np.float64).copy()
        capi.check(capi.lib().kh_map_localizer_set_pose(self._h, robot.ctypes.data, odom.ctypes.data), "kh_map_localizer_set_pose")

    def get_pose(self):
        robot, odom = np.zeros(3), np.zeros(3)
        capi.check(capi.lib().kh_map_localizer_get_pose(self._h, robot.ctypes.data, odom.ctypes.data), "kh_map_localizer_get_pose")
        return robot, odom

    def process(self, ranges, odometric_pose, changes=None, min_fit_score: float = 0.0):
        """kh_map_localizer_process: one tracking step; response and fit say how far to trust it.  -> TrackStep.
        changes: a map_changes.MapChanges layer (on this localizer's map, as a rule).  The step's scan is observed into it at the
        step's matched sensor pose when the fit has known > 0 and score >= min_fit_score -- a step that cannot be trusted teaches the
        layer nothing -- and the answer is a TrackStepObserved whose `labels` are the beams' (class, blocked), None where the scan was
        not observed."""
        ranges = self._ranges(ranges)
        odom = np.ascontiguousarray(odometric_pose, dtype=np.float64).copy()
        t = capi.KhMapTrack()
        capi.check(capi.lib().kh_map_localizer_process(self._h, ranges.ctypes.data, odom.ctypes.data, C.byref(t)), "kh_map_localizer_process")
        step = TrackStep(np.array(t.predicted_pose), np.array(t.robot_pose), np.array(t.sensor_pose), np.array(t.covariance).reshape(3, 3),
                         t.response, _fit_dict(t.fit))
        if changes is None:
            return step
        labels = None
        if step.fit["known"] > 0 and step.fit["score"] >= min_fit_score:
            labels = changes.observe(self._laser, ranges, step.sensor_pose)
        return TrackStepObserved(*step, labels)

    def stats(self) -> dict:
        st = capi.KhMapLocalizerStats()
        capi.check(capi.lib().kh_map_localizer_stats(self._h, C.byref(st)), "kh_map_localizer_stats")
        return {k: getattr(st, k) for k, _ in capi.KhMapLocalizerStats._fields_}

    def close(self):
        if self._h:
            capi.lib().kh_map_localizer_destroy(self._h)
            self._h = C.c_void_p()
        self._map = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
