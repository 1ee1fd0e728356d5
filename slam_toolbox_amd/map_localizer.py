"""Localizing in a map alone over the C ABI (kh_map_seeds, kh_map_fit, kh_map_localizer_*; include/karto_hip.h):
the map is a device view of cell states -- an OccupancyGrid (built, merged, or from_nav of a shipped nav_msgs/OccupancyGrid), a
LiveMap, or a hand-filled capi.KhMapView -- and nothing else: no scans, no pose graph.

    loc = MapLocalizer(dict(loop_search_space_dimension=4.0), laser)
    loc.set_map(OccupancyGrid.from_nav(nav, origin, resolution))
    hyps, summary = loc.relocalize(ranges)                 # where was this scan taken?
    loc.set_pose(hyps[0].robot_pose, odometric_pose)
    step = loc.process(next_ranges, next_odometric_pose)   # ... and from there on, scan by scan
    cast = loc.expected(step.sensor_pose)                  # what the map expects every beam to measure there (kh_map_raycast)
    candidates, _ = loc.align(other_map)                   # where a second map lies in this one (kh_map_align; section 7m)
    merged = loc.merge(other_map, candidates[0].correction)   # ... and the two as one map (kh_map_merge_*; section 7n)
    refined, _ = loc.refine(ranges, hyps[0].fine_mean, truncate_cells=6)   # a pose descended on the map's distance field (section 7o)

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
MapCast = namedtuple("MapCast", "ranges codes cells steps kernel_ms")
AlignCandidate = namedtuple("AlignCandidate", "correction probe_seed hypothesis fine_response index enough fit")


def _fit_dict(f):
    return {k: getattr(f, k) for k in FIT_FIELDS}


def _view_of(source):
    """a capi.KhMapView, or anything with .view() (OccupancyGrid, LiveMap, MapChanges) or a .view that is one (MapMerge)"""
    if isinstance(source, capi.KhMapView):
        return source
    return source.view() if callable(source.view) else source.view


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


def ray_no_return(laser):
    """the reading of a beam that found nothing: the next double above range_threshold where the laser's maximum_range lies above that
    (dropped from the point readings, still clearing the beam in AddScan), else NaN"""
    L = laser if isinstance(laser, capi.KhLaser) else _laser_of(laser)
    above = float(np.nextafter(np.float64(L.range_threshold), np.inf))
    return above if above < L.maximum_range else float("nan")


def map_raycast(view, laser, poses, max_unknown=-1, no_return=None):
    """kh_map_raycast: the scan the map would produce at each of `poses` (n, 3) sensor poses -> MapCast of arrays with a leading pose
    axis: ranges (n, n_beams) float64, codes (KH_RAY_FREE / HIT / UNKNOWN), cells (n, n_beams, 2) lattice i, j, steps; kernel_ms.
    max_unknown: unknown cells a beam may pass (-1: any number).  no_return: the range of a beam without a hit (default ray_no_return)"""
    v = _view_of(view)
    L = laser if isinstance(laser, capi.KhLaser) else _laser_of(laser)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((max(1, len(poses)), L.n_beams), dtype=capi.RAY_DTYPE)
    ms = C.c_double()
    capi.check(capi.lib().kh_map_raycast(C.byref(v), C.byref(L), len(poses), poses.ctypes.data, int(max_unknown),
                                         ray_no_return(L) if no_return is None else float(no_return), out.ctypes.data, C.byref(ms)), "kh_map_raycast")
    out = out[:len(poses)]
    return MapCast(out["range"].copy(), out["code"].copy(), out["cell"].copy(), out["steps"].copy(), ms.value)


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

    def expected(self, sensor_pose, max_unknown=-1, no_return=None):
        """kh_map_raycast against the localizer's map: the scan expected at `sensor_pose` (3,) or poses (n, 3) -> MapCast, to set
        beside the measured ranges of a tracking step (TrackStep.sensor_pose)"""
        if self._map is None:
            raise capi.KartoHipError(capi.KH_ERR_NOT_FOUND, "MapLocalizer.expected: no map set")
        return map_raycast(self._map, self._laser, sensor_pose, max_unknown, no_return)

    def align(self, moving, cap: int = 64, **params):
        """kh_map_align: places the map `moving` (a capi.KhMapView, an OccupancyGrid or a LiveMap) in the localizer's map, with no scan
        of either.  params: fields of kh_map_align_params over the defaults of this localizer; `relocalize` a dict of fields of
        kh_map_relocalize_params.  -> (candidates best first as AlignCandidate records: correction = moving map -> this map;
        times_ms: seeds + cast, relocalizations, fits, the call)"""
        v = _view_of(moving)
        p = capi.KhMapAlignParams()
        capi.lib().kh_map_align_params_default(self._h, C.byref(p))
        for k, value in params.items():
            if k == "initial":
                p.initial[0], p.initial[1], p.initial[2] = (float(x) for x in value)
            elif k == "relocalize":
                for rk, rv in value.items():
                    if rk == "center_xy":
                        p.relocalize.center_xy[0], p.relocalize.center_xy[1] = float(rv[0]), float(rv[1])
                    elif hasattr(p.relocalize, rk):
                        setattr(p.relocalize, rk, rv)
                    else:
                        raise KeyError(rk)
            elif hasattr(p, k):
                setattr(p, k, value)
            else:
                raise KeyError(k)
        out = (capi.KhMapAlignCand * max(1, int(cap)))()
        n, times = C.c_int32(), np.zeros(4)
        capi.check(capi.lib().kh_map_align(self._h, C.byref(v), C.byref(p), out, int(cap), C.byref(n), times.ctypes.data), "kh_map_align")
        cands = [AlignCandidate(np.array(c.correction), c.probe_seed, c.hypothesis, c.fine_response, c.index, bool(c.enough), _fit_dict(c.fit))
                 for c in out[:min(n.value, int(cap))]]
        return cands, times

    def merge(self, moving, correction, **kw):
        """kh_map_merge_create with the localizer's map as the target: `moving` laid into it under `correction` (an AlignCandidate's, as
        `align` returns them).  kw: footprint, conflict, grow.  -> map_merge.MapMerge; its .view is the merged map on this map's lattice"""
        from .map_merge import MapMerge
        if self._map is None:
            raise capi.KartoHipError(capi.KH_ERR_NOT_FOUND, "MapLocalizer.merge: no map set")
        return MapMerge(self._map, moving, correction, **kw)

    def field(self, **params):
        """kh_map_field_create on the localizer's map: its distance field (a snapshot).  params: max_distance, obstacles.
        -> map_field.MapField"""
        from .map_field import MapField
        if self._map is None:
            raise capi.KartoHipError(capi.KH_ERR_NOT_FOUND, "MapLocalizer.field: no map set")
        return MapField(self._map, **params)

    def regions(self, max_distance: float = 2.0, **params):
        """kh_map_regions_create on the localizer's map, through a distance field made for this call that reaches at least
        min_clearance.  params: fields of kh_map_regions_params.  -> map_regions.MapRegions (it does not borrow the field)"""
        f = self.field(max_distance=max(float(max_distance), float(params.get("min_clearance", 0.0))))
        try:
            return f.regions(**params)
        finally:
            f.close()

    def travel(self, max_distance: float = 2.0, **params):
        """kh_map_travel_create on the localizer's map, through a distance field made for this call that reaches max(Rc, Rt): the
        larger of min_clearance and -- with a cost_weight above 0 -- the inflation radius.  params: fields of kh_map_travel_params
        and of its kh_inflation_params.  -> map_travel.MapTravel (it does not borrow the field)"""
        from .map_travel import reach_of
        f = self.field(max_distance=max(float(max_distance), reach_of(params)))
        try:
            return f.travel(**params)
        finally:
            f.close()

    def visibility(self, **params):
        """kh_map_visibility_create on the localizer's map and laser: what a sensor pose would see of the map.  params: fields of
        kh_visibility_params.  -> map_visibility.MapVisibility (it borrows the map's cells, as the localizer does)"""
        from .map_visibility import MapVisibility
        if self._map is None:
            raise capi.KartoHipError(capi.KH_ERR_NOT_FOUND, "MapLocalizer.visibility: no map set")
        return MapVisibility(self._map, self._laser, **params)

    def footprint(self, vertices, max_distance: float = 2.0, **params):
        """kh_map_footprint_create on the localizer's map, through a distance field made for this call (max_distance, and `params`:
        obstacles): its values are the records' min_d2.  -> map_footprint.MapFootprint (it does not borrow the field)"""
        f = self.field(max_distance=max_distance, **params)
        try:
            return f.footprint(vertices)
        finally:
            f.close()

    def refine(self, ranges, sensor_pose, field=None, max_distance: float = 2.0, **params):
        """kh_map_field_refine of `sensor_pose` (3,) or poses (n, 3) -- a hypothesis' or a tracking step's -- with this localizer's
        laser, on `field` (a MapField of the current map, as `field()` makes them) or on one made for this call.  params: fields of
        kh_field_refine_params.  -> (list of map_field.Refined, times_ms)"""
        own = field is None
        f = self.field(max_distance=max_distance) if own else field
        try:
            return f.refine(self._ranges(ranges), sensor_pose, self._laser, **params)
        finally:
            if own:
                f.close()

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
