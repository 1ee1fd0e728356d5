"""Merging mapping sessions into one occupancy map: the host-side mirror of slam_toolbox's merge_maps_kinematic
(src/merge_maps_kinematic.cpp) over kh_merge_* of libkartohip.so.

    merger = MapMerger(resolution=0.05)
    a = merger.add_submap(mapper)                 # a live Mapper (borrowed), or
    b = merger.add_submap("second.khms")          # a session file (Mapper.save), loaded and owned by the merger
    merger.move_submap(b, (x, y, yaw))            # the release of the reference's interactive marker, or
    merger.set_transform(b, (tx, ty, yaw))        # the correction itself
    grid = merger.merge()                         # occupancy_grid.OccupancyGrid over every submap's scans
    fits = merger.fit(b, [(tx, ty, yaw), ...])    # how well each correction places b among the others (counters, score)
    cands, times = merger.align(b, a)             # corrections found by relocalizing probe scans of b in a's map, best fit first

A merge never modifies a session: the correction is applied to the point readings inside the trace kernel, where the scans lie in
HBM.  Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

STATS = ("merges", "scans_traced", "beams_traced", "point_uploads", "range_uploads", "point_uploads_total", "range_uploads_total",
         "table_bytes")
FIT_STATS = ("fits", "candidates_total", "beam_candidates", "kernel_us")
FIT_DTYPE = np.dtype([(k, np.uint64) for k in ("pass_unknown", "pass_occupied", "pass_free", "hits_unknown", "hits_occupied", "hits_free",
                                               "agree", "conflict", "known")] + [("score", np.float64)])
assert FIT_DTYPE.itemsize == C.sizeof(capi.KhMergeFit)
ALIGN_DTYPE = np.dtype([("correction", np.float64, (3,)), ("probe_scan", np.int32), ("hypothesis", np.int32), ("fine_response", np.float64),
                        ("index", np.int32), ("enough", np.int32), ("fit", FIT_DTYPE)])
assert ALIGN_DTYPE.itemsize == C.sizeof(capi.KhMergeAlignCand)
ALIGN_TIMES = ("relocalize_ms", "reference_grid_ms", "fit_kernel_ms", "total_ms")


def _triple(t):
    t = np.ascontiguousarray(t, dtype=np.float64)
    assert t.shape == (3,)
    return t


class MapMerger:
    def __init__(self, resolution: float = 0.05, device: int = 0):
        self._h = C.c_void_p()
        self._borrowed = {}             # submap id -> the live Mapper (kept alive as long as the merger reads it)
        capi.check(capi.lib().kh_merge_create(int(device), float(resolution), C.byref(self._h)), "kh_merge_create")
        self.resolution = float(resolution)

    def add_submap(self, mapper_or_path) -> int:
        """a live mapper.Mapper (borrowed: it may go on processing scans between merges) or the path of a session file; returns the
        submap id.  The correction starts as the identity, the location at the centre of the submap's own grid."""
        sid = C.c_int32(-1)
        if isinstance(mapper_or_path, (str, bytes, os.PathLike)):
            capi.check(capi.lib().kh_merge_add_session(self._h, os.fsencode(mapper_or_path), C.byref(sid)), "kh_merge_add_session")
        else:
            capi.check(capi.lib().kh_merge_add_mapper(self._h, mapper_or_path._h, C.byref(sid)), "kh_merge_add_mapper")
            self._borrowed[sid.value] = mapper_or_path
        return sid.value

    def remove_submap(self, submap_id: int):
        capi.check(capi.lib().kh_merge_remove_submap(self._h, int(submap_id)), "kh_merge_remove_submap")
        self._borrowed.pop(int(submap_id), None)

    def num_submaps(self) -> int:
        return capi.lib().kh_merge_num_submaps(self._h)

    def submap_info(self, submap_id: int) -> dict:
        out = np.zeros(2, dtype=np.int32)
        capi.check(capi.lib().kh_merge_submap_info(self._h, int(submap_id), out), "kh_merge_submap_info")
        return {"n_scans": int(out[0]), "n_beams": int(out[1])}

    def set_transform(self, submap_id: int, transform):
        """the correction (tx, ty, yaw) of the submap"""
        capi.check(capi.lib().kh_merge_set_transform(self._h, int(submap_id), _triple(transform)), "kh_merge_set_transform")

    def transform(self, submap_id: int) -> np.ndarray:
        out = np.zeros(3)
        capi.check(capi.lib().kh_merge_get_transform(self._h, int(submap_id), out), "kh_merge_get_transform")
        return out

    def move_submap(self, submap_id: int, marker_pose):
        """processInteractiveFeedback on release: correction <- correction . inverse(translation(location)) . marker_pose"""
        capi.check(capi.lib().kh_merge_move_submap(self._h, int(submap_id), _triple(marker_pose)), "kh_merge_move_submap")

    def location(self, submap_id: int) -> np.ndarray:
        out = np.zeros(3)
        capi.check(capi.lib().kh_merge_get_location(self._h, int(submap_id), out), "kh_merge_get_location")
        return out

    def transformed_scan(self, submap_id: int, index: int) -> dict:
        """what transformScan leaves on scan `index` of the submap's scans (scan-id order): corrected / odometric / barycenter pose
        (3,), box (min x, min y, max x, max y), points (n_beams, 2)"""
        n = self.submap_info(submap_id)["n_beams"]
        out = {"corrected": np.zeros(3), "odometric": np.zeros(3), "barycenter": np.zeros(3), "box": np.zeros(4), "points": np.zeros((n, 2))}
        capi.check(capi.lib().kh_merge_get_scan(self._h, int(submap_id), int(index), *(out[k].ctypes.data for k in
                                                ("corrected", "odometric", "barycenter", "box", "points"))), "kh_merge_get_scan")
        return out

    def submap_map(self, submap_id: int, min_pass_through: int = 2, occupancy_threshold: float = 0.1):
        """the submap's own, untransformed grid (what addSubmapCallback publishes as /map_N)"""
        from .occupancy_grid import OccupancyGrid
        h = C.c_void_p()
        capi.check(capi.lib().kh_merge_build_submap(self._h, int(submap_id), int(min_pass_through), float(occupancy_threshold), C.byref(h)),
                   "kh_merge_build_submap")
        return OccupancyGrid.from_handle(h, self.resolution)

    def merge(self, min_pass_through: int = 2, occupancy_threshold: float = 0.1):
        """mergeMapCallback: one OccupancyGrid over the scans of every submap, each under its correction"""
        from .occupancy_grid import OccupancyGrid
        h = C.c_void_p()
        capi.check(capi.lib().kh_merge_build(self._h, int(min_pass_through), float(occupancy_threshold), C.byref(h)), "kh_merge_build")
        return OccupancyGrid.from_handle(h, self.resolution)

    def fit(self, submap_id: int, corrections, min_pass_through: int = 2, occupancy_threshold: float = 0.1) -> np.ndarray:
        """kh_merge_fit: candidate corrections (n, 3) of ONE submap against the merge of all the others -> structured array (n,) of
        FIT_DTYPE: the six counters by cell state, agree / conflict / known and score = agree / known.  Nothing of the merger changes."""
        c = np.ascontiguousarray(corrections, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(c.shape[0], dtype=FIT_DTYPE)
        capi.check(capi.lib().kh_merge_fit(self._h, int(submap_id), c.shape[0], c.ctypes.data, int(min_pass_through), float(occupancy_threshold),
                                           out.ctypes.data_as(C.POINTER(capi.KhMergeFit))), "kh_merge_fit")
        return out

    def fit_stats(self) -> dict:
        out = np.zeros(4, dtype=np.int64)
        capi.check(capi.lib().kh_merge_fit_stats(self._h, out), "kh_merge_fit_stats")
        return dict(zip(FIT_STATS, out.tolist()))

    def align_params(self, target: int, **params):
        """kh_merge_align_params_default for `target`, then params: fields of kh_merge_align_params, and of its kh_relocalize_params
        (seed_spacing, n_headings, max_base, center_xy, radius) by their own names"""
        p = capi.KhMergeAlignParams()
        capi.lib().kh_merge_align_params_default(self._h, int(target), C.byref(p))
        for k, v in params.items():
            if k == "center_xy":
                p.relocalize.center_xy[0], p.relocalize.center_xy[1] = float(v[0]), float(v[1])
            elif k in ("n_probes", "top_k", "min_known", "min_pass_through", "occupancy_threshold"):
                setattr(p, k, v)
            elif k in ("seed_spacing", "n_headings", "max_base", "radius"):
                setattr(p.relocalize, k, v)
            else:
                raise KeyError(k)
        return p

    def align(self, moving: int, target: int, cap: int = 256, **params):
        """kh_merge_align: corrections of `moving` proposed by relocalizing probe scans of it in `target`'s map, ranked by how the
        whole submap fits all the others.  Returns (candidates, times): a structured array of ALIGN_DTYPE, best first (candidate 0
        -- index 0 -- is the current correction), and the call's split in ms.  Nothing is applied: set_transform does that."""
        p = self.align_params(target, **params)
        out = np.zeros(max(1, int(cap)), dtype=ALIGN_DTYPE)
        n, times = C.c_int32(0), np.zeros(4)
        capi.check(capi.lib().kh_merge_align(self._h, int(moving), int(target), C.byref(p), out.ctypes.data_as(C.POINTER(capi.KhMergeAlignCand)),
                                             int(cap), C.byref(n), times.ctypes.data), "kh_merge_align")
        return out[:min(int(cap), n.value)].copy(), dict(zip(ALIGN_TIMES, times.tolist()), n_candidates=n.value)

    def stats(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        capi.check(capi.lib().kh_merge_stats(self._h, out), "kh_merge_stats")
        return dict(zip(STATS, out.tolist()))

    def close(self):
        if self._h:
            capi.lib().kh_merge_destroy(self._h)
            self._h = C.c_void_p()
            self._borrowed.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
