"""Python mirror of the node-decay scoring of slam_toolbox::LifelongSlamToolbox (computeScores and the metrics,
src/experimental/slam_toolbox_lifelong.cpp:199-329, 373-478) over the C ABI (kh_lifelong_scores, kh_lifelong_scores_resident)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


def _box(s, keep):
    b = capi.KhScanBox()
    b.barycenter[0], b.barycenter[1] = float(s.barycenter[0]), float(s.barycenter[1])
    b.bbox_size[0], b.bbox_size[1] = float(s.bbox_size[0]), float(s.bbox_size[1])
    b.unique_id, b.n_edges, b.score = int(s.unique_id), int(s.n_edges), float(s.score)
    pts = np.ascontiguousarray(np.asarray(s.points, dtype=np.float64).reshape(-1, 2))
    keep.append(pts)
    b.n_points = pts.shape[0]
    b.points_xy = pts.ctypes.data_as(C.POINTER(C.c_double))
    return b


def computeScores(reference, candidates, params=None, device: int = 0):
    """-> (kept, iou, area_overlap, reading_overlap, score) arrays over `candidates`.  `reference` / candidates are
    objects with barycenter, bbox_size, points (filtered readings), unique_id, n_edges, score; `params` any object
    with the kh_decay_params field names (defaults: slam_toolbox_lifelong.cpp:60-100)."""
    p = capi.KhDecayParams()
    capi.lib().kh_decay_params_default(C.byref(p))
    if params is not None:
        for name, _ in capi.KhDecayParams._fields_:
            if hasattr(params, name):
                setattr(p, name, getattr(params, name))
    keep = []
    ref = _box(reference, keep)
    n = len(candidates)
    arr = (capi.KhScanBox * max(n, 1))(*[_box(c, keep) for c in candidates])
    kept = np.zeros(n, dtype=np.int32)
    iou, area, reading, score = (np.zeros(n) for _ in range(4))
    capi.check(capi.lib().kh_lifelong_scores(device, C.byref(ref), n, arr, C.byref(p), kept.ctypes.data, iou.ctypes.data,
                                             area.ctypes.data, reading.ctypes.data, score.ctypes.data), "kh_lifelong_scores")
    return kept.astype(bool), iou, area, reading, score


def pack_mask(passed) -> np.ndarray:
    """one bit per reading, bit i of word i // 64 set where passed[i]: the filter mask of kh_lifelong_scores_resident"""
    passed = np.asarray(passed, dtype=bool)
    words = np.zeros((passed.shape[0] + 63) // 64, dtype=np.uint64)
    for i in np.flatnonzero(passed):
        words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return words


def computeScoresResident(reference, candidates, readings, passed, params=None, device: int = 0):
    """computeScores in the form the mapper calls (kh_lifelong_scores_resident): readings[k] = the (n_scan, 2) UNFILTERED point
    readings of candidate k (None = not counted), passed[k] = n_scan booleans, True where the reading passed the range filter.
    The candidates' own `points` are not read; the number of readings that count is passed[k].sum()."""
    p = capi.KhDecayParams()
    capi.lib().kh_decay_params_default(C.byref(p))
    if params is not None:
        for name, _ in capi.KhDecayParams._fields_:
            if hasattr(params, name):
                setattr(p, name, getattr(params, name))
    keep = []
    ref = _box(reference, keep)
    n = len(candidates)
    n_scan = len(passed[0]) if n else 1
    arr = (capi.KhScanBox * max(n, 1))()
    pts = (C.c_void_p * max(n, 1))()
    msk = (C.c_void_p * max(n, 1))()
    for k, c in enumerate(candidates):
        arr[k] = _box(c, keep)
        arr[k].points_xy = None
        arr[k].n_points = int(np.asarray(passed[k], dtype=bool).sum())
        assert len(passed[k]) == n_scan
        words = pack_mask(passed[k])
        keep.append(words)
        msk[k] = words.ctypes.data
        if readings[k] is not None:
            r = np.ascontiguousarray(readings[k], dtype=np.float64).reshape(-1, 2)
            assert r.shape[0] == n_scan
            keep.append(r)
            pts[k] = r.ctypes.data
    kept = np.zeros(n, dtype=np.int32)
    iou, area, reading, score = (np.zeros(n) for _ in range(4))
    capi.check(capi.lib().kh_lifelong_scores_resident(device, C.byref(ref), n, arr, pts, msk, n_scan, C.byref(p), kept.ctypes.data,
                                                      iou.ctypes.data, area.ctypes.data, reading.ctypes.data, score.ctypes.data),
               "kh_lifelong_scores_resident")
    return kept.astype(bool), iou, area, reading, score
