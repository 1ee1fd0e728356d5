"""TEST INFRASTRUCTURE (not a test): the arithmetic of a session merge, restated in numpy / python floats.

A correction is T = (tx, ty, yaw); c = cos(yaw) and s = sin(yaw) are libm's, each called on its own (python's math module).

    point        x' = (c x - s y) + tx,  y' = (s x + c y) + ty
    pose         position as a point, heading' = NormalizeAngle(heading + yaw)        (karto's math::NormalizeAngle, Math.h:181-202)
    A . B        (A.x + (cA B.x - sA B.y), A.y + (sA B.x + cA B.y), NormalizeAngle(A.yaw + B.yaw))
    inverse(A)   yaw' = NormalizeAngle(-A.yaw), c', s' of yaw': (-(c' A.x - s' A.y), -(s' A.x + c' A.y), yaw')
    release      correction <- (correction . inverse((location x, location y, 0))) . marker;  location <- (marker x, marker y,
                 location yaw + marker yaw)                                            (processInteractiveFeedback :313-352)
    box          min / max of the four transformed corners of the scan's own box       (transformScan :206-221)
    sensor       GetSensorAt(transformed corrected pose) with the submap's laser offset (Karto.h:5566-5569, 2946-3024)

Every double operation is one IEEE operation in the order written; numpy evaluates elementwise a * b - c * d as two products and
one difference, without contraction.

A SUBMAP here is a dict: "laser" (n_beams, min_range, max_range, range_threshold, offset) and "scans", a list of dicts with
"ranges" (n,), "points" (n, 2) unfiltered point readings, "corrected" (3,), "odometric" (3,), "barycenter" (3,) (GetBarycenterPose)
and "box" (min x, min y, max x, max y).  merged_grid ends at oracle.karto.occupancy_from_scans, which tests/test_occupancy_*.py pin
to the reference's OccupancyGrid::CreateFromScans."""
from __future__ import annotations

import ctypes
import math

import numpy as np

KT_PI = 3.14159265358979323846
KT_2PI = 6.28318530717958647692
IDENTITY = (0.0, 0.0, 0.0)


def normalize_angle(angle: float) -> float:
    """math::NormalizeAngle, Math.h:181-202"""
    angle = float(angle)
    while angle < -KT_PI:
        if angle < -KT_2PI:
            angle += float(int(angle / -KT_2PI)) * KT_2PI
        else:
            angle += KT_2PI
    while angle > KT_PI:
        if angle > KT_2PI:
            angle -= float(int(angle / KT_2PI)) * KT_2PI
        else:
            angle -= KT_2PI
    return angle


def cos_sin(yaw: float):
    return math.cos(float(yaw)), math.sin(float(yaw))


def transform_points(t, xy):
    """xy (..., 2) -> transformed copy"""
    c, s = cos_sin(t[2])
    xy = np.asarray(xy, dtype=np.float64)
    x, y = xy[..., 0], xy[..., 1]
    with np.errstate(invalid="ignore"):                 # (readings of infinite range: inf - inf)
        return np.stack([(c * x - s * y) + float(t[0]), (s * x + c * y) + float(t[1])], axis=-1)


def transform_point(t, x: float, y: float):
    c, s = cos_sin(t[2])
    return (c * float(x) - s * float(y)) + float(t[0]), (s * float(x) + c * float(y)) + float(t[1])


def transform_pose(t, pose):
    x, y = transform_point(t, pose[0], pose[1])
    return np.array([x, y, normalize_angle(float(pose[2]) + float(t[2]))])


def compose(a, b):
    ca, sa = cos_sin(a[2])
    ax, ay, bx, by = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    return np.array([ax + (ca * bx - sa * by), ay + (sa * bx + ca * by), normalize_angle(float(a[2]) + float(b[2]))])


def inverse(a):
    yaw = normalize_angle(-float(a[2]))
    c, s = cos_sin(yaw)
    ax, ay = float(a[0]), float(a[1])
    return np.array([-(c * ax - s * ay), -(s * ax + c * ay), yaw])


def release(correction, location, marker):
    """the release of the marker at `marker` -> (new correction, new location)"""
    previous = (float(location[0]), float(location[1]), 0.0)
    new_correction = compose(compose(correction, inverse(previous)), marker)
    return new_correction, np.array([float(marker[0]), float(marker[1]), float(location[2]) + float(marker[2])])


def loose_box(t, box):
    """box = (min x, min y, max x, max y) -> the axis-aligned box of its four transformed corners"""
    corners = [transform_point(t, box[0], box[1]), transform_point(t, box[2], box[3]), transform_point(t, box[2], box[1]),
               transform_point(t, box[0], box[3])]
    xs, ys = [p[0] for p in corners], [p[1] for p in corners]
    return np.array([min(xs), min(ys), max(xs), max(ys)])


_libm = None


def _sincos(a: float):
    """glibc's sincos: what the reference's Release build calls for a cos / sin pair of one angle (tests/test_abi.py)"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        _libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    s, c = ctypes.c_double(), ctypes.c_double()
    _libm.sincos(float(a), ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


def sensor_at(robot, offset=(0.0, 0.0, 0.0)):
    """LocalizedRangeScan::GetSensorAt: Transform(robot pose).TransformPose(laser offset pose), Karto.h:2946-3024 with
    Matrix3::FromAxisAngle about z (:2482-2511)"""
    rx, ry, rh = (float(v) for v in robot)
    ox, oy, oh = (float(v) for v in offset)
    if rx == 0.0 and ry == 0.0 and rh == 0.0:             # Transform(Pose2(), rPose2) with equal poses: the identity
        return np.array([0.0 + ox, 0.0 + oy, normalize_angle(oh + 0.0)])
    s, c = _sincos(rh - 0.0)
    versine = 1.0 - c
    m00, m01, m02 = 0.0 * 0.0 * versine + c, 0.0 * 0.0 * versine - 1.0 * s, 0.0 * 1.0 * versine + 0.0 * s
    m10, m11, m12 = 0.0 * 0.0 * versine + 1.0 * s, 0.0 * 0.0 * versine + c, 0.0 * 1.0 * versine - 0.0 * s
    x = rx + (m00 * ox + m01 * oy + m02 * oh)
    y = ry + (m10 * ox + m11 * oy + m12 * oh)
    return np.array([x, y, normalize_angle(oh + (rh - 0.0))])


def transformed_scan(t, scan, laser_offset=(0.0, 0.0, 0.0)):
    """what transformScan leaves on one scan, plus the sensor pose the ray trace starts at"""
    corrected = transform_pose(t, scan["corrected"])
    return {"corrected": corrected, "odometric": transform_pose(t, scan["odometric"]), "barycenter": transform_pose(t, scan["barycenter"]),
            "box": loose_box(t, scan["box"]), "points": transform_points(t, scan["points"]), "sensor": sensor_at(corrected, laser_offset)}


def round_half_away(v: float) -> float:
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


def dimensions(boxes, resolution):
    """OccupancyGrid::ComputeDimensions (Karto.h:6086-6112) over boxes (min x, min y, max x, max y) -> width, height, offset"""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    min_x, min_y, max_x, max_y = boxes[:, 0].min(), boxes[:, 1].min(), boxes[:, 2].max(), boxes[:, 3].max()
    scale = 1.0 / float(resolution)
    return (int(round_half_away(float(max_x - min_x) * scale)), int(round_half_away(float(max_y - min_y) * scale)),
            np.array([min_x, min_y]))


def initial_location(submap, resolution):
    """the centre of the submap's own grid (addSubmapCallback :115-122)"""
    w, h, off = dimensions([s["box"] for s in submap["scans"]], resolution)
    return np.array([float(off[0]) + float(w) * float(resolution) / 2.0, float(off[1]) + float(h) * float(resolution) / 2.0, 0.0])


def merged_dimensions(submaps, transforms, resolution):
    return dimensions([loose_box(t, s["box"]) for sm, t in zip(submaps, transforms) for s in sm["scans"]], resolution)


def submap_counters(submap, t, width, height, offset, resolution):
    """pass / hit counters of ONE submap's transformed scans on a given grid, through the occupancy oracle"""
    from oracle import karto
    laser = submap["laser"]
    scans = []
    for s in submap["scans"]:
        ts = transformed_scan(t, s, getattr(laser, "offset", (0.0, 0.0, 0.0)))
        scans.append(karto.Scan(s["ranges"], ts["sensor"], points=ts["points"]))
    _, passes, hits = karto.occupancy_from_scans(width, height, offset, resolution, scans, laser)
    return passes, hits


def update_cells(passes, hits, min_pass_through=2, occupancy_threshold=0.1):
    """OccupancyGrid::Update / UpdateCell, Karto.h:6240-6274"""
    cells = np.zeros(passes.shape, dtype=np.uint8)
    seen = passes > min_pass_through
    ratio = np.divide(hits.astype(np.float64), passes.astype(np.float64), out=np.zeros(passes.shape), where=seen)
    cells[seen & (ratio > occupancy_threshold)] = 100
    cells[seen & ~(ratio > occupancy_threshold)] = 255
    return cells


def merged_grid(submaps, transforms, resolution, min_pass_through=2, occupancy_threshold=0.1):
    """-> dict(width, height, offset, cells, passes, hits): every submap's scans transformed, traced by the occupancy oracle on the
    common dimensions one submap at a time (one laser each); the counters add up; then Update's rule"""
    width, height, offset = merged_dimensions(submaps, transforms, resolution)
    passes = hits = None
    for sm, t in zip(submaps, transforms):
        if not sm["scans"]:
            continue
        p, h = submap_counters(sm, t, width, height, offset, resolution)
        passes = p.copy() if passes is None else passes + p
        hits = h.copy() if hits is None else hits + h
    return {"width": width, "height": height, "offset": offset, "passes": passes, "hits": hits,
            "cells": update_cells(passes, hits, min_pass_through, occupancy_threshold)}
