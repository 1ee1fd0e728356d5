"""The two maps the alignment tests share (tests/test_map_align_rule_oracle.py on the CPU, tests/test_map_align_gpu.py): scans 0 .. 5 of
the small map of tests/relocalize_cases.py as the target, scans 2 .. 7 with their poses carried by a known rigid G as the moving map
-- the same place in a frame that G carries, so the correction that aligns it is inverse(G) -- and the setting of the alignment."""
from __future__ import annotations

import math

import numpy as np

import map_localize_cases as lc
import map_localize_rule as ml
import merge_rule
import relocalize_cases as rc

G = (0.73, -0.41, 0.3)
SETTING = dict(probe_spacing=2.0, n_probes=3, top_k=4, max_unknown=20)
RELOCALIZE = dict(seed_spacing=2.0, n_headings=8)             # the whole target map
_cache = {}


def maps():
    """(target MapOf, moving MapOf)"""
    if "maps" not in _cache:
        from common import LASER
        sm = rc.small_map()
        target = lc.occupancy_map(sm.ranges[0:6], sm.poses[0:6], LASER)
        moved = np.array([merge_rule.transform_pose(G, p) for p in sm.poses[2:8]])
        _cache["maps"] = (target, lc.occupancy_map(sm.ranges[2:8], moved, LASER))
    return _cache["maps"]


def from_the_truth(correction, moving):
    """how far `correction` carries the centre of the moving map from where inverse(G) carries it (m), and the heading between them (rad)"""
    centre = (moving.offset[0] + 0.5 * moving.width * lc.RESOLUTION, moving.offset[1] + 0.5 * moving.height * lc.RESOLUTION)
    truth = merge_rule.inverse(G)
    a, b = merge_rule.transform_point(correction, *centre), merge_rule.transform_point(truth, *centre)
    return math.hypot(a[0] - b[0], a[1] - b[1]), abs(ml.normalize_angle(float(correction[2]) - float(truth[2])))
