"""TEST INFRASTRUCTURE (not a test): the rule of kh_map_visibility_*  in numpy on the CPU oracle -- what a sensor
standing at a pose would see of a map.  It reads nothing of the library; the walk is tests/map_raycast_rule.py's, lattice and TraceLine
tests/map_localize_rule.py's.

  beam cells  beam b of sensor pose p: map_raycast_rule.walk(view, c0, c1, max_unknown) -> (cell, s_end, code); the visited cells are
              beam_cells(c0, c1)[0 .. s_end], the leaving cell included (the HIT cell, the unknown cell that exceeded the budget, c1 on FREE)
  Seen(p)     the window cells among the visited cells of all beams of p; a cell outside the window is never counted; state 100 is
              occupied, 255 free, every other unknown; the sensor's own cell is treated like any other
  covered     one bit per window cell: cleared on create and by clear(), commit(poses) ORs Seen(p) of every pose into it
  record      seen_free / _occupied / _unknown over Seen(p); new_* over Seen(p) minus covered as it stands at the call;
              gain = w_unknown * new_unknown + w_free * new_free + w_occupied * new_occupied; beams_free / _hit / _unknown by code
  reach       floor(range_threshold * scale) + 2 cells bounds the Chebyshev distance from c0 to any c1; above 511 the laser is refused
  select      rounds r = 0 .. k - 1: among the candidates not yet picked the largest gain against the mask as it stands, ties to the
              smallest index; below min_gain the selection ends with r picks; else (index, gain) is recorded and the pose committed.
              The mask is not cleared first and is left holding the picks.
"""
from __future__ import annotations

import math

import numpy as np

import map_localize_rule as ml
import map_raycast_rule as rr

PARAMS = dict(max_unknown=20, w_unknown=1, w_free=0, w_occupied=0)
FIELDS = ("seen_free", "seen_occupied", "seen_unknown", "new_free", "new_occupied", "new_unknown", "gain", "beams_free", "beams_hit", "beams_unknown")
DTYPE = np.dtype([(k, np.uint32) for k in FIELDS])
MAX_REACH, MAX_POSES, MAX_PICKS, MAX_BEAMS = 511, 65536, 4096, 1 << 24


class Refused(ValueError):
    pass


def reach_of(laser, scale):
    return int(math.floor(np.float64(laser.range_threshold) * np.float64(scale))) + 2


def bitmap_bytes(reach):
    side = 2 * reach + 1
    return 4 * ((side * side + 31) // 32)


def params_check(view, laser, params):
    """-> reach; Refused (with the name of the first refusal, in the library's order) where the library answers KH_ERR_INVALID_ARG"""
    if laser.n_beams < 1 or ml.fit_refused(view, laser, (view["anchor"][0], view["anchor"][1], 0.0)) or math.isnan(laser.min_range) or math.isnan(laser.max_range) or \
            not (math.isfinite(laser.min_angle) and math.isfinite(laser.ang_res)):
        raise Refused("laser")
    if params["max_unknown"] < -1:
        raise Refused("max_unknown")
    w = [params[k] for k in ("w_unknown", "w_free", "w_occupied")]
    if any(v < 0 or v > 255 for v in w) or not any(w):
        raise Refused("weights")
    if reach_of(laser, view["scale"]) > MAX_REACH:
        raise Refused("reach")
    return reach_of(laser, view["scale"])


def select_check(n, k, min_gain):
    if not 1 <= n <= MAX_POSES:
        raise Refused("n")
    if not 1 <= k <= min(n, MAX_PICKS):
        raise Refused("k")
    if min_gain < 1:
        raise Refused("min_gain")


def seen(view, laser, pose, max_unknown):
    """one sensor pose -> (Seen(p) as a (height, width) bool array, the beams by code (FREE, HIT, UNKNOWN))"""
    pose = np.asarray(pose, dtype=np.float64)
    assert not rr.cast_refused(view, laser, pose, max_unknown)
    ax, ay, scale = view["anchor"][0], view["anchor"][1], view["scale"]
    c0 = (ml.lattice_cell(pose[0], ax, scale), ml.lattice_cell(pose[1], ay, scale))
    out = np.zeros((view["height"], view["width"]), dtype=bool)
    beams = [0, 0, 0]
    reach = reach_of(laser, scale)
    for p in rr.far_points(laser, pose):
        c1 = (ml.lattice_cell(p[0], ax, scale), ml.lattice_cell(p[1], ay, scale))
        assert max(abs(c1[0] - c0[0]), abs(c1[1] - c0[1])) <= reach, "the reach bounds every far cell"
        _, _, s_end, code = rr.walk(view, c0, c1, max_unknown)
        x, y = rr.beam_cells(c0, c1)
        wx, wy = x[:s_end + 1] - view["ox"], y[:s_end + 1] - view["oy"]
        inside = (wx >= 0) & (wx < view["width"]) & (wy >= 0) & (wy < view["height"])
        out[wy[inside], wx[inside]] = True
        beams[code] += 1
    return out, tuple(beams)


class Visibility:
    """the handle: a view, a laser, parameters and the covered mask.  Seen(p) does not depend on the mask: it is kept per pose."""

    def __init__(self, view, laser, **params):
        self.view, self.laser = view, laser
        self.params = dict(PARAMS, **params)
        self.reach = params_check(view, laser, self.params)
        self.mask = np.zeros((view["height"], view["width"]), dtype=bool)
        self._seen = {}

    def set_map(self, view):
        a, b = self.view, view
        if any(a[k] != b[k] for k in ("ox", "oy", "width", "height", "scale")) or tuple(a["anchor"]) != tuple(b["anchor"]):
            raise Refused("window")
        self.view, self._seen = view, {}

    def clear(self):
        self.mask[:] = False

    def seen(self, pose):
        key = tuple(float(v) for v in pose)
        if key not in self._seen:
            self._seen[key] = seen(self.view, self.laser, pose, self.params["max_unknown"])
        return self._seen[key]

    def commit(self, poses):
        for pose in np.asarray(poses, dtype=np.float64).reshape(-1, 3):
            self.mask |= self.seen(pose)[0]

    def record(self, pose):
        cells = self.view["cells"][:, :self.view["width"]]
        s, beams = self.seen(pose)
        occupied, free = cells == rr.OCCUPIED_STATE, cells == rr.FREE_STATE
        unknown = ~occupied & ~free
        fresh = s & ~self.mask
        r = np.zeros((), dtype=DTYPE)
        r["seen_free"], r["seen_occupied"], r["seen_unknown"] = (s & free).sum(), (s & occupied).sum(), (s & unknown).sum()
        r["new_free"], r["new_occupied"], r["new_unknown"] = (fresh & free).sum(), (fresh & occupied).sum(), (fresh & unknown).sum()
        p = self.params
        gain = p["w_unknown"] * int(r["new_unknown"]) + p["w_free"] * int(r["new_free"]) + p["w_occupied"] * int(r["new_occupied"])
        assert gain < 2 ** 32
        r["gain"] = gain
        r["beams_free"], r["beams_hit"], r["beams_unknown"] = beams
        return r

    def gain(self, poses):
        return np.array([self.record(pose) for pose in np.asarray(poses, dtype=np.float64).reshape(-1, 3)], dtype=DTYPE)

    def select(self, poses, k, min_gain=1):
        """-> (indices, gains at pick time), in pick order"""
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        select_check(len(poses), k, min_gain)
        picks, gains, left = [], [], list(range(len(poses)))
        for _ in range(k):
            g = [int(self.record(poses[i])["gain"]) for i in left]
            best = max(range(len(left)), key=lambda j: (g[j], -left[j]))
            if g[best] < min_gain:
                break
            picks.append(left[best]); gains.append(g[best])
            self.commit([poses[left[best]]])
            del left[best]
        return np.asarray(picks, dtype=np.int32), np.asarray(gains, dtype=np.uint32)


def candidates(frontiers, n_headings=1):
    n_headings = max(1, int(n_headings))
    out = [(float(f["anchor_xy"][0]), float(f["anchor_xy"][1]), h * (2.0 * math.pi / n_headings)) for f in frontiers for h in range(n_headings)]
    return np.asarray(out, dtype=np.float64).reshape(-1, 3)
