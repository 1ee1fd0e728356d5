"""TEST INFRASTRUCTURE (not a test): the rule of kh_map_footprint_*  in numpy and plain Python on the CPU -- an
oriented convex polygon checked against a map's cell states and distance field, at poses and by heading.  It reads nothing of the
library; TraceLine is tests/map_localize_rule.py's.

  footprint    3 .. 16 vertices (vx, vy) in metres, finite, strictly convex in either winding: all cross products of consecutive edges
               have one sign, none is 0, and the polygon goes round once.  r_max = max sqrt(vx^2 + vy^2); reach = ceil(r_max * scale) + 1
               cells, at most 255 (the layer: at most 64)
  vertex cells of pose (x, y, theta): c = cos(theta), s = sin(theta) (libm's); wx_k = x + (c vx_k - s vy_k), wy_k = y + (s vx_k + c vy_k);
               V_k = (round_half_away((wx_k - anchor_x) * scale), round_half_away((wy_k - anchor_y) * scale)); a coordinate beyond
               +-2^30 cells: LATTICE, the record all zeros but the status, min_d2 FAR
  covered      edge k = the cells of TraceLine(V_k, V_(k + 1) mod n) (the outward walk visits exactly these); the outline is the union
               of the edges; for every row j from min V.y to max V.y: lo_j, hi_j the smallest and largest column of an outline cell of
               the row; Covered = {(i, j): lo_j <= i <= hi_j}; no row of the range is empty
  record       counts over Covered by state (100 occupied, 255 free, any other unknown, off the window outside), n_cells their sum,
               min_d2 the smallest field value under the covered window cells (FAR without one), status the largest code that applies:
               FREE 0, UNKNOWN 1 (n_unknown > 0), OUTSIDE 2 (n_outside > 0), COLLISION 3 (n_occupied > 0), LATTICE 4
  layer        theta_h = (2.0 * pi * h) / H; O_hk = (round_half_away((c vx_k - s vy_k) * scale), round_half_away((s vx_k + c vy_k) * scale));
               the vertex cells of window cell (i, j) are (i, j) + O_hk; bit h of its mask is set when that status is <= max_status;
               n_fit[h], n_any, n_all (all H bits set) count the cells
"""
from __future__ import annotations

import math

import numpy as np

import map_localize_rule as ml

FREE, UNKNOWN, OUTSIDE, COLLISION, LATTICE = range(5)
FAR = 0xFFFFFFFF
FIELDS = ("status", "n_cells", "n_free", "n_occupied", "n_unknown", "n_outside", "min_d2", "pad")
DTYPE = np.dtype([(k, np.int32 if k == "status" else np.uint32) for k in FIELDS])
MIN_VERTICES, MAX_VERTICES, MAX_REACH, LAYER_MAX_REACH, MAX_POSES, MAX_HEADINGS = 3, 16, 255, 64, 65536, 32
LATTICE_LIMIT = 2 ** 30


class Refused(ValueError):
    pass


def rectangle(length=1.0, width=0.6):
    return [(length / 2, width / 2), (-length / 2, width / 2), (-length / 2, -width / 2), (length / 2, -width / 2)]


def convex(verts):
    n = len(verts)
    sign, dxs = 0, []
    for k in range(n):
        (x0, y0), (x1, y1), (x2, y2) = verts[k], verts[(k + 1) % n], verts[(k + 2) % n]
        ax, ay, bx, by = x1 - x0, y1 - y0, x2 - x1, y2 - y1
        cross = ax * by - ay * bx
        s = 1 if cross > 0.0 else -1 if cross < 0.0 else 0
        if s == 0 or (sign != 0 and s != sign):
            return False
        sign = s
        if ax != 0.0:
            dxs.append(1 if ax > 0.0 else -1)
    changes = sum(1 for k in range(len(dxs)) if dxs[k] != dxs[k - 1])
    return changes == 2


def reach_of(verts, scale):
    """ceil(r_max * scale) + 1 as a float (it may be huge)"""
    r_max = 0.0
    for vx, vy in verts:
        r_max = max(r_max, math.sqrt(vx * vx + vy * vy))
    return float(np.ceil(np.float64(r_max) * np.float64(scale))) + 1.0


def create_check(verts, scale):
    """-> reach; Refused with the name of the first refusal, in the library's order"""
    verts = [(float(x), float(y)) for x, y in verts]
    if not MIN_VERTICES <= len(verts) <= MAX_VERTICES:
        raise Refused("n_vertices")
    if not all(math.isfinite(v) for p in verts for v in p):
        raise Refused("finite")
    with np.errstate(all="ignore"):
        ok = bool(convex([(np.float64(x), np.float64(y)) for x, y in verts]))
    if not ok:
        raise Refused("convex")
    with np.errstate(all="ignore"):
        r = float(np.ceil(np.sqrt(max(np.float64(x) * np.float64(x) + np.float64(y) * np.float64(y) for x, y in verts)) * np.float64(scale))) + 1.0
    if not r <= MAX_REACH:
        raise Refused("reach")
    return int(r)


def layer_check(n_headings, max_status, reach):
    if not 1 <= n_headings <= MAX_HEADINGS:
        raise Refused("n_headings")
    if not 0 <= max_status <= 2:
        raise Refused("max_status")
    if reach > LAYER_MAX_REACH:
        raise Refused("layer reach")


def _cell(v):
    """round_half_away of one scaled coordinate -> the cell, None beyond +-2^30 cells"""
    if not math.isfinite(v) or abs(v) > LATTICE_LIMIT + 1.0:
        return None
    r = ml.round_half_away(v)
    return int(r) if abs(r) <= LATTICE_LIMIT else None


def pose_cells(verts, pose, anchor, scale):
    """-> [(i, j)] per vertex, or None: LATTICE (a vertex, or the pose's own cell, beyond +-2^30 cells)"""
    x, y, theta = (float(v) for v in pose)
    c, s = math.cos(theta), math.sin(theta)
    ax, ay, scale = float(anchor[0]), float(anchor[1]), float(scale)
    out = []
    for vx, vy in verts:
        vx, vy = float(vx), float(vy)
        wx = x + (c * vx - s * vy)
        wy = y + (s * vx + c * vy)
        out.append((_cell((wx - ax) * scale), _cell((wy - ay) * scale)))
    own = (_cell((x - ax) * scale), _cell((y - ay) * scale))
    if any(v is None for p in out + [own] for v in p):
        return None
    return out


def heading_offsets(verts, h, n_headings, scale):
    theta = (2.0 * math.pi * h) / n_headings
    c, s = math.cos(theta), math.sin(theta)
    scale = float(scale)
    return [(int(ml.round_half_away((c * float(vx) - s * float(vy)) * scale)), int(ml.round_half_away((s * float(vx) + c * float(vy)) * scale))) for vx, vy in verts]


def spans(cells):
    """vertex cells -> (y0, lo, hi): rows y0 .. y0 + len(lo) - 1, row r covering columns lo[r] .. hi[r]"""
    n = len(cells)
    y0, y1 = min(c[1] for c in cells), max(c[1] for c in cells)
    lo, hi = np.full(y1 - y0 + 1, 2 ** 62, dtype=np.int64), np.full(y1 - y0 + 1, -2 ** 62, dtype=np.int64)
    for k in range(n):
        (ax, ay), (bx, by) = cells[k], cells[(k + 1) % n]
        x, y = ml.line_cells(ax, ay, bx, by)
        np.minimum.at(lo, y - y0, x)
        np.maximum.at(hi, y - y0, x)
    assert np.all(lo <= hi), "the outline is a closed loop: no row is empty"
    return y0, lo, hi


def covered(cells):
    """-> (i, j) int64 arrays of the covered lattice cells"""
    y0, lo, hi = spans(cells)
    i = np.concatenate([np.arange(a, b + 1, dtype=np.int64) for a, b in zip(lo, hi)])
    j = np.concatenate([np.full(b - a + 1, y0 + r, dtype=np.int64) for r, (a, b) in enumerate(zip(lo, hi))])
    return i, j


def record_of(view, d2, cells):
    """the record of vertex cells (None: LATTICE); d2: (height, width) uint32 field values of the view's window"""
    r = np.zeros((), dtype=DTYPE)
    r["min_d2"] = FAR
    if cells is None:
        r["status"] = LATTICE
        return r
    i, j = covered(cells)
    wx, wy = i - view["ox"], j - view["oy"]
    inside = (wx >= 0) & (wx < view["width"]) & (wy >= 0) & (wy < view["height"])
    state = view["cells"][wy[inside], wx[inside]]
    n_occ, n_free = int((state == 100).sum()), int((state == 255).sum())
    n_unknown, n_out = int(state.size) - n_occ - n_free, int((~inside).sum())
    r["n_free"], r["n_occupied"], r["n_unknown"], r["n_outside"] = n_free, n_occ, n_unknown, n_out
    r["n_cells"] = n_free + n_occ + n_unknown + n_out
    if state.size:
        r["min_d2"] = d2[wy[inside], wx[inside]].min()
    r["status"] = COLLISION if n_occ else OUTSIDE if n_out else UNKNOWN if n_unknown else FREE
    return r


def check(view, d2, verts, poses):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    if not 1 <= len(poses) <= MAX_POSES:
        raise Refused("n")
    if not np.all(np.isfinite(poses)):
        raise Refused("pose")
    return np.array([record_of(view, d2, pose_cells(verts, p, view["anchor"], view["scale"])) for p in poses], dtype=DTYPE)


def layer(view, verts, n_headings, max_status):
    """-> (masks (height, width) uint32, dict(n_fit (H,) uint64, n_any, n_all)).  Per heading the blocking cells under every span by
    row prefix sums over the window padded with `reach` cells of "outside"."""
    reach = create_check(verts, view["scale"])
    layer_check(n_headings, max_status, reach)
    h_, w_ = view["height"], view["width"]
    win = view["cells"][:h_, :w_]
    blocks = np.full((h_ + 2 * reach, w_ + 2 * reach), max_status < OUTSIDE, dtype=np.int64)
    blocks[reach:reach + h_, reach:reach + w_] = (win == 100) | ((win != 255) & (win != 100) & (max_status < UNKNOWN))
    prefix = np.zeros((blocks.shape[0], blocks.shape[1] + 1), dtype=np.int64)
    prefix[:, 1:] = np.cumsum(blocks, axis=1)
    masks = np.zeros((h_, w_), dtype=np.uint32)
    n_fit = np.zeros(n_headings, dtype=np.uint64)
    for h in range(n_headings):
        offsets = heading_offsets(verts, h, n_headings, view["scale"])
        assert all(abs(v) <= reach for p in offsets for v in p), "the reach bounds every offset"
        y0, lo, hi = spans(offsets)
        blocked = np.zeros((h_, w_), dtype=np.int64)
        for r, (a, b) in enumerate(zip(lo, hi)):
            rows = slice(reach + y0 + r, reach + y0 + r + h_)
            blocked += prefix[rows, reach + b + 1:reach + b + 1 + w_] - prefix[rows, reach + a:reach + a + w_]
        fits = blocked == 0
        masks |= fits.astype(np.uint32) << np.uint32(h)
        n_fit[h] = fits.sum()
    full = np.uint32((1 << n_headings) - 1)
    return masks, dict(n_fit=n_fit, n_any=int((masks != 0).sum()), n_all=int((masks == full).sum()))


def path_poses(xy):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    poses = np.zeros((len(xy), 3), dtype=np.float64)
    poses[:, :2] = xy
    if len(xy) > 1:
        d = xy[1:] - xy[:-1]
        poses[:-1, 2] = np.arctan2(d[:, 1], d[:, 0])
        poses[-1, 2] = poses[-2, 2]
    return poses


def check_path(view, d2, verts, xy, level=COLLISION):
    records = check(view, d2, verts, path_poses(xy))
    at = np.flatnonzero(records["status"] >= level)
    return records, (int(at[0]) if len(at) else -1)
