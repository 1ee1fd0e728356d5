"""TEST INFRASTRUCTURE (not a test): the rule of the distance field in numpy -- what kh_map_field_* must compute.
It reads nothing of the library.  The gate, the lattice cell and the refusals of a pose are tests/map_localize_rule.py's, the scan
points the CPU oracle's.

  field       window cells only; an obstacle is state 100 (OCCUPIED) or any state but 255 (NOT_FREE); R = ceil(max_distance * scale),
              0 = uncapped; d2 = min over obstacles of (i - a)^2 + (j - b)^2; kept when R == 0 or d2 <= R * R, else FAR; all FAR
              without an obstacle; metres = sqrt(d2) / scale, +inf for FAR
  costs       Rt = ceil(inflation_radius * scale); table[d2] = 254 at 0, 253 while m <= inscribed, int(252 exp(-k (m - inscribed)))
              while m <= inflation, else 0; an unknown cell under track_unknown is 255 unless c >= 253 or (inflate_unknown and c > 0)
  clearance   the lattice cell of the point; beyond +-2^30 cells or outside the window OUTSIDE, a FAR value FAR, else OK
  score       the gate's hit beams at their own end point; T = truncate_cells or R; cost = sum of min(d2, T^2), a missing cell T^2
  refine      compass search over 27 candidates on the integer cost; the centre wins ties, else the smallest index
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import map_localize_rule as ml

FAR = 0xFFFFFFFF
OCCUPIED, NOT_FREE = 0, 1
OK, CLEAR_FAR, OUTSIDE = 0, 1, 2
CONVERGED, MAX_ROUNDS, LEFT_LATTICE = 0, 1, 2
MAX_RADIUS, MAX_SIDE, MAX_CELLS, MAX_UNCAPPED_SIDE = 1024, 32768, 1 << 28, 4096
INFLATION = dict(inscribed_radius=0.22, inflation_radius=0.55, cost_scaling_factor=10.0, track_unknown=1, inflate_unknown=0)
REFINE = dict(step_heading=0.02, n_halvings=4, max_rounds=64, truncate_cells=0)       # step_xy: 2 / scale


class Refused(Exception):
    pass


def radius_cells(metres, scale):
    """ceil(metres * scale); Refused where the library answers KH_ERR_INVALID_ARG"""
    if not (math.isfinite(metres) and metres >= 0.0):
        raise Refused("distance")
    product = float(metres) * float(scale)
    if not product <= MAX_RADIUS:                              # (the ceiling of a value above an integer lies above it too)
        raise Refused("radius")
    return int(math.ceil(product))


def field_check(width, height, scale, max_distance, obstacles):
    """-> R; Refused in the library's order"""
    r = radius_cells(max_distance, scale)
    if obstacles not in (OCCUPIED, NOT_FREE):
        raise Refused("obstacles")
    if width > MAX_SIDE or height > MAX_SIDE:
        raise Refused("side")
    if width * height > MAX_CELLS:
        raise Refused("cells")
    if r == 0 and (width > MAX_UNCAPPED_SIDE or height > MAX_UNCAPPED_SIDE):
        raise Refused("uncapped side")
    return r


def obstacle_mask(view, obstacles=OCCUPIED):
    win = view["cells"][:view["height"], :view["width"]]
    return win == 100 if obstacles == OCCUPIED else win != 255


def capped(d2, r):
    """int64 squared distances (a huge value for none) -> the stored uint32 values"""
    far = (d2 >= 2 ** 40) | ((d2 > r * r) if r > 0 else False)
    return np.where(far, FAR, d2).astype(np.uint32)


NONE = 2 ** 50


def d2_brute(view, r, obstacles=OCCUPIED, chunk=2048):
    """the minimum over all obstacle cells, cell by cell"""
    mask = obstacle_mask(view, obstacles)
    h, w = mask.shape
    b, a = (v.astype(np.int64) for v in np.nonzero(mask))
    out = np.full(h * w, NONE, dtype=np.int64)
    if a.size:
        j, i = (v.ravel().astype(np.int64) for v in np.mgrid[0:h, 0:w])
        for at in range(0, h * w, chunk):
            di, dj = i[at:at + chunk, None] - a[None, :], j[at:at + chunk, None] - b[None, :]
            out[at:at + chunk] = (di * di + dj * dj).min(axis=1)
    return capped(out.reshape(h, w), r)


def column_distances(mask):
    """the distance along the column to the nearest obstacle of the column, NONE where the column has none"""
    h, w = mask.shape
    down, up = np.full((h, w), NONE, dtype=np.int64), np.full((h, w), NONE, dtype=np.int64)
    run = np.full(w, NONE, dtype=np.int64)
    for row in range(h):
        run = np.where(mask[row], 0, np.where(run >= NONE, NONE, run + 1))
        down[row] = run
    run = np.full(w, NONE, dtype=np.int64)
    for row in range(h - 1, -1, -1):
        run = np.where(mask[row], 0, np.where(run >= NONE, NONE, run + 1))
        up[row] = run
    return np.minimum(down, up)


def d2_separable(view, r, obstacles=OCCUPIED):
    """column distances, then per row the minimum over the row's columns of g^2 + (i - k)^2: the larger maps"""
    mask = obstacle_mask(view, obstacles)
    h, w = mask.shape
    g = column_distances(mask)
    g2 = np.where(g >= NONE, NONE, g * g)
    k = np.arange(w, dtype=np.int64)
    across = (k[:, None] - k[None, :]) ** 2
    out = np.empty((h, w), dtype=np.int64)
    for row in range(h):
        out[row] = (g2[row][None, :] + across).min(axis=1)
    return capped(out, r)


def metres(d2, scale):
    d2 = np.asarray(d2)
    with np.errstate(invalid="ignore"):
        return np.where(d2 == FAR, np.inf, np.sqrt(d2.astype(np.float64)) / np.float64(scale))


def stats(d2):
    near = d2[d2 != FAR]
    return dict(n_obstacles=int((d2 == 0).sum()), n_far=int((d2 == FAR).sum()), max_d2=int(near.max()) if near.size else 0)


# ---------------------------------------------------------------- costs
def inflation_check(p, scale):
    """-> Rt; Refused where the library answers KH_ERR_INVALID_ARG"""
    for k in ("inscribed_radius", "inflation_radius", "cost_scaling_factor"):
        if not (math.isfinite(p[k]) and p[k] >= 0.0):
            raise Refused(k)
    if p["inscribed_radius"] > p["inflation_radius"] or p["track_unknown"] not in (0, 1) or p["inflate_unknown"] not in (0, 1):
        raise Refused("parameters")
    if not (math.isfinite(scale) and scale > 0.0):
        raise Refused("scale")
    return radius_cells(p["inflation_radius"], scale)


def cost_of(p, scale, d2):
    if d2 == 0:
        return 254
    m = math.sqrt(float(d2)) / scale
    if m <= p["inscribed_radius"]:
        return 253
    if m <= p["inflation_radius"]:
        return int(252.0 * math.exp(-p["cost_scaling_factor"] * (m - p["inscribed_radius"])))
    return 0


def cost_table(scale, **params):
    p = dict(INFLATION, **params)
    rt = inflation_check(p, scale)
    return np.array([cost_of(p, float(scale), d2) for d2 in range(rt * rt + 1)], dtype=np.uint8)


def costs(view, d2, r, **params):
    """(height, width) uint8 from the field's values; Refused for a field that does not reach the inflation radius"""
    p = dict(INFLATION, **params)
    table = cost_table(view["scale"], **params)
    rt2 = table.size - 1
    if 0 < r and r * r < rt2:
        raise Refused("reach")
    c = np.where(d2 <= rt2, table[np.minimum(d2, rt2)], 0).astype(np.uint8)
    win = view["cells"][:view["height"], :view["width"]]
    unknown = (win != 100) & (win != 255)
    if p["track_unknown"]:
        keep = (c >= 253) | ((c > 0) if p["inflate_unknown"] else False)
        c = np.where(unknown & ~keep, 255, c).astype(np.uint8)
    return c


# ---------------------------------------------------------------- clearance
def value_at(view, d2, cx, cy):
    """the value of lattice cell (cx, cy), None where the window has no such cell"""
    wx, wy = cx - view["ox"], cy - view["oy"]
    if 0 <= wx < view["width"] and 0 <= wy < view["height"] and cx != -2 ** 31 and cy != -2 ** 31:
        return int(d2[wy, wx])
    return None


def clearance(view, d2, xy):
    """-> (metres, status, d2) of (n, 2) world points"""
    out_m, out_s, out_d = [], [], []
    for x, y in np.asarray(xy, dtype=np.float64).reshape(-1, 2):
        cx, cy = ml.lattice_cell(x, view["anchor"][0], view["scale"]), ml.lattice_cell(y, view["anchor"][1], view["scale"])
        v = value_at(view, d2, cx, cy) if max(abs(cx), abs(cy)) <= 2 ** 30 else None
        if v is None:
            out_m.append(math.inf); out_s.append(OUTSIDE); out_d.append(FAR)
        elif v == FAR:
            out_m.append(math.inf); out_s.append(CLEAR_FAR); out_d.append(FAR)
        else:
            out_m.append(math.sqrt(float(v)) / view["scale"]); out_s.append(OK); out_d.append(v)
    return np.array(out_m), np.array(out_s, dtype=np.int32), np.array(out_d, dtype=np.uint32)


# ---------------------------------------------------------------- score
def truncation(truncate_cells, r):
    if not 0 <= truncate_cells <= MAX_RADIUS:
        raise Refused("truncate_cells")
    t = truncate_cells if truncate_cells > 0 else r
    if t <= 0:
        raise Refused("an uncapped field needs truncate_cells")
    return t


def score(view, d2, r, laser, ranges, pose, truncate_cells=0):
    """kh_field_score's fields for one scan at sensor pose `pose`; Refused as kh_map_fit refuses"""
    from oracle import karto
    ranges = np.asarray(ranges, dtype=np.float64)
    pose = np.asarray(pose, dtype=np.float64)
    if ml.fit_refused(view, laser, pose):
        raise Refused("pose")
    t2 = truncation(truncate_cells, r) ** 2
    points = karto.scan_points(ranges, pose, laser)
    n = dict(n_kept=0, n_hit=0, n_inside=0, n_near=0, sum_d2=0)
    for rd, p in zip(ranges, points):
        kept, hit, end = ml.gate(rd, p, pose, laser)
        n["n_kept"] += kept
        if not (kept and hit):
            continue
        n["n_hit"] += 1
        v = value_at(view, d2, ml.lattice_cell(end[0], view["anchor"][0], view["scale"]), ml.lattice_cell(end[1], view["anchor"][1], view["scale"]))
        if v is None:
            continue
        n["n_inside"] += 1
        if v <= t2:
            n["n_near"] += 1
            n["sum_d2"] += v
    n["cost"] = n["sum_d2"] + (n["n_hit"] - n["n_near"]) * t2
    n["score"] = 1.0 - float(n["cost"]) / (float(n["n_hit"]) * float(t2)) if n["n_hit"] > 0 else 0.0
    return n


def score_arrays(view, d2, r, laser, ranges, pose, truncate_cells=0):
    """score() with the beams as arrays (the refinement asks for hundreds of poses; tests/test_map_field_rule_oracle.py holds the two
    side by side).  A hit beam lies below the range threshold, so the gate leaves its end point as it is."""
    from oracle import karto
    ranges = np.asarray(ranges, dtype=np.float64)
    pose = np.asarray(pose, dtype=np.float64)
    if ml.fit_refused(view, laser, pose):
        raise Refused("pose")
    t2 = truncation(truncate_cells, r) ** 2
    points = np.asarray(karto.scan_points(ranges, pose, laser), dtype=np.float64).reshape(-1, 2)
    kept = ~((ranges <= laser.min_range) | (ranges >= laser.max_range) | np.isnan(ranges))
    hit = kept & (ranges < (laser.range_threshold - 1e-06))
    cx = ml.o_round((points[hit, 0] - np.float64(view["anchor"][0])) * np.float64(view["scale"])).astype(np.int64) - view["ox"]
    cy = ml.o_round((points[hit, 1] - np.float64(view["anchor"][1])) * np.float64(view["scale"])).astype(np.int64) - view["oy"]
    inside = (cx >= 0) & (cx < view["width"]) & (cy >= 0) & (cy < view["height"])
    v = d2[cy[inside], cx[inside]].astype(np.int64)
    near = v <= t2
    n = dict(n_kept=int(kept.sum()), n_hit=int(hit.sum()), n_inside=int(inside.sum()), n_near=int(near.sum()), sum_d2=int(v[near].sum()))
    n["cost"] = n["sum_d2"] + (n["n_hit"] - n["n_near"]) * t2
    n["score"] = 1.0 - float(n["cost"]) / (float(n["n_hit"]) * float(t2)) if n["n_hit"] > 0 else 0.0
    return n


# ---------------------------------------------------------------- refine
Refined =namedtuple("Refined", "pose cost_start cost n_hit rounds halvings status")


def candidate(pose, s, a, c):
    return (pose[0] + float(c % 3 - 1) * s, pose[1] + float(c // 3 % 3 - 1) * s, pose[2] + float(c // 9 - 1) * a)


def pick(costs):
    """the candidate of least cost: the centre if it is among the least, else the smallest index"""
    least = min(costs)
    return 13 if costs[13] == least else costs.index(least)


def refine_params_check(p):
    if not (math.isfinite(p["step_xy"]) and p["step_xy"] > 0.0 and math.isfinite(p["step_heading"]) and p["step_heading"] >= 0.0 and
            0 <= p["n_halvings"] <= 32 and 1 <= p["max_rounds"] <= 4096 and 0 <= p["truncate_cells"] <= MAX_RADIUS):
        raise Refused("refine parameters")


def refine_with(cost_of_pose, refused, start, p):
    """the state machine on any cost function: cost_of_pose(pose) -> (cost, n_hit); refused(pose) -> bool"""
    pose = tuple(float(v) for v in start)
    s, a = float(p["step_xy"]), float(p["step_heading"])
    cost, n_hit = cost_of_pose(pose)
    cost_start, rounds, halvings = cost, 0, 0
    while True:
        cands = [candidate(pose, s, a, c) for c in range(27)]
        if any(refused(c) for c in cands):
            return Refined(np.array(pose), cost_start, cost, n_hit, rounds, halvings, LEFT_LATTICE)
        costs = [cost_of_pose(c)[0] for c in cands]
        best = pick(costs)
        rounds += 1
        cost = costs[best]
        if best == 13:
            if halvings == p["n_halvings"]:
                return Refined(np.array(pose), cost_start, cost, n_hit, rounds, halvings, CONVERGED)
            s, a, halvings = s * 0.5, a * 0.5, halvings + 1
        else:
            pose = cands[best]
        if rounds >= p["max_rounds"]:
            return Refined(np.array(pose), cost_start, cost, n_hit, rounds, halvings, MAX_ROUNDS)


def refine(view, d2, r, laser, ranges, starts, **params):
    """kh_map_field_refine: one Refined per start"""
    p = dict(REFINE, step_xy=2.0 / view["scale"])
    p.update(params)
    refine_params_check(p)
    truncation(p["truncate_cells"], r)
    memo = {}

    def cost_of_pose(pose):
        if pose not in memo:
            sc = score_arrays(view, d2, r, laser, ranges, pose, p["truncate_cells"])
            memo[pose] = (sc["cost"], sc["n_hit"])
        return memo[pose]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    if any(ml.fit_refused(view, laser, s) for s in starts):
        raise Refused("start")
    return [refine_with(cost_of_pose, lambda q: ml.fit_refused(view, laser, q), s, p) for s in starts]
