"""TEST INFRASTRUCTURE (not a test): the rule of the region analysis in numpy -- what kh_map_regions_* must
compute.  It reads nothing of the library.  The field's values are tests/map_field_rule.py's, the lattice cell of a point
tests/map_localize_rule.py's.

  inputs      the field's snapshot of the cell states and its d2 values over the field's window; cells outside the window do not
              exist, columns width .. width_step - 1 are never read and never connect anything
  N           the 4 or the 8 neighbours of a cell (connectivity), for everything below
  Rc          ceil(min_clearance * scale), the field's own radius_cells; a field with 0 < R < Rc is refused
  traversable state 255 and d2 >= Rc * Rc (FAR counts as beyond)
  unknown     state neither 100 nor 255
  frontier    state 255 and at least one cell of N inside the window unknown -- on states alone, not on clearance
  components  of each mask under N; the root of a component is the window index j * width + i of its smallest cell: the label
  kept        a component of at least min cells that stands among the first max such components in root order; kept components are
              numbered 0, 1, ... in root order; the id grid holds the kept id, NONE off the mask, DROPPED for the rest
  record      root, n_cells, box (x, y, w, h in lattice cells), sum_i, sum_j (window-relative), max_d2 (FAR if any member is FAR),
              n_other (members set in the OTHER mask), link (the smallest kept id of the other set among the members, else NONE),
              anchor_cell (the member nearest the centroid cell ((2 sum_i + n) // (2 n), (2 sum_j + n) // (2 n)) by squared cell
              distance, ties to the smallest window index), centroid and anchor_xy in doubles
  lookup      the clearance call's cell rule; OUTSIDE off the window or beyond +-2^30 cells, AT_NONE off the traversable mask,
              AT_DROPPED, AT_OK with the id
"""
from __future__ import annotations

import math

import numpy as np

import map_field_rule as fr
import map_localize_rule as ml

NONE, DROPPED = 0xFFFFFFFF, 0xFFFFFFFE
REGIONS, FRONTIERS = 0, 1
AT_OK, AT_NONE, AT_DROPPED, OUTSIDE = 0, 1, 2, 3
MAX_COUNT = 1 << 20
PARAMS = dict(min_clearance=0.0, connectivity=8, min_region_cells=1, max_regions=4096, min_frontier_cells=1, max_frontiers=4096)
RECORD_FIELDS = ("root", "n_cells", "box", "sum_i", "sum_j", "max_d2", "n_other", "link", "anchor_cell", "centroid", "anchor_xy")
Refused = fr.Refused


def params_check(p, scale):
    """-> Rc; Refused in the library's order"""
    if not (math.isfinite(p["min_clearance"]) and p["min_clearance"] >= 0.0):
        raise Refused("min_clearance")
    rc = fr.radius_cells(p["min_clearance"], scale)
    if p["connectivity"] not in (4, 8):
        raise Refused("connectivity")
    if p["min_region_cells"] < 1 or p["min_frontier_cells"] < 1:
        raise Refused("minimum")
    if not (1 <= p["max_regions"] <= MAX_COUNT and 1 <= p["max_frontiers"] <= MAX_COUNT):
        raise Refused("maximum")
    return rc


def masks(view, d2, rc, connectivity):
    """-> (traversable, frontier), (height, width) bool each"""
    h, w = view["height"], view["width"]
    win = view["cells"][:h, :w]
    free, unknown = win == 255, (win != 100) & (win != 255)
    traversable = free & (np.asarray(d2, dtype=np.int64) >= rc * rc)
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = unknown
    near = np.zeros((h, w), dtype=bool)
    for dj, di in neighbours(connectivity):
        near |= pad[1 + dj:1 + dj + h, 1 + di:1 + di + w]
    return traversable, free & near


def neighbours(connectivity):
    four = [(-1, 0), (0, -1), (0, 1), (1, 0)]
    return four if connectivity == 4 else four + [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def components(mask, connectivity):
    """(height, width) int64: the root of every cell's component, -1 off the mask.  Union-find over the runs of the rows: runs are
    numbered in row-major order of their first cell, a union keeps the smaller number, so a root run's first cell is the component's
    smallest."""
    h, w = mask.shape
    parent, first, runs, previous = [], [], [], []
    reach = 1 if connectivity == 8 else 0

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    for j in range(h):
        edge = np.diff(np.concatenate(([0], mask[j].astype(np.int8), [0])))
        current = []
        for x0, x1 in zip(np.nonzero(edge == 1)[0].tolist(), np.nonzero(edge == -1)[0].tolist()):
            k = len(parent)
            parent.append(k); first.append(j * w + x0); runs.append((j, x0, x1)); current.append((x0, x1, k))
            for a0, a1, q in previous:
                if a0 < x1 + reach and a1 > x0 - reach:
                    a, b = find(k), find(q)
                    parent[max(a, b)] = min(a, b)
        previous = current
    out = np.full((h, w), -1, dtype=np.int64)
    for k, (j, x0, x1) in enumerate(runs):
        out[j, x0:x1] = first[find(k)]
    return out


def keep(roots, minimum, maximum):
    """-> (id grid uint32, kept roots, n_total, truncated)"""
    found, counts = np.unique(roots[roots >= 0], return_counts=True)
    passing = found[counts >= minimum]
    kept = passing[:maximum]
    ids = np.full(roots.shape, NONE, dtype=np.uint32)
    ids[roots >= 0] = DROPPED
    if kept.size:
        at = np.searchsorted(kept, roots)
        hit = (roots >= 0) & (at < kept.size)
        hit[hit] = kept[at[hit]] == roots[hit]
        ids[hit] = at[hit].astype(np.uint32)
    return ids, kept, int(found.size), bool(passing.size > maximum)


def records(view, d2, ids, n_kept, other_ids):
    """the records of one set: a list of n_kept dicts"""
    h, w = ids.shape
    jj, ii = np.nonzero(ids < DROPPED)
    k = ids[jj, ii].astype(np.int64)
    index = jj.astype(np.int64) * w + ii
    n = np.bincount(k, minlength=n_kept).astype(np.int64)
    sum_i, sum_j = (np.bincount(k, weights=v.astype(np.float64), minlength=n_kept).astype(np.int64) for v in (ii, jj))   # exact below 2^53
    big = np.iinfo(np.int64).max
    x0, y0, x1, y1, root = (np.full(n_kept, v, dtype=np.int64) for v in (big, big, -1, -1, big))
    np.minimum.at(x0, k, ii); np.minimum.at(y0, k, jj); np.maximum.at(x1, k, ii); np.maximum.at(y1, k, jj); np.minimum.at(root, k, index)
    max_d2 = np.zeros(n_kept, dtype=np.int64)
    np.maximum.at(max_d2, k, np.asarray(d2, dtype=np.int64)[jj, ii])
    other = other_ids[jj, ii].astype(np.int64)
    n_other = np.bincount(k, weights=(other != NONE).astype(np.float64), minlength=n_kept).astype(np.int64)
    link = np.full(n_kept, NONE, dtype=np.int64)
    np.minimum.at(link, k, np.where(other < DROPPED, other, NONE))
    ci, cj = (2 * sum_i + n) // np.maximum(2 * n, 1), (2 * sum_j + n) // np.maximum(2 * n, 1)
    key = (((ii - ci[k]) ** 2 + (jj - cj[k]) ** 2).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)
    best = np.full(n_kept, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(best, k, key)
    anchor_cell = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out = []
    ax, ay, scale = float(view["anchor"][0]), float(view["anchor"][1]), float(view["scale"])
    for q in range(n_kept):
        ai, aj = int(anchor_cell[q] % w), int(anchor_cell[q] // w)
        out.append(dict(
            root=int(root[q]), n_cells=int(n[q]), box=(int(x0[q]) + view["ox"], int(y0[q]) + view["oy"], int(x1[q] - x0[q]) + 1, int(y1[q] - y0[q]) + 1),
            sum_i=int(sum_i[q]), sum_j=int(sum_j[q]), max_d2=int(max_d2[q]), n_other=int(n_other[q]), link=int(link[q]), anchor_cell=int(anchor_cell[q]),
            centroid=(ax + (float(view["ox"]) + float(sum_i[q]) / float(n[q])) / scale, ay + (float(view["oy"]) + float(sum_j[q]) / float(n[q])) / scale),
            anchor_xy=(ax + float(view["ox"] + ai) / scale, ay + float(view["oy"] + aj) / scale)))
    return out


def analyse(view, d2, radius, **params):
    """the whole analysis of a field (its view dict, its values, its R) -> dict(region_ids, frontier_ids, regions, frontiers, stats)"""
    p = dict(PARAMS, **params)
    rc = params_check(p, view["scale"])
    if 0 < radius < rc:
        raise Refused("reach")
    traversable, frontier = masks(view, d2, rc, p["connectivity"])
    sets = []
    for mask, minimum, maximum in ((traversable, p["min_region_cells"], p["max_regions"]), (frontier, p["min_frontier_cells"], p["max_frontiers"])):
        sets.append(keep(components(mask, p["connectivity"]), minimum, maximum))
    (rid, rkept, rtotal, rcut), (fid, fkept, ftotal, fcut) = sets
    stats = dict(ox=view["ox"], oy=view["oy"], width=view["width"], height=view["height"], clearance_cells=rc, connectivity=p["connectivity"],
                 n_traversable=int(traversable.sum()), n_frontier_cells=int(frontier.sum()), n_total=[rtotal, ftotal], n_kept=[int(rkept.size), int(fkept.size)],
                 truncated=[int(rcut), int(fcut)])
    return dict(region_ids=rid, frontier_ids=fid, regions=records(view, d2, rid, rkept.size, fid), frontiers=records(view, d2, fid, fkept.size, rid), stats=stats)


def lookup(view, region_ids, xy):
    """-> (status int32, id uint32) of (n, 2) world points"""
    status, ids = [], []
    for x, y in np.asarray(xy, dtype=np.float64).reshape(-1, 2):
        cx, cy = ml.lattice_cell(x, view["anchor"][0], view["scale"]), ml.lattice_cell(y, view["anchor"][1], view["scale"])
        v = fr.value_at(view, region_ids, cx, cy) if max(abs(cx), abs(cy)) <= 2 ** 30 else None
        if v is None:
            status.append(OUTSIDE); ids.append(NONE)
        elif v == NONE:
            status.append(AT_NONE); ids.append(NONE)
        elif v == DROPPED:
            status.append(AT_DROPPED); ids.append(DROPPED)
        else:
            status.append(AT_OK); ids.append(v)
    return np.array(status, dtype=np.int32), np.array(ids, dtype=np.uint32)


def reachable(view, region_ids, a, b):
    (sa, sb), (ia, ib) = lookup(view, region_ids, [a, b])
    return bool(sa == AT_OK and sb == AT_OK and ia == ib)


def tile_grid(width, height):
    """the 64 x 16-cell tiles of a window: (tiles across, tiles down, horizontal seams x width + vertical seams x height)"""
    tx, ty = (width + 63) // 64, (height + 15) // 16
    return tx, ty, (ty - 1) * width + (tx - 1) * height


def centroid_cell(total, n):
    return (2 * total + n) // (2 * n)
