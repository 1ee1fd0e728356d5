"""The rule of the map-sourced correlation grid, stated in numpy on the CPU oracle: what
kh_matcher_add_map / kh_matcher_match_map* must compute.

    points = map_points(view)                     # the occupied cells' world points, row-major
    grid = rule_grid(om, query_pose, points)      # centre the oracle, AddScan's point loop on a zeroed array
    install(om, grid)                             # ... into the oracle's own grid
    response, mean, cov = match(om, scan, params) # MatchScan's control flow on the oracle's CorrelateScan

The expected mean, covariance and response are therefore the oracle's own CorrelateScan on the rule's grid.
tests/test_map_match_rule_oracle.py pins the loop and the control flow to the oracle's AddScans / MatchScan."""
from __future__ import annotations

import numpy as np

from oracle import karto

OCCUPIED = 100
MAX_VARIANCE = 500.0                    # Mapper.cpp:52
PI_180 = 0.01745329251994329577         # Math.h:34


def view_dict(cells, anchor, scale, ox=0, oy=0, width=None):
    """a map view as the rule reads it: cells (height, >= width) uint8 of karto cell states"""
    cells = np.asarray(cells, dtype=np.uint8)
    return dict(cells=cells, width=cells.shape[1] if width is None else int(width), height=cells.shape[0], ox=int(ox), oy=int(oy),
                anchor=(float(anchor[0]), float(anchor[1])), scale=float(scale))


def map_points(view):
    """world points (n, 2) of the cells whose state is exactly 100, row j outer, column i inner: anchor + (o + i) / scale in
    float64, the integer sum first (CoordinateConverter::GridToWorld without flip)"""
    cells = view["cells"][:view["height"], :view["width"]]
    j, i = np.nonzero(cells == OCCUPIED)            # row-major order
    x = view["anchor"][0] + (view["ox"] + i.astype(np.int64)).astype(np.float64) / view["scale"]
    y = view["anchor"][1] + (view["oy"] + j.astype(np.int64)).astype(np.float64) / view["scale"]
    return np.stack([x, y], axis=1).reshape(-1, 2)


def _round(v):
    """math::Round (Math.h:87-90), half away from zero"""
    return np.where(v >= 0.0, np.floor(v + 0.5), np.ceil(v - 0.5))


def rule_grid(om, query_pose, points, stats=None):
    """Centres the oracle's grid on the query's sensor pose (MatchScan steps 1-4, ko_center_grid) and runs ScanMatcher::AddScan's
    point loop (Mapper.cpp:1082-1104; ko_add_scan without FindValidPoints) over `points`, in their order, on a zeroed array with
    the oracle's geometry and smear kernel.  stats (a dict): 'stamped', and 'skipped' = points whose cell already held 100."""
    karto.lib().ko_center_grid(om.h, np.ascontiguousarray(query_pose, dtype=np.float64))
    gi = om.grid_info()
    kernel = om.kernel()
    k, ws = gi["kernel_size"], gi["width_step"]
    hk = k // 2
    data = np.zeros(gi["data_size"], dtype=np.uint8).reshape(-1, ws)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    # CoordinateConverter::WorldToGrid, Karto.h:4421-4436
    gxd = _round((points[:, 0] - gi["offset_x"]) * gi["scale"])
    gyd = _round((points[:, 1] - gi["offset_y"]) * gi["scale"])
    inside = (gxd >= 0) & (gxd < gi["roi_w"]) & (gyd >= 0) & (gyd < gi["roi_h"])        # (NaN compares false)
    stamped = skipped = 0
    for gx, gy in zip(gxd[inside].astype(np.int64), gyd[inside].astype(np.int64)):
        x, y = int(gx) + gi["roi_x"], int(gy) + gi["roi_y"]                               # CorrelationGrid::GridIndex
        if data[y, x] == OCCUPIED:
            skipped += 1
            continue
        data[y, x] = OCCUPIED
        window = data[y - hk:y + hk + 1, x - hk:x + hk + 1]                               # SmearPoint, Mapper.h:1152-1183
        np.maximum(window, kernel, out=window)
        stamped += 1
    if stats is not None:
        stats.update(stamped=stamped, skipped=skipped, inside=int(inside.sum()))
    return data.reshape(-1)


def _inside_span(anchor, scale, o, n, offset, grid_scale, roi_n):
    """(first, last) of the map's cells 0 .. n - 1 along one axis whose centre WorldToGrid puts inside the region of interest; None
    where there is none"""
    v = anchor + (o + np.arange(n, dtype=np.int64)).astype(np.float64) / scale
    g = _round((v - offset) * grid_scale)
    k = np.nonzero((g >= 0) & (g < roi_n))[0]
    return (int(k[0]), int(k[-1])) if k.size else None


def _unit_bound(view, gi, grow):
    cols = _inside_span(view["anchor"][0], view["scale"], view["ox"], view["width"], gi["offset_x"], gi["scale"], gi["roi_w"])
    rows = _inside_span(view["anchor"][1], view["scale"], view["oy"], view["height"], gi["offset_y"], gi["scale"], gi["roi_h"])
    if cols is None or rows is None:
        return 0
    cw = min(cols[1] + grow, view["width"] - 1) - max(cols[0] - grow, 0) + 1
    ch = min(rows[1] + grow, view["height"] - 1) - max(rows[0] - grow, 0) + 1
    return -(-cw // 64) * ch


def units_lower_bound(view, grid_info):
    """A lower bound of the units (64 cells of a row) of the map's clip to the region of interest, from the rule's own WorldToGrid: the
    columns and rows whose cell centres fall inside the region span cw' and ch' cells, the clip keeps at least those, so
    n_units >= ceil(cw' / 64) * ch'.  grid_info: the oracle's, centred on the query (rule_grid centres it)."""
    return _unit_bound(view, grid_info, 0)


def units_upper_bound(view, grid_info):
    """... and an upper bound where a cell centre falls inside the region: the clip starts at floor(edge) - 1 and ends at ceil(edge) + 1
    for the region's edges in map cells, which is at most two cells beyond the first and the last centre inside, and it ends with the map.
    (A region that holds no cell centre gives 0, which bounds nothing.)"""
    return _unit_bound(view, grid_info, 2)


def install(om, grid):
    """writes `grid` into the oracle's own correlation grid (ko_grid_data is the live buffer; Matcher.grid() copies)"""
    n = om.grid_info()["data_size"]
    live = np.ctypeslib.as_array(karto.lib().ko_grid_data(om.h), shape=(n,))
    live[:] = np.asarray(grid, dtype=np.uint8).reshape(-1)


def match(om, scan, params, do_penalize=True, do_refine=True):
    """ko_match_scan's control flow (Mapper.cpp:534-639: coarse, up to three expansions, fine) on Matcher.correlate_scan with the
    covariance threaded through, against the grid the oracle HOLDS (rule_grid + install with this scan's pose).  `params`: the
    dict the oracle matcher was made with.  Returns (response, mean, cov (3, 3))."""
    pose = np.asarray(scan.sensor_pose, dtype=np.float64)
    car = params["coarse_angle_resolution"]
    if scan.n == 0:                                                                      # Mapper.cpp:547-557
        cov = np.zeros((3, 3))
        cov[0, 0] = cov[1, 1] = MAX_VARIANCE
        cov[2, 2] = 4 * (car * car)
        return 0.0, pose.copy(), cov
    res = 1.0 / om.grid_info()["scale"]
    side = om.probs().shape[0]
    cso = 0.5 * (float(side) - 1) * res
    csr = 2 * res
    cov = np.zeros(9)
    best, mean, cov = om.correlate_scan(scan, pose, (cso, cso), (csr, csr), params["coarse_search_angle_offset"], car, do_penalize,
                                        False, cov)
    if best == -1e9:
        return best, mean, cov
    if params["use_response_expansion"] and abs(best - 0.0) <= 1e-06:                   # math::DoubleEqual
        new_offset = params["coarse_search_angle_offset"]
        for _ in range(3):
            new_offset += 20 * PI_180
            best, mean, cov = om.correlate_scan(scan, pose, (cso, cso), (csr, csr), new_offset, car, do_penalize, False, cov)
            if best == -1e9:
                return best, mean, cov
            if not abs(best - 0.0) <= 1e-06:
                break
    if do_refine:
        center = mean.copy()
        best, mean, cov = om.correlate_scan(scan, center, (csr * 0.5, csr * 0.5), (res, res), 0.5 * car,
                                            params["fine_search_angle_offset"], do_penalize, True, cov)
    return best, mean, cov
