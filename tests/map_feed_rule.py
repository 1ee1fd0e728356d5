"""The map feed's rule as plain numpy, independent of the library: karto's cell states as
nav_msgs/OccupancyGrid values, the tiles of the lattice, and a consumer that applies what a feed hands out.

Values: vis_utils::toNavMap (include/slam_toolbox/visualization_utils.hpp:108-146) -- 0 unknown -> -1, 100 occupied -> 100,
255 free -> 0.  Tiles: tile (tx, ty) covers lattice cells [16 tx, 16 tx + 16) x [16 ty, 16 ty + 16) with tx, ty FLOOR quotients, so
the tiles left of and below the anchor are negative.  A window is (ox, oy, width, height) in lattice cells, all multiples of 16."""
import numpy as np

TILE = 16


def to_nav(cells):
    """int8 nav values of an array of karto cell states; any other state is an error of the caller"""
    c = np.asarray(cells)
    assert np.isin(c, (0, 100, 255)).all(), "a cell state that is neither unknown, occupied nor free"
    out = np.full(c.shape, -1, dtype=np.int8)
    out[c == 100] = 100
    out[c == 255] = 0
    return out


def tile_of(cell):
    """floor quotient: cell -1 lies in tile -1, cell -16 too, cell -17 in tile -2"""
    return np.floor_divide(np.asarray(cell, dtype=np.int64), TILE)


def tiles_that_differ(old_nav, new_nav, ox, oy):
    """(n, 2) int32 of (tx, ty): the tiles in which two (height, width) maps of the window starting at lattice cell (ox, oy) differ,
    in ascending (ty, tx) order"""
    old_nav, new_nav = np.asarray(old_nav), np.asarray(new_nav)
    assert old_nav.shape == new_nav.shape and old_nav.ndim == 2
    h, w = old_nav.shape
    assert ox % TILE == 0 and oy % TILE == 0 and w % TILE == 0 and h % TILE == 0, "a tile straddles the window's edge"
    differs = (old_nav != new_nav).reshape(h // TILE, TILE, w // TILE, TILE).any(axis=(1, 3))
    rows, cols = np.nonzero(differs)                   # row-major: ascending (row, column)
    return np.stack([tile_of(ox) + cols, tile_of(oy) + rows], axis=1).astype(np.int32).reshape(-1, 2)


def patch(consumer, window, tile_xy, data):
    """What a consumer does with one poll.  consumer: (nav (height, width) int8, (ox, oy, width, height)) or None for a consumer that
    has seen nothing; window: the feed's window after the poll, which holds the consumer's; tile_xy (n, 2), data (n, 16, 16).
    Returns the new (nav, window): the old map grown to `window` with -1, the tiles written over it.  The input is not changed."""
    ox, oy, w, h = (int(v) for v in window)
    nav = np.full((h, w), -1, dtype=np.int8)
    if consumer is not None:
        old, (px, py, pw, ph) = consumer
        assert px >= ox and py >= oy and px + pw <= ox + w and py + ph <= oy + h, "the window shrank"
        nav[py - oy:py - oy + ph, px - ox:px - ox + pw] = old
    tile_xy, data = np.asarray(tile_xy).reshape(-1, 2), np.asarray(data).reshape(-1, TILE, TILE)
    assert tile_xy.shape[0] == data.shape[0]
    for (tx, ty), tile in zip(tile_xy, data):
        x, y = int(tx) * TILE - ox, int(ty) * TILE - oy
        assert 0 <= x <= w - TILE and 0 <= y <= h - TILE, "a tile outside the window"
        nav[y:y + TILE, x:x + TILE] = tile
    return nav, (ox, oy, w, h)


def single_cell_tiles(old_nav, new_nav, ox, oy):
    """[(tx, ty, row, column)] of the tiles that differ in exactly ONE cell, with that cell's place inside its tile"""
    out = []
    for tx, ty in tiles_that_differ(old_nav, new_nav, ox, oy):
        x, y = int(tx) * TILE - ox, int(ty) * TILE - oy
        rows, cols = np.nonzero(np.asarray(old_nav)[y:y + TILE, x:x + TILE] != np.asarray(new_nav)[y:y + TILE, x:x + TILE])
        if rows.size == 1:
            out.append((int(tx), int(ty), int(rows[0]), int(cols[0])))
    return out


# Single cells in tile corners: two scans of a three-beam laser whose beam 0 points along +x exactly and whose other beams read
# under the minimum range, on a dyadic lattice (cell c has its centre at c * resolution, exactly).  Beam 0 of the first scan leaves
# cell (15, 15) -- the LAST row and column of tile (0, 0) -- and runs right through tile (1, 0); beam 0 of the second runs from
# cell (-48, -16) through tile (-3, -1) and ends in cell (-32, -16), the FIRST row and column of tile (-2, -1).
CORNER_RESOLUTION, CORNER_ANCHOR, CORNER_SHIFT = 0.0625, (0.0, 0.0), (1024, 1024)
CORNER_BEAMS = (((15, 15), 16), ((-48, -16), 16))            # (sensor cell, length of beam 0 in cells)


def corner_scans():
    """[(pose (3,), ranges (3,), points (3, 2))] of the two scans: what a mapper that places them at `pose` holds"""
    out = []
    for (cx, cy), n in CORNER_BEAMS:
        sx, sy, r = cx * CORNER_RESOLUTION, cy * CORNER_RESOLUTION, n * CORNER_RESOLUTION
        out.append((np.array([sx, sy, 0.0]), np.array([r, 0.05, 0.05]), np.array([[sx + r, sy], [sx, sy], [sx, sy]])))
    return out


def corner_expected(min_pass_through=0, occupancy_threshold=0.1):
    """(window, nav values of the window) after the two corner scans, from the occupancy oracle alone (tests/live_map_rule.py)"""
    import live_map_rule as rule
    import occupancy_cases as oc
    from oracle import karto
    placed = corner_scans()
    scans = [karto.Scan(r, pose, points=pts) for pose, r, pts in placed]
    every = np.concatenate([pts[:1] for _, _, pts in placed] + [pose[None, :2] for pose, _, _ in placed])
    assert rule.shift_is_exact(every, CORNER_ANCHOR, CORNER_SHIFT, CORNER_RESOLUTION)
    win = rule.window(None, np.array([pose[:2] for pose, _, _ in placed]), CORNER_ANCHOR, CORNER_RESOLUTION, oc.GATES.range_threshold)
    cells = rule.expected(win, scans, CORNER_ANCHOR, CORNER_RESOLUTION, oc.GATES, min_pass_through, occupancy_threshold, CORNER_SHIFT)[0]
    return win, to_nav(cells[:, :win[2]])


def corner_precondition():
    """asserts that, seen from an all -1 map, one tile changes in exactly one cell in its last row and last column and another in
    exactly one cell in its first row and first column; returns the two as (tx, ty, row, column)"""
    win, nav = corner_expected()
    singles = single_cell_tiles(np.full(nav.shape, -1, dtype=np.int8), nav, win[0], win[1])
    last = [s for s in singles if s[2:] == (TILE - 1, TILE - 1)]
    first = [s for s in singles if s[2:] == (0, 0)]
    assert last and first, f"no tile changes in a single corner cell: {singles}"
    return last[0], first[0]
