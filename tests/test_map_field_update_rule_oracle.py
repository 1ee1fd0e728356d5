"""CPU: the two arguments kh_map_field_update stands on, in numpy, against tests/map_field_rule.py.

  region   after any edit, the values inside V = C grown by R (C: the box of the cells whose obstacle-ness changed), recomputed from
           NOTHING but the new states within 2R of C and the old values elsewhere, are d2_separable of the whole new map; and
           column distances change only in the columns of C on rows C.y grown by R
  bands    column distances swept band by band -- R rows of warm-up above and below, from "none" -- equal the whole-column sweep
           capped at R, whatever the band height

The same file checks that every case of tests/map_field_update_cases.py sits on the edge its name says.  No GPU."""
import numpy as np
import pytest

import map_field_cases as fc
import map_field_rule as rule
import map_field_update_cases as cases

NO_COLUMN = 0xFFFF


def capped_columns(mask, r):
    """rule.column_distances as k_field_columns stores them for a capped field"""
    g = rule.column_distances(mask)
    return np.where(g > r, NO_COLUMN, g).astype(np.int64)


def banded_columns(mask, r, band, x0=0, x1=None, y0=0, y1=None, g=None):
    """k_field_columns_band's sweeps in numpy: rows [y0, y1) in bands of `band`, each from its own warm-up; writes into g"""
    h, w = mask.shape
    x1, y1 = w if x1 is None else x1, h if y1 is None else y1
    g = np.full((h, w), -1, dtype=np.int64) if g is None else g
    step = lambda run, row: np.where(mask[row, x0:x1], 0, np.where(run >= r, NO_COLUMN, run + 1))      # noqa: E731
    for b0 in range(y0, y1, band):
        b1 = min(b0 + band, y1)
        run = np.full(x1 - x0, NO_COLUMN, dtype=np.int64)
        down = {}
        for row in range(max(0, b0 - r), b1):
            run = step(run, row)
            down[row] = run
        run = np.full(x1 - x0, NO_COLUMN, dtype=np.int64)
        for row in range(min(h, b1 + r) - 1, b0 - 1, -1):
            run = step(run, row)
            if row < b1:
                g[row, x0:x1] = np.minimum(run, down[row])
    return g


def rows_from(g, r, x0, x1, y0, y1, out):
    """k_field_rows_region in numpy: cells [x0, x1) x [y0, y1) from g, reading g no farther than R columns away"""
    w = g.shape[1]
    for row in range(y0, y1):
        for i in range(x0, x1):
            lo, hi = max(0, i - r), min(w, i + r + 1)
            k = np.arange(lo, hi)
            col = g[row, lo:hi]
            v = np.where(col == NO_COLUMN, rule.NONE, col * col + (k - i) ** 2)
            best = int(v.min())
            out[row, i] = rule.FAR if best >= rule.NONE or best > r * r else best


@pytest.mark.parametrize("r", [1, 2, 3, 5, 11])
def test_region_update_equals_the_whole_transform(r):
    rng = np.random.default_rng(900 + r)
    for trial in range(60):
        w, h = int(rng.integers(1, 61)), int(rng.integers(1, 71))
        obstacles = int(rng.integers(0, 2))
        before = cases.view(fc.mixed(rng, h, w, float(rng.choice([0.02, 0.15, 0.4]))))
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        ew, eh = int(rng.integers(1, w - x0 + 1)), int(rng.integers(1, h - y0 + 1))
        cells = cases.window_cells(before).copy()
        cells[y0:y0 + eh, x0:x0 + ew] = fc.mixed(rng, eh, ew, float(rng.choice([0.0, 0.1, 0.5])))
        after = cases.view(cells)
        old_mask, new_mask = rule.obstacle_mask(before, obstacles), rule.obstacle_mask(after, obstacles)
        want = rule.d2_separable(after, r, obstacles)
        d2 = rule.d2_separable(before, r, obstacles).copy()
        g = capped_columns(old_mask, r)
        c = cases.box_of(old_mask != new_mask)
        if c is None:
            assert np.array_equal(d2, want)
            continue
        v = cases.grow(c, r, r, w, h)
        cols = cases.grow(c, 0, r, w, h)
        reads = cases.grow(c, 0, 2 * r, w, h)
        # the column pass sees nothing but the new states of `reads`
        seen = np.zeros_like(new_mask)
        seen[reads[1]:reads[1] + reads[3], reads[0]:reads[0] + reads[2]] = new_mask[reads[1]:reads[1] + reads[3], reads[0]:reads[0] + reads[2]]
        banded_columns(seen, r, max(r, 8), cols[0], cols[0] + cols[2], cols[1], cols[1] + cols[3], g)
        assert np.array_equal(g, capped_columns(new_mask, r)), "g changed outside the columns of C on rows C.y grown by R"
        rows_from(g, r, v[0], v[0] + v[2], v[1], v[1] + v[3], d2)
        assert np.array_equal(d2, want), (trial, w, h, r, obstacles)
        exp = cases.expected(before, after, r, obstacles)
        assert exp["values_box"] == v and exp["cells_recomputed"] == v[2] * v[3]


@pytest.mark.parametrize("r", [1, 2, 3, 5, 11])
def test_banded_columns_equal_the_capped_sweep(r):
    rng = np.random.default_rng(40 + r)
    for w, h in ((1, 1), (5, 2), (7, 23), (13, 40), (3, 65)):
        for p in (0.0, 0.03, 0.3):
            mask = rng.random((h, w)) < p
            want = capped_columns(mask, r)
            for band in sorted({1, 2, max(1, r - 1), r, r + 1, h}):
                assert np.array_equal(banded_columns(mask, r, band), want), (w, h, p, band)
    # a rectangle of rows only: what lies outside keeps its value, what lies inside is the whole sweep's
    mask = rng.random((40, 9)) < 0.1
    g = np.full((40, 9), -5, dtype=np.int64)
    banded_columns(mask, r, 4, 2, 7, 11, 30, g)
    assert np.array_equal(g[11:30, 2:7], capped_columns(mask, r)[11:30, 2:7]) and (g[:11] == -5).all() and (g[30:] == -5).all() and (g[:, :2] == -5).all()


def test_the_cases_sit_on_their_edges():
    shapes = cases.shape_edits()
    assert len(shapes) == len(cases.SHAPES) * len(cases.RADII)
    e = next(s for s in shapes if s.name == "13 x 7, R 1")
    exp = cases.expected(e.before, e.after, 1, e.obstacles)
    assert exp["cells_box"][0] + exp["cells_box"][2] == e.after["ox"] + 13, "the change reaches the last column of a width that is no multiple of 4"
    e = next(s for s in shapes if s.name == "1 x 7, R 11")
    assert cases.expected(e.before, e.after, 11, e.obstacles)["values_box"] == (-3, 2, 1, 7), "R reaches past the window on both axes"
    for kind in ("added", "only removed", "neighbour removed"):
        edits = cases.single_cell_edits(kind)
        assert len(edits) == 9
        for e in edits:
            exp = cases.expected(e.before, e.after, e.radius, e.obstacles)
            assert exp["cells_box"][2:] == (1, 1) and 0 < exp["cells_recomputed"] <= 49 < e.after["width"] * e.after["height"]
            old, new = rule.d2_brute(e.before, e.radius), rule.d2_brute(e.after, e.radius)
            if kind == "only removed":
                assert (new == rule.FAR).all() and (old != rule.FAR).any()
            if kind == "neighbour removed":
                assert (new >= old).all() and (new > old).any(), "distances grow"
    quiet = cases.state_only_edit(rule.OCCUPIED)
    exp = cases.expected(quiet.before, quiet.after, quiet.radius, quiet.obstacles)
    assert exp["values_box"] == cases.NONE and exp["cells_box"] == (12, 13, 6, 4) and exp["cells_recomputed"] == 0
    loud = cases.state_only_edit(rule.NOT_FREE)
    exp = cases.expected(loud.before, loud.after, loud.radius, loud.obstacles)
    assert exp["values_box"] == (9, 10, 12, 10) and not np.array_equal(rule.d2_brute(loud.before, 3, rule.NOT_FREE), rule.d2_brute(loud.after, 3, rule.NOT_FREE))
    for e in cases.rect_forms():
        exp = cases.expected(e.before, e.after, e.radius, e.obstacles, e.rect)
        assert exp["values_box"] == (9, 10, 12, 10), e.name
    assert cases.expected(loud.before, loud.after, 3, rule.NOT_FREE, (10, 11, 100, 100))["cells_compared"] == 19 * 22
    for rect in cases.OUTSIDE_RECTS:
        assert cases.expected(loud.after, loud.after, 3, rule.NOT_FREE, rect)["cells_compared"] == 0
