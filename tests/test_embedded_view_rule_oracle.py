"""CPU: tests/embedded_view.py places a window where its layouts say -- the alignment of every row from the rule
(base + row * stride + col) % 4 alone -- and every row tests/embedded_view_cases.py names exists and sits on the edge the GPU test
needs it for.  No library, no GPU."""
import numpy as np
import pytest

import embedded_view as ev
import embedded_view_cases as cases
import map_field_rule as field_rule
import map_field_update_cases as uc

SHAPES = [(1, 1), (1, 7), (3, 2), (5, 5), (13, 9), (37, 30), (40, 50), (67, 3), (77, 60)]         # width x height


def aligned_dwords(lay, height, width):
    """per row: does a window column that is a multiple of 4 start a dword of the buffer -- k_field_changed's dword branch"""
    return [(lay.base + row * lay.stride + 4 * (width // 8)) % 4 == 0 for row in range(height)]


@pytest.mark.parametrize("width, height", SHAPES)
def test_layouts(width, height):
    for name in ev.layouts_for(width):
        lay = ev.layout(name, width, height)
        res = ev.residues(lay, height)
        assert res == [(lay.base + row * lay.stride + 0) % 4 for row in range(height)]
        assert lay.stride >= width and lay.top >= ev.MARGIN_ROWS and lay.size >= lay.base + (height + ev.MARGIN_ROWS) * lay.stride - lay.left
        if name == "L1":
            assert lay.base % 4 == 1 and lay.stride % 4 == 0 and set(res) == {1}
        if name == "L2":
            assert lay.base % 4 == 2 and lay.stride % 4 == 2 and res == [2 if row % 2 == 0 else 0 for row in range(height)]
        if name == "L3":
            assert lay.base % 4 == 3 and lay.stride % 2 == 1
            if height >= 4:
                assert set(res) == {0, 1, 2, 3}, "the alignment rotates through all four"
                both = aligned_dwords(lay, height, width)
                assert any(both) and not all(both), "rows on both branches of k_field_changed inside one launch"
        if name == "L4":
            assert lay.stride == width and width % 2 == 1 and lay.left == 0 and lay.base % 2 == 1
            if height >= 4:
                assert set(res) == {0, 1, 2, 3}
        else:
            assert lay.left >= ev.MARGIN_COLUMNS and lay.stride - lay.left - width >= ev.MARGIN_COLUMNS
    assert ("L4" in ev.layouts_for(width)) == (width % 2 == 1)


@pytest.mark.parametrize("width, height", SHAPES)
def test_embed_puts_the_window_among_poison(width, height):
    rng = np.random.default_rng(width * 100 + height)
    cells = rng.choice(np.array([0, 100, 255, 7], dtype=np.uint8), size=(height, width))
    view = uc.view(cells, -5, 3)
    for name in ev.layouts_for(width):
        for fill in ev.FILLS:
            lay, flat, inner = ev.embed(view, name, fill)
            assert flat.dtype == np.uint8 and flat.size == lay.size
            assert np.array_equal(ev.window_of(inner), cells) and inner["cells"].shape == (height, lay.stride)
            assert all(inner[k] == view[k] for k in ("width", "height", "ox", "oy", "anchor", "scale"))
            grid = flat.reshape(-1, lay.stride)
            if name != "L4":
                assert np.array_equal(grid[lay.top:lay.top + height, lay.left:lay.left + width], cells)
                rest = np.ones(grid.shape, dtype=bool)
                rest[lay.top:lay.top + height, lay.left:lay.left + width] = False
                assert (grid[rest] == fill).all() and (inner["cells"][:, width:] == fill).all(), "what is no cell of the window is poison"
            else:
                assert np.array_equal(grid[lay.top:lay.top + height], cells) and (grid[:lay.top] == fill).all() and (grid[lay.top + height:] == fill).all()
            assert (flat[:lay.base] == fill).all() and flat[:lay.base].size >= ev.MARGIN_ROWS * lay.stride
    t = ev.tight(view)
    assert t["cells"].shape == (height, width) and np.array_equal(t["cells"], cells)


def test_the_rows_exist_and_cover_the_widths():
    tables = dict(seeds=cases.seed_rows(), fit=cases.fit_rows(), ray=cases.ray_rows(), observe=cases.observe_rows(), field=cases.field_rows())
    widths = set()
    for name, table in tables.items():
        assert 2 <= len(table), name
        assert any(c.view["ox"] < 0 and c.view["oy"] < 0 for c in table), f"{name}: no row of a negative origin"
        widths |= {c.view["width"] for c in table}
    merges = cases.merge_rows()
    assert any(c.target["ox"] < 0 and c.moving["ox"] < 0 for c in merges)
    assert any(c.correction[2] != 0.0 and c.target["width"] == 70 for c in merges), "under a rotation"
    assert sum("wholly outside" in c.name for c in merges) == 2, "wholly apart, grown and not"
    widths |= {c.target["width"] for c in merges}
    maps = cases.map_cases()
    assert any(c.view["ox"] < 0 for c in maps)
    widths |= {c.view["width"] for c in maps}
    edits = cases.shape_edit_rows() + cases.rect_forms_mod4()
    assert all(e.before["ox"] < 0 for e in edits)
    widths |= {e.before["width"] for e in edits}
    assert cases.WIDTHS <= widths, sorted(cases.WIDTHS - widths)
    # the sensor outside the window on each side
    ray = cases.ray_rows()[0]
    v = ray.view
    lo = (v["anchor"][0] + (v["ox"] - 0.5) / v["scale"], v["anchor"][1] + (v["oy"] - 0.5) / v["scale"])
    hi = (lo[0] + v["width"] / v["scale"], lo[1] + v["height"] / v["scale"])
    sides = {(int(p[0] > hi[0]) - int(p[0] < lo[0]), int(p[1] > hi[1]) - int(p[1] < lo[1])) for p in ray.poses}
    assert {(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)} <= sides, sides
    for c in cases.field_rows():
        if cases.inflation_for(c.radius) is not None:
            field_rule.costs(c.view, field_rule.d2_brute(c.view, c.radius, c.obstacles), c.radius, **cases.inflation_for(c.radius))     # not Refused


def test_the_rectangles_take_every_residue():
    forms = cases.rect_forms_mod4()
    firsts = {(e.rect[0] - e.before["ox"]) % 4 for e in forms}
    lasts = {(e.rect[0] - e.before["ox"] + e.rect[2] - 1) % 4 for e in forms}
    assert firsts == lasts == {0, 1, 2, 3} and len(forms) == 16
    for e in forms:
        exp = uc.expected(e.before, e.after, e.radius, e.obstacles, e.rect)                 # (asserts the caller's promise)
        assert exp["cells_box"] == (12, 13, 6, 4) and exp["values_box"] == (9, 10, 12, 10) and exp["cells_compared"] == e.rect[2] * 6
    lay = ev.layout("L3", 37, 30)
    rows_aligned = [(lay.base + row * lay.stride + 20) % 4 == 0 for row in range(9, 15)]
    assert any(rows_aligned) and not all(rows_aligned), "the rectangle's rows take both branches on L3"
    rounds = list(uc.random_rounds(**cases.RANDOM_ROUNDS))
    assert len(rounds) == 11 and rounds[0][0]["ox"] < 0
