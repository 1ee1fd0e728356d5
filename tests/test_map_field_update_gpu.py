"""GPU: a field that follows its map (kh_map_field_update, MapField.update; csrc/occupancy_field_update.hip) on the cases of
tests/map_field_update_cases.py.  After EVERY update: the values are byte-equal to a fresh MapField of the same view and to
tests/map_field_rule.py, the statistics are the rule's, and what the update reports (rebuilt, both boxes, the cells recomputed) is
what the case table works out from the two windows.  Everything is an integer and is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import map_field_cases as fc
import map_field_rule as rule
import map_field_update_cases as cases
import map_localize_cases as lc
from common import bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_field import MapField
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu
REPORTED = ("rebuilt", "relayout", "cells_box", "values_box", "cells_recomputed", "cells_compared")


class Followed:
    """a view in device memory of the caller's own and a field made from it; step() rewrites the cells and updates the field.
    d2_rule: the form of tests/map_field_rule.py the values are held against (d2_brute for windows too wide for the separable one);
    place: what puts a view dict into device memory (DeviceView, or tests/embedded_view.py's EmbeddedView in one of its layouts)"""

    def __init__(self, view, radius, obstacles=rule.OCCUPIED, first_update=True, d2_rule=rule.d2_separable, place=DeviceView):
        self.radius, self.obstacles, self.view, self.d2_rule = radius, obstacles, view, d2_rule
        self.d = place(view)
        self.field = MapField(self.d.v, max_distance=radius / view["scale"], obstacles=obstacles)
        if first_update:                                       # a field from kh_map_field_create: its first update allocates g and rebuilds
            got = self.field.update(self.d.v)
            assert {k: got[k] for k in REPORTED} == cases.rebuilt(view)
            self.check()

    def upload(self, view):
        self.d.upload(view)
        self.view = view

    def step(self, after, rect=None, want=None):
        want = cases.expected(self.view, after, self.radius, self.obstacles, rect) if want is None else want
        self.upload(after)
        got = self.field.update(self.d.v, rect)
        assert {k: got[k] for k in REPORTED} == want, (got, want)
        assert got["times_ms"][3] > 0
        self.check()
        return got

    def check(self):
        view, f = self.view, self.field
        want = self.d2_rule(view, self.radius, self.obstacles)
        d2 = f.d2
        assert np.array_equal(d2, want), f"{int((d2 != want).sum())} values differ from the rule"
        fresh = MapField(self.d.v, max_distance=self.radius / view["scale"], obstacles=self.obstacles)
        assert np.array_equal(d2, fresh.d2), "the updated field differs from a fresh one"
        for st in (f.stats, fresh.stats):
            assert {k: st[k] for k in ("n_obstacles", "n_far", "max_d2")} == rule.stats(want), st
            assert (st["ox"], st["oy"], st["width"], st["height"], st["radius_cells"]) == (view["ox"], view["oy"], view["width"], view["height"], self.radius)
        fresh.close()

    def close(self):
        self.field.close()
        self.d.close()


SHAPE_EDITS = cases.shape_edits()


@pytest.mark.parametrize("edit", SHAPE_EDITS, ids=[e.name for e in SHAPE_EDITS])
def test_window_shapes_at_every_band_height(kartohip_lib, edit):
    """forwards and backwards at forced band heights 1, 4, 5 and the library's choice: the same values every time"""
    f = Followed(edit.before, edit.radius, edit.obstacles)
    for band in cases.BANDS:
        f.field.set_band_rows(band)
        f.step(edit.after)
        f.step(edit.before)
    f.field.set_band_rows(1)
    f.field.update(f.d.v)                                      # nothing changed
    f.upload(edit.after)
    f.field.set_band_rows(0)
    got = f.field.update(f.d.v)
    assert got["times_ms"][0] > 0 and got["times_ms"][1] > 0 and got["times_ms"][2] > 0
    f.check()
    f.close()


@pytest.mark.parametrize("kind", ["added", "only removed", "neighbour removed"])
def test_single_cell_edits(kartohip_lib, kind):
    edits = cases.single_cell_edits(kind)
    f = Followed(edits[0].before, edits[0].radius)
    for e in edits:
        f.step(e.before)                                       # from the last case's window to this one's
        got = f.step(e.after)
        assert got["rebuilt"] == 0 and got["cells_box"][2:] == (1, 1) and got["cells_recomputed"] < e.after["width"] * e.after["height"], e.name
    f.close()


def test_a_state_change_that_is_no_obstacle_change_launches_no_pass(kartohip_lib):
    quiet = cases.state_only_edit(rule.OCCUPIED)
    f = Followed(quiet.before, quiet.radius, rule.OCCUPIED)
    before = f.field.d2
    got = f.step(quiet.after)
    assert got["values_box"] == cases.NONE and got["cells_box"] == (12, 13, 6, 4)
    assert got["times_ms"][0] > 0 and got["times_ms"][1] == 0.0 and got["times_ms"][2] == 0.0, "a column or a row kernel ran"
    assert np.array_equal(f.field.d2, before)
    assert np.array_equal(f.field.costs(), rule.costs(quiet.after, before, quiet.radius)), "the costs follow the states"
    f.close()
    loud = cases.state_only_edit(rule.NOT_FREE)
    f = Followed(loud.before, loud.radius, rule.NOT_FREE)
    before = f.field.d2
    got = f.step(loud.after)
    assert got["values_box"] == (9, 10, 12, 10) and got["times_ms"][1] > 0 and got["times_ms"][2] > 0
    assert not np.array_equal(f.field.d2, before)
    f.close()


def test_rectangle_forms(kartohip_lib):
    forms = cases.rect_forms()
    f = Followed(forms[0].before, forms[0].radius, forms[0].obstacles)
    for e in forms:
        f.step(e.after, e.rect)
        f.step(e.before, e.rect)
    # an unchanged view: compared, nothing found, nothing recomputed
    whole = f.view["width"] * f.view["height"]
    got = f.step(f.view, None, dict(rebuilt=0, relayout=0, cells_box=cases.NONE, values_box=cases.NONE, cells_recomputed=0, cells_compared=whole))
    assert got["times_ms"][1] == 0.0 and got["times_ms"][2] == 0.0
    # wholly outside the window, or empty: a no-op that is KH_OK
    for rect in cases.OUTSIDE_RECTS:
        got = f.field.update(f.d.v, rect)
        assert {k: got[k] for k in REPORTED} == dict(rebuilt=0, relayout=0, cells_box=cases.NONE, values_box=cases.NONE, cells_recomputed=0, cells_compared=0), rect
        assert got["times_ms"][:3] == [0.0, 0.0, 0.0]
    f.check()
    f.close()


def test_radius_beyond_both_sides(kartohip_lib):
    rng = np.random.default_rng(3)
    before = fc.mixed(rng, 4, 5, 0.1)
    after = before.copy()
    after[1, 2] = cases.F if before[1, 2] == cases.O else cases.O
    f = Followed(cases.view(before, 7, 7), 11)
    got = f.step(cases.view(after, 7, 7))
    assert got["values_box"] == (7, 7, 5, 4) and got["rebuilt"] == 0
    f.close()


@pytest.mark.parametrize("density, obstacles, radius", [(0.02, rule.OCCUPIED, 11), (0.3, rule.OCCUPIED, 4), (0.02, rule.NOT_FREE, 4), (0.3, rule.NOT_FREE, 11)])
def test_random_runs(kartohip_lib, density, obstacles, radius):
    rounds = cases.random_rounds(density, obstacles, 30, seed=radius)
    first, _ = next(rounds)
    f = Followed(first, radius, obstacles)
    smaller = 0
    for after, rect in rounds:
        got = f.step(after, rect)
        smaller += 0 < got["cells_recomputed"] < 40 * 50
    assert smaller > 0, "no round recomputed less than the window"
    f.close()


def test_an_uncapped_field_rebuilds(kartohip_lib):
    rounds = cases.random_rounds(0.05, rule.OCCUPIED, 3, seed=9)
    first, _ = next(rounds)
    f = Followed(first, 0)
    for after, rect in rounds:
        f.step(after, rect, cases.rebuilt(after))
    f.close()


def test_the_first_update_of_a_created_field(kartohip_lib):
    rounds = cases.random_rounds(0.1, rule.OCCUPIED, 1, seed=4)
    first, _ = next(rounds)
    after, rect = next(rounds)
    f = Followed(first, 4, first_update=False)
    f.step(after, rect, cases.rebuilt(after))                  # it allocates the column distances: a rebuild, whatever rect says
    f.step(first, rect)                                        # from then on by region
    f.close()


def test_relayout_and_the_lattice(kartohip_lib):
    rng = np.random.default_rng(21)
    big = fc.mixed(rng, 60, 70, 0.05)
    f = Followed(cases.view(big[10:40, 10:50].copy(), 10, 10), 4)
    fields_before = f.field.d2
    for name, cells, ox, oy in (("larger", big, 0, 0), ("shifted", big[15:45, 20:60].copy(), 20, 15), ("smaller", big[20:30, 30:33].copy(), 30, 20)):
        view = cases.view(cells, ox, oy)
        d = DeviceView(view)
        got = f.field.update(d.v, (0, 0, 1, 1))
        assert {k: got[k] for k in REPORTED} == cases.rebuilt(view, relayout=1), name
        f.d.close()
        f.d, f.view = d, view
        f.check()
        assert (f.field.width, f.field.height) == (view["width"], view["height"])
        changed = cells.copy()
        changed[1, 1] = cases.O if cells[1, 1] != cases.O else cases.F
        f.step(cases.view(changed, ox, oy))                    # and by region on the new window
    del fields_before
    # off the lattice: refused, in the order anchor x, anchor y, scale, device, and the field is as it was
    want = f.field.d2
    for field, value, word in (("anchor0", np.nextafter(cases.A[0], 9.0), "anchor x"), ("anchor1", np.nextafter(cases.A[1], 9.0), "anchor y"),
                               ("scale", np.nextafter(cases.K, 9.0), "scale"), ("device", 1, "device")):
        v = capi.KhMapView.from_buffer_copy(f.d.v)
        if field.startswith("anchor"):
            v.anchor[int(field[-1])] = value
        else:
            setattr(v, field, value)
        with pytest.raises(capi.KartoHipError) as e:
            f.field.update(v)
        assert e.value.code == capi.KH_ERR_INVALID_ARG and word in str(e.value), field
    v = capi.KhMapView.from_buffer_copy(f.d.v)
    v.anchor[0], v.scale = 9.0, 2.0
    with pytest.raises(capi.KartoHipError) as e:
        f.field.update(v)
    assert "anchor x" in str(e.value), "the first difference is the refusal"
    assert np.array_equal(f.field.d2, want)
    f.check()
    f.close()


def test_read_rect_and_costs_rect(kartohip_lib):
    rounds = cases.random_rounds(0.05, rule.OCCUPIED, 2, seed=6)
    first, _ = next(rounds)
    f = Followed(first, 11)
    for after, rect in rounds:
        f.step(after, rect)
    view, d2 = f.view, f.field.d2
    ox, oy, w, h = view["ox"], view["oy"], view["width"], view["height"]
    rects = [(ox, oy, 1, 1), (ox + w - 1, oy + h - 1, 1, 1), (ox, oy, w, h), (ox + 3, oy + 5, 9, 7), (ox + 1, oy + 2, w - 1, 3), (ox + 38, oy, 2, h)]
    for x, y, rw, rh in rects:
        block = f.field.read_rect(x, y, rw, rh)
        assert block.dtype == np.uint32 and np.array_equal(block, d2[y - oy:y - oy + rh, x - ox:x - ox + rw]), (x, y, rw, rh)
    for params in fc.INFLATIONS:
        for track, inflate in fc.UNKNOWN_POLICIES:
            kw = dict(params, track_unknown=track, inflate_unknown=inflate)
            whole = f.field.costs(**kw)
            assert np.array_equal(whole, rule.costs(view, d2, 11, **kw))
            for x, y, rw, rh in rects:
                block = f.field.costs_rect(x, y, rw, rh, **kw)
                assert block.dtype == np.uint8 and np.array_equal(block, whole[y - oy:y - oy + rh, x - ox:x - ox + rw]), (kw, x, y, rw, rh)
    L, p = capi.lib(), capi.KhInflationParams(0.22, 0.55, 10.0, 1, 0)
    values, costs = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint8)
    for x, y, rw, rh in ((ox - 1, oy, 2, 2), (ox, oy, w + 1, 1), (ox, oy + h - 1, 1, 2), (ox + w, oy, 1, 1), (ox, oy, 0, 1), (ox, oy, 1, -1)):
        assert L.kh_map_field_read_rect(f.field._h, x, y, rw, rh, values.ctypes.data) == capi.KH_ERR_INVALID_ARG, (x, y, rw, rh)
        assert L.kh_map_field_costs_rect(f.field._h, C.byref(p), x, y, rw, rh, costs.ctypes.data) == capi.KH_ERR_INVALID_ARG, (x, y, rw, rh)
    assert (values == 7).all() and (costs == 7).all(), "a refused rectangle wrote"
    with pytest.raises(capi.KartoHipError) as e:
        f.field.costs_rect(ox, oy, 2, 2, inflation_radius=3.0)         # 12 cells: beyond the field's 11
    assert e.value.code == capi.KH_ERR_INVALID_ARG
    f.close()


def test_readers_on_an_updated_field(kartohip_lib, oracle_lib):
    """clearance, score and refinement of an updated field are a fresh field's, bit for bit"""
    rounds = cases.random_rounds(0.05, rule.OCCUPIED, 4, seed=2)
    first, _ = next(rounds)
    f = Followed(first, 11)
    for after, rect in rounds:
        f.step(after, rect)
    fresh = MapField(f.d.v, max_distance=11 / cases.K)
    pts = fc.clearance_points(f.view, f.field.d2)
    for a, b in zip(f.field.clearance(pts), fresh.clearance(pts)):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
    laser = lc.circle(65)
    rng = np.random.default_rng(8)
    ranges = rng.uniform(0.5, 4.9, size=65)
    centre = np.array([cases.A[0] + (f.view["ox"] + 20) / cases.K, cases.A[1] + (f.view["oy"] + 25) / cases.K, 0.3])
    poses = centre + rng.uniform(-1.0, 1.0, size=(9, 3)) * [2.0, 2.0, 0.5]
    for t in (0, 3):
        got, want = f.field.score(ranges, poses, laser, truncate_cells=t), fresh.score(ranges, poses, laser, truncate_cells=t)
        assert got == want and any(s["n_near"] > 0 for s in got)
        rules = rule.score(f.view, f.field.d2, 11, laser, ranges, poses[0], t)
        assert all(got[0][k] == rules[k] for k in ("n_kept", "n_hit", "n_inside", "n_near", "sum_d2", "cost"))
    a, _ = f.field.refine(ranges, poses[:4], laser)
    b, _ = fresh.refine(ranges, poses[:4], laser)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x.pose), bits(y.pose)) and tuple(x)[1:] == tuple(y)[1:]
    fresh.close()
    f.close()
