"""GPU: every entry point that reads the cells of a kh_map_view, on views "filled by hand over any device buffer": the window of a
row of the existing case tables (tests/embedded_view_cases.py) inside a larger buffer of poison, its first cell off a dword, its
stride no multiple of 4 (tests/embedded_view.py's layouts L1 .. L4, poison 100 and 255).  For every case the answer is the existing
rule's on the inner window, is bit for bit what the library gives for the same window in a tight, aligned buffer, and the whole
buffer, poison included, is byte-equal afterwards to what was uploaded.  Everything is compared exactly."""
import numpy as np
import pytest

import embedded_view as ev
import embedded_view_cases as cases
import map_changes_rule as changes_rule
import map_field_cases as fc
import map_field_rule as field_rule
import map_field_update_cases as uc
import map_localize_cases as lc
import map_localize_rule as ml
import map_match_rule as mr
import map_merge_rule as merge_rule
import map_raycast_rule as ray_rule
from common import bits
from embedded_view import EmbeddedView
from slam_toolbox_amd.map_changes import MapChanges
from slam_toolbox_amd.map_field import MapField
from slam_toolbox_amd.map_localizer import MapLocalizer, map_fit, map_raycast, map_seeds
from slam_toolbox_amd.map_merge import MapMerge
from test_map_field_gpu import same_field
from test_map_field_update_gpu import REPORTED, Followed
from test_map_fit_gpu import same_fit
from test_map_merge_gpu import same_merge
from test_map_raycast_gpu import same_cast
from test_map_seeds_gpu import DeviceView, same_seeds

pytestmark = pytest.mark.gpu

SEED_ROWS, FIT_ROWS, RAY_ROWS, MERGE_ROWS = cases.seed_rows(), cases.fit_rows(), cases.ray_rows(), cases.merge_rows()
OBSERVE_ROWS, FIELD_ROWS, SHAPE_EDITS = cases.observe_rows(), cases.field_rows(), cases.shape_edit_rows()
names = lambda table: [c.name for c in table]               # noqa: E731


def placements(view):
    """the view in every layout its width takes and with both poisons, one at a time"""
    for name in ev.layouts_for(view["width"]):
        for fill in ev.FILLS:
            e = EmbeddedView(view, name, fill)
            yield e
            e.untouched()
            e.close()


def without_times(stats):
    return {k: v for k, v in stats.items() if k != "times_ms"}


@pytest.mark.parametrize("case", SEED_ROWS, ids=names(SEED_ROWS))
def test_seeds(kartohip_lib, case):
    t = DeviceView(ev.tight(case.view))
    ref = map_seeds(t.v, case.spacing, case.center, case.radius)
    for e in placements(case.view):
        got = map_seeds(e.v, case.spacing, case.center, case.radius)
        same_seeds(got, ml.seeds(e.inner, case.spacing, case.center, case.radius))
        same_seeds(got, ref)
        case.check(got[0].astype(np.int64), got[1])
    t.close()


@pytest.mark.parametrize("case", FIT_ROWS, ids=names(FIT_ROWS))
def test_fit(kartohip_lib, oracle_lib, case):
    t = DeviceView(ev.tight(case.view))
    ref = map_fit(t.v, case.laser, case.ranges, case.poses)
    for e in placements(case.view):
        got = map_fit(e.v, case.laser, case.ranges, case.poses)
        assert len(got) == len(case.poses)
        for g, r, pose in zip(got, ref, case.poses):
            same_fit(g, ml.fit(e.inner, case.laser, case.ranges, pose))
            same_fit(g, r)
        case.check(got)
    t.close()


@pytest.mark.parametrize("case", RAY_ROWS, ids=names(RAY_ROWS))
def test_raycast(kartohip_lib, oracle_lib, case):
    t = DeviceView(ev.tight(case.view))
    ref = map_raycast(t.v, case.laser, case.poses, case.max_unknown, case.no_return)
    for e in placements(case.view):
        got = map_raycast(e.v, case.laser, case.poses, case.max_unknown, case.no_return)
        same_cast(got, ray_rule.cast_poses(e.inner, case.laser, case.poses, case.max_unknown, case.no_return))
        same_cast(got, ref)
        case.check(got)
    t.close()


def test_the_matchers_map_entries(kartohip_lib, oracle_lib):
    """kh_matcher_add_map: the correlation grid from the occupied cells of the window, in their row-major order; kh_matcher_match_map
    and _match_map_batch: the match on that grid, against tests/map_match_rule.py's"""
    from common import OFFLINE_PARAMS
    from test_map_match_gpu import pair, scans_at
    hm, om = pair(cases.MATCHER, max_batch=2)
    for case in cases.map_cases():
        hq, oq = scans_at(case.pose, case.ranges)
        other, _ = scans_at(case.pose + [0.02, -0.01, 0.03], case.ranges)
        stats = {}
        want = mr.rule_grid(om, case.pose, mr.map_points(case.view), stats)
        mr.install(om, want)
        want_match = mr.match(om, oq, OFFLINE_PARAMS, True, True)
        assert stats["stamped"] > 4 and want_match[0] > 0.5, case.name
        t = DeviceView(ev.tight(case.view))
        hm.AddMap(hq, t.v, 0)
        ref = hm.GetCorrelationGrid(0).copy()
        ref_match, ref_batch = hm.MatchScanMap(hq, t.v), hm.MatchScanMapBatch([hq, other], t.v)
        t.close()
        assert np.array_equal(ref, want), case.name
        for a, b in zip(ref_match, want_match):
            assert np.array_equal(bits(a), bits(b)), case.name
        for e in placements(case.view):
            where = (case.name, e.name, e.fill)
            hm.AddMap(hq, e.v, 0)
            got = hm.GetCorrelationGrid(0)
            assert np.array_equal(got, mr.rule_grid(om, case.pose, mr.map_points(e.inner))), where
            assert np.array_equal(got, ref), where
            e.untouched()
            for a, b in zip(hm.MatchScanMap(hq, e.v), ref_match):
                assert np.array_equal(bits(a), bits(b)), where
            for a, b in zip(hm.MatchScanMapBatch([hq, other], e.v), ref_batch):
                assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b), where
    hm.close()


@pytest.mark.parametrize("case", MERGE_ROWS, ids=names(MERGE_ROWS))
def test_merge_with_target_and_moving_in_different_layouts(kartohip_lib, case):
    kw = dict(footprint=case.footprint, conflict=case.conflict, grow=case.grow)
    dt, dm = DeviceView(ev.tight(case.target)), DeviceView(ev.tight(case.moving))
    ref = MapMerge(dt.v, dm.v, case.correction, **kw)
    ref_cells, ref_codes, ref_stats = ref.cells(), ref.codes(), without_times(ref.stats)
    ref.close(); dt.close(); dm.close()
    ran = 0
    for lt, lm in cases.MERGE_LAYOUTS:
        if lt not in ev.layouts_for(case.target["width"]) or lm not in ev.layouts_for(case.moving["width"]):
            continue
        for ft, fm in ((100, 255), (255, 100)):
            et, em = EmbeddedView(case.target, lt, ft), EmbeddedView(case.moving, lm, fm)
            got = MapMerge(et.v, em.v, case.correction, **kw)
            want = merge_rule.merge(et.inner, em.inner, case.correction, case.footprint, case.conflict, case.grow)
            same_merge(got, want)
            case.check(want)
            assert np.array_equal(got.cells(), ref_cells) and np.array_equal(got.codes(), ref_codes) and without_times(got.stats) == ref_stats, (lt, lm, ft, fm)
            et.untouched(); em.untouched()
            got.close(); et.close(); em.close()
            ran += 1
    assert ran >= 6


@pytest.mark.parametrize("case", OBSERVE_ROWS, ids=names(OBSERVE_ROWS))
def test_the_change_layer_and_what_its_view_feeds(kartohip_lib, oracle_lib, case):
    """observe, diff, the changed list, read and view; the layer takes the view's stride, so its own view has an odd one -- that
    view goes on into MapField and MapMerge"""
    view, w = case.view, case.view["width"]
    t = DeviceView(ev.tight(view))
    ref_layer = MapChanges(t.v)
    ref_labels = ref_layer.observe(case.laser, case.ranges, case.poses, case.tolerance)
    ref_diff, ref_read, ref_nav = ref_layer.diff(0, 0.4), ref_layer.read(), ref_layer.nav()
    ref_layer.close(); t.close()
    moving = lc.view_of(lc.random_cells(np.random.default_rng(61), 15, 18, p_free=0.4, p_occ=0.2), view["anchor"], view["scale"], view["ox"] + 3, view["oy"] - 4)
    dm = DeviceView(moving)
    for e in placements(view):
        layer, rules = MapChanges(e.v), changes_rule.Layer(e.inner)
        assert layer.width_step == e.layout.stride
        got = layer.observe(case.laser, case.ranges, case.poses, case.tolerance)
        want = rules.observe(case.laser, case.ranges, case.poses, case.tolerance)
        assert np.array_equal(got.reshape(want.shape), want) and np.array_equal(got, ref_labels)
        e.untouched()
        d, wd = layer.diff(0, 0.4), rules.diff(0, 0.4)
        r = layer.read()
        assert np.array_equal(r["passes"], rules.passes) and np.array_equal(r["hits"], rules.hits)
        assert np.array_equal(r["codes"], wd["codes"]) and np.array_equal(r["patched"], wd["patched"])
        assert np.array_equal(d["counts"], wd["counts"]) and np.array_equal(d["cells"], wd["cells"]) and d["n_changed"] == len(wd["cells"])
        assert np.array_equal(d["cells"], ref_diff["cells"]) and np.array_equal(d["counts"], ref_diff["counts"])
        for k in ("passes", "hits", "codes", "patched"):
            assert np.array_equal(r[k][:, :w], ref_read[k][:, :w]), k
        assert np.array_equal(layer.nav(), ref_nav)
        e.untouched()
        # the layer's own view: the patched cells at the view's stride
        v = layer.view()
        assert (v.width, v.height, v.width_step, v.ox, v.oy) == (w, view["height"], e.layout.stride, view["ox"], view["oy"])
        patched = dict(e.inner, cells=wd["patched"])
        for radius, obstacles in ((3, field_rule.OCCUPIED), (0, field_rule.NOT_FREE)):
            field = MapField(v, max_distance=radius / view["scale"], obstacles=obstacles)
            same_field(field, field_rule.d2_brute(patched, radius, obstacles), view, radius)
            field.close()
        for correction in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.4)):
            merged = MapMerge(v, dm.v, correction)
            same_merge(merged, merge_rule.merge(patched, moving, correction))
            merged.close()
        assert np.array_equal(layer.read()["patched"], wd["patched"]), "a reader wrote the layer's view"
        e.untouched()
        layer.close()
    dm.close()


def test_the_localizers_map(kartohip_lib, oracle_lib):
    """kh_map_localizer_set_map, then the expected scan and the field of that map"""
    from test_map_localize_gpu import PARAMS
    case = RAY_ROWS[0]
    view = case.view
    loc = MapLocalizer(PARAMS, case.laser, max_batch=2)
    want_cast = ray_rule.cast_poses(view, case.laser, case.poses, 3)
    want_d2 = field_rule.d2_brute(view, 5)
    for e in placements(view):
        loc.set_map(e.v)
        same_cast(loc.expected(case.poses, 3), want_cast)
        field = loc.field(max_distance=5 / view["scale"])
        same_field(field, want_d2, view, 5)
        field.close()
    loc.close()


def test_an_alignment_of_two_embedded_maps(kartohip_lib, oracle_lib):
    """kh_map_align reads the moving map (its seeds, its cast scans) and the localizer's map (the relocalizations, the fits): both
    embedded, against both tight.  The tight pair is held against the rule by tests/test_map_align_gpu.py"""
    import map_align_cases as ac
    from common import LASER
    from test_map_localize_gpu import PARAMS
    target, moving = ac.maps()
    loc = MapLocalizer(PARAMS, LASER, max_batch=32)
    dt, dm = DeviceView(ev.tight(target.view)), DeviceView(ev.tight(moving.view))
    ref, _ = loc.set_map(dt.v).align(dm.v, relocalize=ac.RELOCALIZE, **ac.SETTING)
    dt.close(); dm.close()
    et, em = EmbeddedView(target.view, "L2", 255), EmbeddedView(moving.view, "L3", 100)
    got, _ = loc.set_map(et.v).align(em.v, relocalize=ac.RELOCALIZE, **ac.SETTING)
    assert len(got) == len(ref) > 1
    for c, r in zip(got, ref):
        assert (c.index, c.probe_seed, c.hypothesis, c.enough) == (r.index, r.probe_seed, r.hypothesis, r.enough)
        assert np.array_equal(bits(c.correction), bits(r.correction)) and np.array_equal(bits(c.fine_response), bits(r.fine_response))
        same_fit(c.fit, r.fit)
    et.untouched(); em.untouched()
    loc.close()
    et.close(); em.close()


@pytest.mark.parametrize("case", FIELD_ROWS, ids=names(FIELD_ROWS))
def test_field_create_and_its_readers(kartohip_lib, case):
    view, r = case.view, case.radius
    t = DeviceView(ev.tight(view))
    ref = MapField(t.v, max_distance=r / view["scale"], obstacles=case.obstacles)
    t.close()
    ref_d2, ref_stats = ref.d2, without_times(ref.stats)
    inflation = cases.inflation_for(r)
    ox, oy, w, h = view["ox"], view["oy"], view["width"], view["height"]
    rect = (ox + min(1, w - 1), oy + min(2, h - 1), max(1, w - 2), max(1, h - 3))
    for e in placements(view):
        got = MapField(e.v, max_distance=r / view["scale"], obstacles=case.obstacles)
        e.untouched()
        want = field_rule.d2_brute(e.inner, r, case.obstacles)
        same_field(got, want, view, r)
        case.check(got.d2)
        assert np.array_equal(got.d2, ref_d2) and without_times(got.stats) == ref_stats
        if inflation is not None:
            costs = field_rule.costs(e.inner, want, r, **inflation)
            assert np.array_equal(got.costs(**inflation), costs) and np.array_equal(got.costs(**inflation), ref.costs(**inflation))
            block = got.costs_rect(*rect, **inflation)
            assert np.array_equal(block, costs[rect[1] - oy:rect[1] - oy + rect[3], rect[0] - ox:rect[0] - ox + rect[2]])
        pts = fc.clearance_points(view, want)
        metres, status, value = got.clearance(pts)
        want_m, want_s, want_v = field_rule.clearance(e.inner, want, pts)
        assert np.array_equal(status, want_s) and np.array_equal(value, want_v) and np.array_equal(bits(metres), bits(want_m))
        got.close()
    ref.close()


# ---------------------------------------------------------------- MapField.update
class Twins:
    """the same field twice: one follows the view in a layout, one the same window in a tight, aligned buffer.  Every step goes to
    both (Followed.step holds what is reported against the case table, the values against the rule and a fresh field); the two
    reports and the two fields must be equal, and the embedded buffer as it was uploaded."""

    def __init__(self, view, radius, obstacles, name, fill):
        self.a = Followed(view, radius, obstacles, d2_rule=field_rule.d2_brute, place=lambda v: EmbeddedView(v, name, fill))
        self.b = Followed(ev.tight(view), radius, obstacles, d2_rule=field_rule.d2_brute)
        self.a.d.untouched()

    def band(self, rows):
        self.a.field.set_band_rows(rows)
        self.b.field.set_band_rows(rows)

    def step(self, after, rect=None):
        got, ref = self.a.step(after, rect), self.b.step(ev.tight(after), rect)
        assert {k: got[k] for k in REPORTED} == {k: ref[k] for k in REPORTED}
        assert np.array_equal(self.a.field.d2, self.b.field.d2)
        self.a.d.untouched()
        return got

    def close(self):
        self.a.close()
        self.b.close()


def every_placement(width):
    return [(name, fill) for name in ev.layouts_for(width) for fill in ev.FILLS]


@pytest.mark.parametrize("name, fill", every_placement(37))
def test_update_rectangles_at_every_residue(kartohip_lib, name, fill):
    forms = uc.rect_forms() + cases.rect_forms_mod4()
    f = Twins(forms[0].before, forms[0].radius, forms[0].obstacles, name, fill)
    for e in forms:
        got = f.step(e.after, e.rect)
        assert got["values_box"] == (9, 10, 12, 10)
        f.step(e.before, e.rect)
    f.close()


@pytest.mark.parametrize("edit", SHAPE_EDITS, ids=names(SHAPE_EDITS))
def test_update_window_shapes(kartohip_lib, edit):
    for name, fill in every_placement(edit.before["width"]):
        f = Twins(edit.before, edit.radius, edit.obstacles, name, fill)
        for band in (1, 0):
            f.band(band)
            f.step(edit.after)
            f.step(edit.before)
        f.close()


@pytest.mark.parametrize("fill", ev.FILLS)
def test_update_random_rounds_on_the_rotating_layout(kartohip_lib, fill):
    rounds = uc.random_rounds(**cases.RANDOM_ROUNDS)
    first, _ = next(rounds)
    f = Twins(first, cases.RANDOM_RADIUS, cases.RANDOM_ROUNDS["obstacles"], "L3", fill)
    smaller = 0
    for after, rect in rounds:
        got = f.step(after, rect)
        smaller += 0 < got["cells_recomputed"] < 40 * 50
    assert smaller > 0, "no round recomputed less than the window"
    f.close()
