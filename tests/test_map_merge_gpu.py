"""GPU: the map merge (kh_map_merge_*, MapMerge; k_map_known_box and k_map_merge in csrc/occupancy_map.hip) against
tests/map_merge_rule.py on the hand-made views of tests/map_merge_cases.py, uploaded through kh_device_upload, and on the real pair of
tests/map_align_cases.py: cells, codes, all six counters, the bits of the agreement, the known box and the output window are the
rule's exactly, and both inputs are byte-identical afterwards.  Through that identity the CPU conditions of
tests/test_map_merge_rule_oracle.py on the real pair hold on the device."""
import ctypes as C

import numpy as np
import pytest

import map_align_cases as ac
import map_localize_cases as lc
import map_localize_rule as ml
import map_match_rule as mr
import map_merge_cases as cases
import map_merge_rule as rule
from common import LASER, bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_changes import MapChanges
from slam_toolbox_amd.map_localizer import MapLocalizer, map_fit
from slam_toolbox_amd.map_merge import MapMerge
from test_map_fit_gpu import same_fit
from test_map_localize_gpu import PARAMS
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

MERGE_CASES = cases.merge_cases()
NAV = np.full(256, -1, dtype=np.int8)
NAV[100], NAV[255] = 100, 0


def same_merge(got, want):
    st = got.stats
    assert (st["ox"], st["oy"], st["width"], st["height"], st["width_step"]) == tuple(want.window), (st, want.window)
    assert st["footprint"] == want.footprint and tuple(st["known_box"]) == tuple(want.known_box), (st["known_box"], want.known_box)
    assert {k: st[k] for k in rule.COUNTERS} == want.counters, (st, want.counters)
    assert st["overlap"] == want.overlap and np.array_equal(bits(st["agreement"]), bits(want.agreement))
    cells, codes = got.cells(), got.codes()
    assert np.array_equal(codes, want.codes), f"{int((codes != want.codes).sum())} codes differ"
    assert np.array_equal(cells, want.cells), f"{int((cells != want.cells).sum())} cells differ"
    assert np.array_equal(got.nav(), NAV[want.cells[:, :want.window.width]])
    v = got.view
    assert (v.ox, v.oy, v.width, v.height, v.width_step) == tuple(want.window) and v.device_cells
    assert (v.anchor[0], v.anchor[1], v.scale) == (*want.view["anchor"], want.view["scale"])


@pytest.mark.parametrize("case", MERGE_CASES, ids=[c.name for c in MERGE_CASES])
def test_merge_cases(kartohip_lib, case):
    dt, dm = DeviceView(case.target), DeviceView(case.moving)
    got = MapMerge(dt.v, dm.v, case.correction, footprint=case.footprint, conflict=case.conflict, grow=case.grow)
    want = rule.merge(case.target, case.moving, case.correction, case.footprint, case.conflict, case.grow)
    same_merge(got, want)
    case.check(want)
    assert np.array_equal(dt.download(), case.target["cells"].ravel()) and np.array_equal(dm.download(), case.moving["cells"].ravel()), "an input was written"
    assert got.stats["times_ms"][2] >= got.stats["times_ms"][0] + got.stats["times_ms"][1] - 1e-3
    got.close()
    dt.close(); dm.close()


def test_a_merge_whose_target_is_another_merge(kartohip_lib):
    rng = np.random.default_rng(5)
    a = lc.view_of(lc.random_cells(rng, 20, 31), cases.A, cases.K, -4, 3)
    b = lc.view_of(lc.random_cells(rng, 25, 18), cases.A, cases.K, 2, -6)
    c = lc.view_of(lc.random_cells(rng, 40, 44), (0.1, 0.2), 2 * cases.K, -9, -9)
    da, db, dc = DeviceView(a), DeviceView(b), DeviceView(c)
    first = MapMerge(da.v, db.v, (0.3, 0.2, 0.5))
    want_first = rule.merge(a, b, (0.3, 0.2, 0.5))
    second = MapMerge(first, dc.v, (-0.4, 0.1, -1.2), conflict="moving")
    same_merge(second, rule.merge(want_first.view, c, (-0.4, 0.1, -1.2), conflict=rule.CONFLICT_MOVING))
    same_merge(first, want_first)                              # the first merge is an input like any other: left as it was
    second.close(); first.close()
    for d in (da, db, dc):
        d.close()


def test_refusals(kartohip_lib):
    L = kartohip_lib
    rng = np.random.default_rng(6)
    t, m = lc.view_of(lc.random_cells(rng, 7, 12), cases.A, cases.K), lc.view_of(lc.random_cells(rng, 6, 5), cases.A, cases.K)
    dt, dm = DeviceView(t), DeviceView(m)

    def refused(code, target, moving, correction, **kw):
        with pytest.raises(capi.KartoHipError) as e:
            MapMerge(target, moving, correction, **kw)
        assert e.value.code == code, (e.value.code, kw)
    other = capi.KhMapView.from_buffer_copy(dm.v)
    other.device = 1
    refused(capi.KH_ERR_INVALID_ARG, dt.v, other, (0.0, 0.0, 0.0))
    refused(capi.KH_ERR_INVALID_ARG, dt.v, dm.v, (1e12, 0.0, 0.0))
    refused(capi.KH_ERR_INVALID_ARG, dt.v, dm.v, (0.0, -1e12, 0.3))
    far = MapMerge(dt.v, dm.v, (1e12, 0.0, 0.0), grow=0)     # not grown: every sample falls beyond the moving lattice and reads unknown
    same_merge(far, rule.merge(t, m, (1e12, 0.0, 0.0), grow=0))
    far.close()
    # the size caps: refused from the window plan, before a cell of the target is read (these views name more cells than their buffer holds)
    for width, height in ((32769, 1), (32768, 8193)):
        big = capi.KhMapView.from_buffer_copy(dt.v)
        big.width, big.height, big.width_step = width, height, width
        refused(capi.KH_ERR_INVALID_ARG, big, dm.v, (0.0, 0.0, 0.0))
        refused(capi.KH_ERR_INVALID_ARG, big, dm.v, (0.0, 0.0, 0.0), grow=0)
    refused(capi.KH_ERR_INVALID_ARG, dt.v, dm.v, (32766.7 / cases.K + 1.5, 0.0, 0.0))      # grown to a side of more than 32768 cells
    for kw in (dict(footprint=5), dict(conflict=4), dict(grow=2)):
        refused(capi.KH_ERR_INVALID_ARG, dt.v, dm.v, (0.0, 0.0, 0.0), **kw)
    h = C.c_void_p(1)
    p = capi.KhMapMergeParams()
    L.kh_map_merge_params_default(C.byref(p))
    assert L.kh_map_merge_create(C.byref(dt.v), C.byref(other), C.byref(p), C.byref(h)) == capi.KH_ERR_INVALID_ARG and h.value is None
    assert np.array_equal(dt.download(), t["cells"].ravel()) and np.array_equal(dm.download(), m["cells"].ravel())
    dt.close(); dm.close()


# ---------------------------------------------------------------- the real pair
@pytest.fixture(scope="module")
def pair(kartohip_lib, oracle_lib):
    """both maps in device memory of the test's own, a localizer on the target, the merge under the true correction"""
    target, moving, want = cases.real_pair()
    dt, dm = DeviceView(target.view), DeviceView(moving.view)
    loc = MapLocalizer(PARAMS, LASER, max_batch=32).set_map(dt.v)
    got = loc.merge(dm.v, cases.TRUTH, footprint=1, conflict="occupied", grow=1)
    yield target, moving, want, dt, dm, loc, got
    got.close()
    loc.close()
    dt.close(); dm.close()


def test_the_real_pair_equals_the_rule(pair):
    target, moving, want, dt, dm, loc, got = pair
    same_merge(got, want)
    print(f"window {tuple(want.window)}, counters {want.counters}, agreement {want.agreement:.5f}, times {got.stats['times_ms']}")
    assert np.array_equal(dt.download(), target.view["cells"].ravel()) and np.array_equal(dm.download(), moving.view["cells"].ravel())


def test_the_merged_view_is_a_map_like_any_other(pair):
    """the localizer, the matcher's map entry point and the change layer take it; a scan only the moving map saw fits it better than the target"""
    from test_map_match_gpu import LOOP, pair as matchers, scans_at
    import relocalize_cases as rc
    target, moving, want, dt, dm, loc, got = pair
    sm = rc.small_map()
    pose = np.asarray(sm.poses[7], dtype=np.float64)
    on_merged, on_target = map_fit(got.view, LASER, sm.ranges[7], [pose])[0], map_fit(dt.v, LASER, sm.ranges[7], [pose])[0]
    same_fit(on_merged, ml.fit(want.view, LASER, sm.ranges[7], pose))
    print(f"scan 7 at its true pose: known {on_merged['known']} on the merged map, {on_target['known']} on the target alone")
    assert on_merged["known"] > on_target["known"]
    other = MapLocalizer(PARAMS, LASER, max_batch=2).set_map(got)
    other.set_pose(pose)
    other.close()
    hm, om = matchers(LOOP)
    hq, _ = scans_at(pose)
    hm.AddMap(hq, got.view)
    assert np.array_equal(hm.GetCorrelationGrid(), mr.rule_grid(om, pose, mr.map_points(want.view)))
    hm.close()
    layer = MapChanges(got)
    assert (layer.width, layer.height, layer.width_step) == (want.window.width, want.window.height, want.window.width_step)
    layer.observe(LASER, sm.ranges[7], pose)
    assert layer.diff()["n_confirmed"] > 0
    layer.close()
    same_merge(got, want)                                      # ... and none of them wrote it


def test_the_best_alignment_merges_better_than_no_correction(pair):
    target, moving, want, dt, dm, loc, got = pair
    cands, _ = loc.align(dm.v, relocalize=ac.RELOCALIZE, **ac.SETTING)
    zero = next(c for c in cands if c.index == 0)
    assert cands[0].index != 0 and np.array_equal(zero.correction, np.zeros(3))
    best, none = loc.merge(dm.v, cands[0].correction), loc.merge(dm.v, zero.correction)
    same_merge(best, rule.merge(target.view, moving.view, cands[0].correction))
    print(f"agreement {best.stats['agreement']:.5f} under the best candidate, {none.stats['agreement']:.5f} under no correction, "
          f"{want.agreement:.5f} under the truth")
    assert best.stats["agreement"] > none.stats["agreement"] and best.stats["overlap"] > 0
    best.close(); none.close()


def test_merge_needs_a_map(kartohip_lib):
    fresh = MapLocalizer(PARAMS, LASER, max_batch=2)
    with pytest.raises(capi.KartoHipError) as e:
        fresh.merge(capi.KhMapView(), (0.0, 0.0, 0.0))
    assert e.value.code == capi.KH_ERR_NOT_FOUND
    fresh.close()
