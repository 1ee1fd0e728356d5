"""GPU: the map change layer (kh_map_changes_*; k_map_observe, k_map_diff, k_map_changed, k_map_decay in csrc/occupancy_changes.hip) against
tests/map_changes_rule.py, exactly: pass, hits, labels, codes, counts, patched cells, the changed-cell list and its order -- on the
hand-made views of tests/map_localize_cases.py and tests/map_changes_cases.py, then end to end on the small map: an unchanged world, a
changed one, and through the map localizer.  After every call the source view's cells are downloaded and must be unchanged."""
import math

import numpy as np
import pytest

import map_changes_cases as cc
import map_changes_rule as rule
import map_localize_cases as cases
import map_localize_rule as ml
import map_match_rule as mr
from common import LASER, OFFLINE_PARAMS, bits
from slam_toolbox_amd import capi, synth
from slam_toolbox_amd.map_changes import MapChanges
from slam_toolbox_amd.map_localizer import MapLocalizer, TrackStep, TrackStepObserved
from test_map_fit_gpu import same_fit
from test_map_seeds_gpu import DeviceView

pytestmark = pytest.mark.gpu

OBSERVE_CASES = cc.observe_cases()
UNIT_CASES = cc.unit_cases()
F, O, U = cc.F, cc.O, cc.U


class Pair:
    """a layer of the library and the rule's on the same view; every call goes to both and the view's cells must stay as they were"""

    def __init__(self, view):
        self.view, self.d = view, DeviceView(view)
        self.lib, self.rule = MapChanges(self.d.v), rule.Layer(view)

    def untouched(self):
        assert np.array_equal(self.d.download(), self.view["cells"].ravel()), "the view's cells were written"

    def observe(self, laser, ranges, poses, t=1):
        got = self.lib.observe(laser, ranges, poses, t)
        want = self.rule.observe(laser, ranges, poses, t)
        assert got.dtype == np.int32 and np.array_equal(got.reshape(want.shape), want), np.argwhere(got.reshape(want.shape) != want)[:5]
        self.untouched()
        return want

    def same_layer(self):
        r = self.lib.read()
        assert np.array_equal(r["passes"], self.rule.passes) and np.array_equal(r["hits"], self.rule.hits)
        self.untouched()
        return r

    def diff(self, min_pass=2, threshold=0.1, cap=None):
        got, want = self.lib.diff(min_pass, threshold, cap), self.rule.diff(min_pass, threshold)
        r = self.same_layer()
        assert np.array_equal(r["codes"], want["codes"]) and np.array_equal(r["patched"], want["patched"])
        assert np.array_equal(got["counts"], want["counts"]) and got["counts"].sum() == self.view["width"] * self.view["height"]
        n = len(want["cells"])
        listed = n if cap is None else min(n, cap)
        assert got["n_changed"] == n == want["counts"][2:].sum() and got["n_listed"] == listed
        assert np.array_equal(got["cells"], want["cells"][:listed]), "the changed cells, in row-major order"
        assert got["scans_observed"] == self.rule.scans and got["beams_observed"] == self.rule.beams
        return got, want

    def close(self):
        self.lib.close()
        self.d.close()


@pytest.mark.parametrize("case", OBSERVE_CASES, ids=[c.name for c in OBSERVE_CASES])
def test_observe_cases(kartohip_lib, oracle_lib, case):
    p = Pair(case.view)
    p.observe(case.laser, case.ranges, case.poses, case.tolerance)
    p.same_layer()
    p.diff(0, 0.4)
    p.diff()
    p.close()


def test_two_scans_on_the_same_cells_sum(kartohip_lib, oracle_lib):
    case = next(c for c in OBSERVE_CASES if c.name.startswith("all eight octants"))
    p = Pair(case.view)
    ranges, poses = np.repeat(case.ranges, 2, axis=0), np.repeat(case.poses, 2, axis=0)
    p.observe(case.laser, ranges, poses)
    r = p.same_layer()
    assert r["passes"].max() == 2 * 16 and r["hits"].sum() == 2 * 16, "the sensor's cell: 16 beams of each of the two scans"
    once = rule.Layer(case.view)
    once.observe(case.laser, case.ranges, case.poses)
    assert np.array_equal(r["passes"], 2 * once.passes) and np.array_equal(r["hits"], 2 * once.hits)
    p.observe(case.laser, case.ranges, case.poses)            # ... and a second call on top of the first
    assert np.array_equal(p.same_layer()["passes"], 3 * once.passes)
    p.close()


def test_tolerances_with_the_end_cell_in_a_window_corner(kartohip_lib, oracle_lib):
    view = cc.corner_view()
    corners = [(-6, -4), (6, 4), (6, -4), (-6, 4)]
    ranges, poses = cc.spots(view, corners)
    want = {0: [rule.NOVEL] * 4, 1: [rule.NOVEL] * 4, 2: [rule.EXPLAINED, rule.NOVEL, rule.NOVEL, rule.NOVEL],
            4: [rule.EXPLAINED, rule.EXPLAINED, rule.NOVEL, rule.NOVEL]}
    for t in cc.TOLERANCES:
        p = Pair(view)
        labels = p.observe(cc.spot_laser(), ranges, poses, t)
        assert labels[:, 0, 0].tolist() == want[t] and not labels[:, 0, 1].any(), t
        p.diff(0, 0.1)
        p.close()
    # a beam along the first row into the first corner, past the padding's 100 on the row above's end
    p = Pair(view)
    labels = p.observe(cases.circle(1), [[2.0]], [(0.5, -1.0, 0.0)], 4)
    assert labels[0, 0].tolist() == [rule.EXPLAINED, 0]
    p.close()


def test_diff_lists_around_the_unit_boundaries(kartohip_lib, oracle_lib):
    """zero changes, one change, changes in the last column of a width that is no multiple of 64 and on either side of a 64-cell unit
    boundary; cap 0 and a cap below the total"""
    view = cc.wide_view()
    ox, oy = view["ox"], view["oy"]
    p = Pair(view)
    got, _ = p.diff(0, 0.1)
    assert got["n_changed"] == 0 and got["counts"].tolist() == [130 * 3, 0, 0, 0, 0, 0] and got["cells"].shape == (0, 3)
    laser = cc.spot_laser()
    p.observe(laser, *cc.spots(view, [(ox + 64, oy + 1)]))
    got, _ = p.diff(0, 0.1)
    assert got["cells"].tolist() == [[ox + 64, oy + 1, rule.APPEARED]] and got["counts"].tolist() == [130 * 3 - 1, 0, 1, 0, 0, 0]
    more = [(ox + 129, oy), (ox + 63, oy + 2), (ox + 64, oy + 2), (ox, oy), (ox + 129, oy + 2), (ox + 127, oy + 1), (ox + 128, oy + 1), (ox + 63, oy)]
    p.observe(laser, *cc.spots(view, more))
    got, want = p.diff(0, 0.1)
    assert got["n_changed"] == 9 and got["cells"][:, 0].tolist() == [ox, ox + 63, ox + 129, ox + 64, ox + 127, ox + 128, ox + 63, ox + 64, ox + 129]
    for cap in (0, 1, 4, 8, 9, 20):
        got, _ = p.diff(0, 0.1, cap)
        assert got["n_changed"] == 9 and len(got["cells"]) == min(cap, 9)
    # no more than `cap` entries are written: the caller's room past them stays as it was
    room = np.full((9, 3), -77, dtype=np.int32)
    s = capi.KhMapChangesSummary()
    capi.check(kartohip_lib.kh_map_changes_diff(p.lib._h, 0, 0.1, room.ctypes.data, 4, s), "kh_map_changes_diff")
    assert s.n_changed == 9 and s.n_listed == 4 and np.array_equal(room[:4], want["cells"][:4]) and (room[4:] == -77).all()
    assert s.diff_kernel_ms > 0 and s.list_kernel_ms > 0 and s.observe_kernel_ms > 0
    p.close()


@pytest.mark.parametrize("case", UNIT_CASES, ids=[c.name for c in UNIT_CASES])
def test_unit_cases(kartohip_lib, oracle_lib, case):
    """views of 1023 .. 35 200 units (tests/map_changes_cases.py): the second and later trips of k_map_changed's strided loop, and
    k_map_changed_scan with more than one unit per thread; the whole list, no list, and lists cut at the caps of the case"""
    p = Pair(case.view)
    p.observe(case.laser, case.ranges, case.poses)
    for cap in case.caps:
        got, _ = p.diff(case.min_pass, case.threshold, cap)
        assert got["n_changed"] > max(c or 0 for c in case.caps) or case.n_units == cc.TRIP_UNITS + 1
    if case.name == cc.ROOM_CASE:
        # no more than `cap` entries are written, by any trip: the caller's room past them stays as it was
        want, cap = p.rule.diff(case.min_pass, case.threshold)["cells"], case.caps[-1]
        room = np.full((len(want), 3), -77, dtype=np.int32)
        s = capi.KhMapChangesSummary()
        capi.check(kartohip_lib.kh_map_changes_diff(p.lib._h, case.min_pass, case.threshold, room.ctypes.data, cap, s), "kh_map_changes_diff")
        assert s.n_changed == len(want) and s.n_listed == cap and np.array_equal(room[:cap], want[:cap]) and (room[cap:] == -77).all()
    if case.name == cc.DECAY_CASE:
        # a count phase over a unit buffer that holds the prefix of the diff before: after the decay only the end cell is observed
        p.lib.decay(1)
        p.rule.decay(1)
        got, _ = p.diff(case.min_pass, case.threshold)
        assert got["counts"][rule.UNOBSERVED] == case.view["height"] - 1 and got["n_changed"] == 1
        p.observe(case.laser, case.ranges, case.poses)          # ... and the dense list again, over the buffer of the sparse one
        got, _ = p.diff(case.min_pass, case.threshold, case.caps[-1])
        assert got["n_listed"] == case.caps[-1]
    p.close()


def test_thresholds_a_map_state_of_7_and_decay(kartohip_lib, oracle_lib):
    cells = np.full((4, 70), F, dtype=np.uint8)
    cells[1, 5], cells[1, 6], cells[2, 66], cells[3, 3] = 7, 7, O, U
    view = cases.view_of(cells, (2.0, -3.0), 4.0, 5, -9, padding=O)
    spot = lambda i, j: (5 + i, -9 + j)                        # noqa: E731
    p = Pair(view)
    laser = cc.spot_laser()
    # every spot: pass 2, hits 1
    p.observe(laser, *cc.spots(view, [spot(0, 0), spot(5, 1), spot(66, 2), spot(3, 3), spot(69, 0)]))
    got, _ = p.diff(2, 0.1)
    assert got["n_changed"] == 0 and got["counts"][rule.UNOBSERVED] == 4 * 70, "pass == min_pass_through is not observed"
    got, _ = p.diff(1, 0.5)
    assert got["cells"][:, 2].tolist() == [rule.DISCOVERED_FREE, rule.VANISHED, rule.DISCOVERED_FREE], "hits / pass == threshold is free"
    assert got["counts"][rule.CONFIRMED] == 2
    got, _ = p.diff(1, math.nextafter(0.5, 0.0))
    assert got["cells"].tolist() == [[5, -9, 2], [74, -9, 2], [10, -8, 4], [8, -6, 4]], "... and above it occupied; a state of 7 counts as unknown"
    assert p.lib.read()["patched"][1, 6] == 7, "an unobserved cell keeps the map's state, whatever it is"
    # a clipped beam over the 7s and the free cells, three times: pass 3 on its line; then a decay
    line = cases.circle(1, range_threshold=3.0)
    for _ in range(3):
        p.observe(line, [[4.0]], [(view["anchor"][0] + 6 / 4.0, view["anchor"][1] - 8 / 4.0, math.pi)])
    got, _ = p.diff(2, 0.1)
    assert got["counts"].tolist() == [4 * 70 - 13, 11, 0, 0, 1, 1], "columns 1 .. 13 of row 1: eleven free cells, the 7 with the spot's hit, the other 7"
    p.lib.decay(1)
    p.rule.decay(1)
    r = p.same_layer()
    assert r["passes"][1, 6] == 1 and r["passes"][1, 5] == 2 and r["hits"][1, 5] == 0, "3 >> 1, 5 >> 1, 1 >> 1"
    got, _ = p.diff(0, 0.1)
    assert got["counts"][rule.DISCOVERED_FREE] == 3 and got["counts"][rule.VANISHED] == 1 and got["counts"][rule.APPEARED] == 0
    p.lib.decay(31)
    p.rule.decay(31)
    got, _ = p.diff(0, 0.1)
    assert got["counts"][rule.UNOBSERVED] == 4 * 70
    # clear: the counters of scans and beams start again
    p.observe(laser, *cc.spots(view, [spot(0, 0)]))
    p.lib.clear()
    p.rule.clear()
    got, _ = p.diff(0, 0.1)
    assert got["scans_observed"] == 0 and got["counts"][rule.UNOBSERVED] == 4 * 70
    p.close()


def test_a_refused_observe_changes_nothing(kartohip_lib, oracle_lib):
    case = next(c for c in OBSERVE_CASES if c.name.startswith("all eight octants"))
    p = Pair(case.view)
    p.observe(case.laser, case.ranges, case.poses)
    before = p.lib.read()
    good = case.poses[0]

    def refused(laser, ranges, poses, t=1):
        with pytest.raises(capi.KartoHipError) as e:
            p.lib.observe(laser, ranges, poses, t)
        assert e.value.code == capi.KH_ERR_INVALID_ARG
        with pytest.raises(rule.Refused):
            p.rule.observe(laser, ranges, poses, t)
    for pose in cases.REFUSED_POSES:
        refused(case.laser, np.repeat(case.ranges, 2, axis=0), [good, pose])
    far = cases.circle(16, range_threshold=(2 ** 20 - 1) / case.view["scale"], max_range=1e9)
    refused(far, case.ranges, [good])
    for t in (-1, 5):
        refused(case.laser, case.ranges, [good], t)
    for shift in (0, 32):
        with pytest.raises(capi.KartoHipError) as e:
            p.lib.decay(shift)
        assert e.value.code == capi.KH_ERR_INVALID_ARG
    after = p.same_layer()
    assert all(np.array_equal(before[k], after[k]) for k in ("passes", "hits")), "a refused call wrote the layer"
    got, _ = p.diff(0, 0.1)
    assert got["scans_observed"] == 1 and got["beams_observed"] == 16
    p.close()


def test_handle_states(kartohip_lib, oracle_lib):
    view = cc.wide_view(20, 5)
    d = DeviceView(view)
    layer = MapChanges(d.v)
    for call in (layer.view, layer.nav):
        with pytest.raises(capi.KartoHipError) as e:
            call()
        assert e.value.code == capi.KH_ERR_NOT_FOUND, "before a diff"
    r = layer.read()
    assert not any(v.any() for v in r.values()), "zero at creation"
    layer.diff()
    v = layer.view()
    assert (v.width, v.height, v.width_step, v.ox, v.oy, v.scale, v.device) == (20, 5, 24, view["ox"], view["oy"], 4.0, 0)
    assert v.device_cells != d.v.device_cells and tuple(v.anchor) == view["anchor"]
    assert np.array_equal(layer.nav(), rule.nav_of(view["cells"], 20)), "nothing observed: the patched map is the map"
    layer.close()
    d.close()


# ---------------------------------------------------------------- end to end on the small map
@pytest.fixture(scope="module")
def small(kartohip_lib, oracle_lib):
    sm, m = cases.small_map()
    d = DeviceView(m.view)
    yield sm, m, d
    d.close()


def test_unchanged_world(small):
    """the eight scans that built the map, observed at their own poses: nothing changed, every observed cell confirmed, the patched nav
    values the map's -- exactly: the counters, the lattice and the thresholds are the map's own"""
    sm, m, d = small
    p = Pair(m.view)
    p.observe(LASER, np.array(sm.ranges), sm.poses)
    got, _ = p.diff()
    assert got["n_changed"] == 0 and got["counts"][2:].sum() == 0
    assert got["counts"][rule.CONFIRMED] == (m.view["cells"][:, :m.width] != U).sum() > 0
    assert np.array_equal(p.lib.nav(), m.nav)
    print(f"unchanged world: observe {got['observe_kernel_ms']:.3f} ms for {got['beams_observed']} beams, diff {got['diff_kernel_ms']:.3f} ms, "
          f"list {got['list_kernel_ms']:.3f} ms, download {got['download_ms']:.3f} ms")
    p.close()


def test_changed_world(small):
    """a pallet across the aisle and the first rack gone (tests/map_changes_cases.py): the library equals the rule, the patched map the
    occupancy oracle of the scan wherever it was observed, and the three geometric statements hold for the library's own answer"""
    from oracle import karto
    sm, m, d = small
    cw = cc.changed_world()
    p = Pair(m.view)
    labels = p.lib.observe(LASER, cw.ranges, cw.pose, 1)
    assert np.array_equal(labels, p.rule.observe(LASER, [cw.ranges], [cw.pose], 1)[0])
    got, _ = p.diff()
    cc.check_changed_world(m.view, LASER, cw, labels, got)
    cells, passes, _ = karto.occupancy_from_scans(m.width, m.height, m.offset, cases.RESOLUTION, [karto.Scan(cw.ranges, cw.pose, LASER)], LASER)
    seen = passes[:, :m.width] > 2
    patched = p.lib.read()["patched"]
    assert np.array_equal(patched[:, :m.width][seen], cells[:, :m.width][seen])
    assert np.array_equal(patched[:, :m.width][~seen], m.view["cells"][:, :m.width][~seen])
    assert np.array_equal(p.lib.nav(), rule.nav_of(patched, m.width))
    print(f"changed world: counts {got['counts'].tolist()}, labels {np.bincount(labels[:, 0], minlength=6).tolist()}")
    p.close()


def test_through_the_localizer(kartohip_lib, oracle_lib):
    """The setting of test_map_localises_like_a_chain: the map of 40 trajectory scans, then scans 40 .. 45 tracked with a layer: the layer
    equals the rule's after observing each scan at the step's returned sensor pose, the steps are those of a localizer without a layer
    bit for bit, and a step on the patched map equals the rule on the patched view."""
    from oracle import karto
    create = (0.3, 0.01, 0.03)
    params = dict(correlation_search_space_dimension=create[0], correlation_search_space_resolution=create[1],
                  correlation_search_space_smear_deviation=create[2])
    world, rng = synth.make_world(12345), np.random.default_rng(77)
    truth, _ = synth.trajectory(60)
    ranges = [synth.make_scan(world, truth[i], rng) for i in range(47)]
    m = cases.occupancy_map(ranges[:40], truth[:40], LASER)
    p = Pair(m.view)
    loc, plain = MapLocalizer(params, LASER, max_batch=1).set_map(p.d.v), MapLocalizer(params, LASER, max_batch=1).set_map(p.d.v)
    drift = np.array([0.06, -0.05, 0.02])
    loc.set_pose(truth[39])
    plain.set_pose(truth[39])
    for i in range(40, 46):
        got, want = loc.process(ranges[i], truth[i] + drift, changes=p.lib), plain.process(ranges[i], truth[i] + drift)
        assert isinstance(got, TrackStepObserved) and type(want) is TrackStep
        for a, b in zip(got[:5], want[:5]):
            assert np.array_equal(bits(a), bits(b)), i
        same_fit(got.fit, want.fit)
        assert got.fit["known"] > 0 and got.labels is not None and got.labels.shape == (LASER.n_beams, 2)
        assert np.array_equal(got.labels, p.rule.observe(LASER, [ranges[i]], [got.sensor_pose], 1)[0]), i
        p.same_layer()
    # a step that is not trusted teaches the layer nothing
    held = loc.get_pose()
    step = loc.process(ranges[45], truth[45] + drift, changes=p.lib, min_fit_score=1.5)
    assert step.labels is None
    loc.set_pose(*held)
    p.same_layer()
    got, _ = p.diff()
    assert got["scans_observed"] == 6 and got["counts"][rule.CONFIRMED] > 0
    # the patched map back into the localizer
    patched = rule.patched_view(m.view, p.rule.diff()["patched"])
    loc.set_map(p.lib.view())
    odometric = truth[46] + drift
    step = loc.process(ranges[46], odometric)
    seq = karto.Matcher(*create, LASER.range_threshold, OFFLINE_PARAMS)
    want = ml.track_step(patched, mr.map_points(patched), LASER, seq, OFFLINE_PARAMS, held[0], held[1], ranges[46], odometric)
    for a, b in ((step.predicted_pose, want.predicted), (step.sensor_pose, want.sensor_pose), (step.covariance, want.covariance),
                 (step.response, want.response), (step.robot_pose, want.robot_pose)):
        assert np.array_equal(bits(a), bits(b)), (a, b)
    same_fit(step.fit, want.fit)
    p.untouched()
    loc.close(); plain.close(); p.close()
