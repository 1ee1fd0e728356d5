"""GPU: the session merger's two kernels (k_occ_trace_merged through MapMerger.merge, k_occ_fit_merged through MapMerger.fit) at the
edge inputs of tests/merge_cases.py, next to the rule (tests/merge_rule.py, tests/merge_fit_rule.py, ending at the occupancy oracle).
tests/test_merge_cases_oracle.py has shown on the CPU that every case sits on its edge.  Everything is exact: width, height, the
bits of the offset, pass, hits, cells; the six fit counters, agree, conflict, known and the bits of the score.

A hand-made submap goes through a Mapper without scan matching, one Process call per scan, every scan accepted; the rule's view of
it is tests/test_merge_gpu.py's _submap_of, with the mapper's own point readings -- which are also, bit for bit, those the cases
were checked with.  A mapper is made once per submap and borrowed by every merger that needs it."""
import numpy as np
import pytest

import merge_cases as mc
import merge_fit_rule as fr
import merge_rule as rule
import test_merge_fit_gpu as tf
import test_merge_gpu as tm
from common import bits
from slam_toolbox_amd import capi
from slam_toolbox_amd.merge import MapMerger

pytestmark = pytest.mark.gpu
TRACE, FIT = mc.trace_cases(), mc.fit_cases()


class Pool:
    """the mappers of the hand-made submaps and the rule's view of each, made on first use"""

    def __init__(self, tmp):
        self.tmp, self.made = tmp, {}

    def get(self, sub):
        if id(sub) not in self.made:
            from slam_toolbox_amd.mapper import Mapper
            m = Mapper(sub.laser, max_candidates=1, use_scan_matching=0, do_loop_closing=0)
            for k, (pose, ranges) in enumerate(sub.scans):
                assert m.Process(ranges, pose, float(k))[0], (k, pose)
            assert len(m.alive()) == len(sub.scans)
            want = mc.rule_submap(sub)
            if sub.scans:
                sm = tm._submap_of(m, sub.laser, self.tmp, f"sub{len(self.made)}")
                for got, made in zip(sm["scans"], want["scans"]):                # what the CPU checks were fed with
                    assert tm._same_bits(got["points"], made["points"]) and tm._same_bits(got["ranges"], made["ranges"])
                    assert np.array_equal(bits(got["corrected"]), bits(made["corrected"])) and np.array_equal(bits(got["box"]), bits(made["box"]))
            else:
                sm = want
            self.made[id(sub)] = (m, sm, sub)                                    # (sub: kept alive, so that its id stays its own)
        return self.made[id(sub)][:2]

    def merger(self, subs, transforms=None, resolution=mc.RES):
        """-> MapMerger, submap ids, rule submaps"""
        mg = MapMerger(resolution)
        ids, sms = [], []
        for k, sub in enumerate(subs):
            m, sm = self.get(sub)
            ids.append(mg.add_submap(m))
            sms.append(sm)
            if transforms is not None:
                mg.set_transform(ids[-1], transforms[k])
        return mg, ids, sms

    def close(self):
        for m, _, _ in self.made.values():
            m.close()


@pytest.fixture(scope="module")
def pool(kartohip_lib, tmp_path_factory):
    p = Pool(tmp_path_factory.mktemp("merge_edges"))
    yield p
    p.close()


def _grid_dict(g):
    p, h = g.counters()
    return {"width": g.width, "height": g.height, "offset": g.offset.copy(), "passes": p, "hits": h, "cells": g.cells()}


def _assert_grid(got, want):
    """an OccupancyGrid against merge_rule.merged_grid's dict"""
    assert (got.width, got.height) == (want["width"], want["height"])
    assert np.array_equal(bits(got.offset), bits(want["offset"]))
    p, h = got.counters()
    assert np.array_equal(p, want["passes"]) and np.array_equal(h, want["hits"])
    assert np.array_equal(got.cells(), want["cells"])


def _merge_is_the_rule(mg, sms, transforms, resolution=mc.RES, min_pass=2, threshold=0.1):
    got = mg.merge(min_pass, threshold)
    want = rule.merged_grid(sms, transforms, resolution, min_pass, threshold)
    _assert_grid(got, want)
    return got, want


# ---------------------------------------------------------------- k_occ_trace_merged
@pytest.mark.parametrize("case", TRACE, ids=[c.name for c in TRACE])
def test_trace_case(pool, case):
    mg, ids, sms = pool.merger(case.subs, case.transforms, case.resolution)
    got, want = _merge_is_the_rule(mg, sms, case.transforms, case.resolution, case.min_pass, case.threshold)
    case.check(mc.Ctx(case, sms, _grid_dict(got)))                              # the edge, on the library's own answer
    st = mg.stats()
    assert st["scans_traced"] == sum(len(s.scans) for s in case.subs)
    assert st["beams_traced"] == sum(len(s.scans) * s.laser.n_beams for s in case.subs)
    got.close(); mg.close()


def test_a_quarter_turn_transposes_and_mirrors_the_counters(pool):
    """device against device: the merge with every submap turned by +-pi / 2 about the origin is the identity merge transposed and
    mirrored (tests/test_merge_rule_oracle.py shows it for the rule; the lines of merge_cases.TURNED walk clear of TraceLine's ties)"""
    subs = [mc.FRAME, mc.TURNED]
    mg, ids, sms = pool.merger(subs)
    flat = mg.merge(0, 0.1)
    u = _grid_dict(flat)
    assert (u["width"], u["height"]) == (mc.W, mc.H)
    for yaw in (mc.PI / 2, -mc.PI / 2):
        for i in ids:
            mg.set_transform(i, (0.0, 0.0, yaw))
        turned = mg.merge(0, 0.1)
        mc.quarter_turn(u, _grid_dict(turned), yaw)
        turned.close()
    flat.close(); mg.close()


# ---------------------------------------------------------------- k_occ_fit_merged
@pytest.mark.parametrize("case", FIT, ids=[c.name for c in FIT])
def test_fit_case(pool, case):
    mg, ids, sms = pool.merger(list(case.others) + [case.moving], list(case.transforms) + [mc.IDENTITY], case.resolution)
    moving = ids[-1]
    grid = fr.reference_grid(sms[:-1], case.transforms, case.resolution, case.min_pass, case.threshold)
    want = fr.fit_on(sms[-1], case.candidates, grid, case.resolution)
    got = mg.fit(moving, case.candidates, case.min_pass, case.threshold)
    tf._same(got, want)
    case.check([{k: (float(g[k]) if k == "score" else int(g[k])) for k in fr.FIELDS} for g in got], grid)
    if case.own is not None:                                                    # the submap's own correction plays no part
        mg.set_transform(moving, case.own)
        again = mg.fit(moving, case.candidates, case.min_pass, case.threshold)
        assert again.tobytes() == got.tobytes()
    st = mg.fit_stats()
    assert st["candidates_total"] == len(case.candidates) * st["fits"]
    assert st["beam_candidates"] == len(case.candidates) * len(case.moving.scans) * case.moving.laser.n_beams
    mg.close()


def test_the_moving_submap_in_the_middle_of_the_id_order_and_two_gates(pool):
    """the fit's gates are the moving submap's, the reference's are each submap's own"""
    case = next(c for c in TRACE if c.name == "two submaps with different gates")
    mg, ids, sms = pool.merger(case.subs, case.transforms)
    cands = [case.transforms[1], mc.IDENTITY, mc.about(-1.0, 0.5, 0.5)]
    tf._same(mg.fit(ids[1], cands, 0, 0.1), fr.fit(sms[1], cands, [sms[0], sms[2]], [case.transforms[0], case.transforms[2]], mc.RES, 0, 0.1))
    tf._same(mg.fit(ids[2], cands, 0, 0.1), fr.fit(sms[2], cands, [sms[0], sms[1]], [case.transforms[0], case.transforms[1]], mc.RES, 0, 0.1))
    mg.close()


# ---------------------------------------------------------------- the bound of the fit
def _reference(pool):
    mg, ids, sms = pool.merger(list(mc.REFERENCE[0]) + [mc.ORIGIN_RAY])
    return mg, ids[-1], sms, fr.reference_grid(sms[:-1], mc.REFERENCE[1], mc.RES, 0, 0.1)


def test_a_sensor_cell_at_the_bound_is_accepted_and_counts_nothing(pool):
    mg, moving, sms, grid = _reference(pool)
    assert fr.fit_refused(sms[-1], mc.ACCEPTED, grid, mc.RES) is None
    got = mg.fit(moving, mc.ACCEPTED, 0, 0.1)
    tf._same(got, fr.fit_on(sms[-1], mc.ACCEPTED, grid, mc.RES))
    assert all(int(g[k]) == 0 for g in got for k in fr.FIELDS[:-1]) and (got["score"] == 0.0).all()
    assert mg.fit_stats()["fits"] == 1
    mg.close()


@pytest.mark.parametrize("k", range(len(mc.REFUSED)))
def test_a_metre_beyond_the_bound_is_refused(pool, k):
    mg, moving, sms, grid = _reference(pool)
    ordinary = [mc.IDENTITY, (4.5, 4.25, 0.0)]
    cands = [ordinary[1]] * k + [mc.REFUSED[k], mc.IDENTITY]
    assert fr.fit_refused(sms[-1], cands, grid, mc.RES) == ("pose", k)
    before = mg.fit(moving, ordinary, 0, 0.1)
    st = mg.fit_stats()
    tm._error(lambda: mg.fit(moving, cands, 0, 0.1), capi.KH_ERR_INVALID_ARG)
    text = capi.lib().kh_last_error()
    assert b"kh_merge_fit: correction %d " % k in text and b"2^30" in text, text
    assert mg.fit_stats() == st, "a refused fit counts nothing"
    after = mg.fit(moving, ordinary, 0, 0.1)
    tf._same(after, fr.fit_on(sms[-1], ordinary, grid, mc.RES))
    assert after.tobytes() == before.tobytes() and after[1]["hits_free"] == 1
    mg.close()


def test_a_laser_that_walks_too_far_is_refused(pool):
    mg, ids, sms = pool.merger([mc.TINY, mc.LONG_LASER], resolution=mc.FINE_RES)
    grid = fr.reference_grid(sms[:1], [mc.IDENTITY], mc.FINE_RES, 0, 0.1)
    assert fr.fit_refused(sms[1], [mc.IDENTITY], grid, mc.FINE_RES) == ("laser", -1)
    tm._error(lambda: mg.fit(ids[1], [mc.IDENTITY], 0, 0.1), capi.KH_ERR_INVALID_ARG)
    text = capi.lib().kh_last_error()
    assert b"kh_merge_fit: " in text and b"range_threshold" in text and b"2^20" in text, text
    assert mg.fit_stats()["fits"] == 0
    mg.close()
    # ... and the same laser on 0.25 m cells is an ordinary fit
    mg, ids, rsms = pool.merger(list(mc.REFERENCE[0]) + [mc.LONG_LASER])
    rgrid = fr.reference_grid(rsms[:-1], mc.REFERENCE[1], mc.RES, 0, 0.1)
    cands = [mc.IDENTITY, (5.0, 4.0, 0.3)]
    got = mg.fit(ids[-1], cands, 0, 0.1)
    tf._same(got, fr.fit_on(rsms[-1], cands, rgrid, mc.RES))
    assert got[1]["pass_free"] > 0 and got[1]["hits_unknown"] > 0, "from the middle of the room through its rim"
    mg.close()


# ---------------------------------------------------------------- refusals of set_transform and move_submap
@pytest.mark.parametrize("bad", mc.NOT_FINITE, ids=[repr(t) for t in mc.NOT_FINITE])
def test_a_correction_or_marker_pose_that_is_not_finite_is_refused(pool, bad):
    subs, transforms = [mc.FRAME, mc.TURNED], [mc.IDENTITY, mc.about(0.7, 0.5, -0.25)]
    mg, ids, sms = pool.merger(subs, transforms)
    state = [(mg.transform(i), mg.location(i)) for i in ids]
    tm._error(lambda: mg.set_transform(ids[1], bad), capi.KH_ERR_INVALID_ARG)
    assert b"kh_merge_set_transform" in capi.lib().kh_last_error()
    tm._error(lambda: mg.move_submap(ids[1], bad), capi.KH_ERR_INVALID_ARG)
    assert b"kh_merge_move_submap" in capi.lib().kh_last_error()
    for i, (t, loc) in zip(ids, state):
        assert np.array_equal(bits(mg.transform(i)), bits(t)) and np.array_equal(bits(mg.location(i)), bits(loc))
    got, _ = _merge_is_the_rule(mg, sms, transforms, min_pass=0)
    got.close(); mg.close()


# ---------------------------------------------------------------- one handle, several calls
def test_merge_fit_merge_fit_on_one_handle(pool):
    """merge, a fit with 70 candidates, a merge after set_transform, a fit with one candidate: each is the rule's and a fresh
    merger's -- the growing work buffer and the residency tables carry nothing over"""
    subs = [mc.FRAME, mc.ROOM, mc.TURNED]
    moved = mc.about(-2.0, 0.5, 0.25)
    cands = mc.layout_candidates()
    mg, ids, sms = pool.merger(subs)

    def fresh(transforms):
        other, _, _ = pool.merger(subs, transforms)
        return other

    first, _ = _merge_is_the_rule(mg, sms, [mc.IDENTITY] * 3, min_pass=0)
    other = fresh([mc.IDENTITY] * 3)
    theirs = other.merge(0, 0.1)
    _assert_grid(theirs, _grid_dict(first))
    grid = fr.reference_grid(sms[:2], [mc.IDENTITY] * 2, mc.RES, 0, 0.1)
    many = mg.fit(ids[2], cands, 0, 0.1)
    tf._same(many, fr.fit_on(sms[2], cands, grid, mc.RES))
    assert many.tobytes() == other.fit(ids[2], cands, 0, 0.1).tobytes()
    theirs.close(); other.close()
    mg.set_transform(ids[1], moved)
    second, _ = _merge_is_the_rule(mg, sms, [mc.IDENTITY, moved, mc.IDENTITY], min_pass=0)
    other = fresh([mc.IDENTITY, moved, mc.IDENTITY])
    theirs = other.merge(0, 0.1)
    _assert_grid(theirs, _grid_dict(second))
    grid = fr.reference_grid(sms[:2], [mc.IDENTITY, moved], mc.RES, 0, 0.1)
    one = mg.fit(ids[2], cands[4:5], 0, 0.1)
    tf._same(one, fr.fit_on(sms[2], cands[4:5], grid, mc.RES))
    assert one.tobytes() == other.fit(ids[2], cands[4:5], 0, 0.1).tobytes() and one[0]["known"] > 0
    assert mg.stats()["merges"] == 2 and mg.fit_stats()["fits"] == 2
    for g in (first, second, theirs):
        g.close()
    other.close(); mg.close()
