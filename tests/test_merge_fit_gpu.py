"""GPU: the fit of candidate corrections of one submap against the merge of the others (kh_merge_fit, MapMerger.fit;
k_occ_fit_merged) against tests/merge_fit_rule.py, which ends at the occupancy oracle.  Equality is exact: the six counters, the
three derived integers, and the bits of the score.

The sessions are a few scans each, placed where they were taken (use_scan_matching 0: nothing here is about matching); the scan
counts and lasers are chosen for the kernel's work layout -- one wave per (candidate, scan, run of 64 beams), four waves per
workgroup, a workgroup never across two candidates."""
import math

import numpy as np
import pytest

import merge_fit_rule as fr
import merge_rule as rule
import test_merge_gpu as tm
from common import bits
from slam_toolbox_amd import capi, synth
from slam_toolbox_amd.merge import MapMerger

pytestmark = pytest.mark.gpu
RES = tm.RES
FAR = (1000.0, 1000.0, 0.0)                   # every beam outside the grid
NEAR = (0.4, -0.3, 0.2)
LOW = (-5.0, -4.0, 0.0)                       # towards the grid's low corner: walks that start inside and leave through negative cells
BELOW = (-7.0, -5.5, 0.0)                     # past it: walks that start at negative cells and enter


def _laser(n_beams):
    return synth.Laser(n_beams=n_beams, ang_res=(synth.MAX_ANGLE - synth.MIN_ANGLE) / (n_beams - 1))


LASER_65, LASER_40 = _laser(65), _laser(40)


def _poses(n, column=1, first=0):
    """on the centre line of aisle `column`, 4 m apart, turning by 0.7 rad from scan to scan"""
    return [np.array([2.5 + 4.0 * column + RES / 4, 5.0 + 4.0 * (first + k) + RES / 4, 0.3 + 0.7 * (first + k)]) for k in range(n)]


def _mapper(laser, poses, seed):
    from slam_toolbox_amd.mapper import Mapper
    world, rng = synth.make_world(12345), np.random.default_rng(seed)
    m = Mapper(laser, max_candidates=1, use_scan_matching=0, do_loop_closing=0)
    for k, pose in enumerate(poses):
        assert not synth.inside_obstacle(world, pose[0], pose[1], margin=0.2)
        assert m.Process(synth.make_scan(world, pose, rng, laser), pose, float(k))[0]
    assert len(m.alive()) == len(poses)
    return m


def _same(got, want):
    """MapMerger.fit's structured array against the rule's list of dicts"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        have = [int(g[name]) for name in fr.FIELDS[:-1]]
        assert np.array_equal(have, [w[name] for name in fr.FIELDS[:-1]]), (k, dict(zip(fr.FIELDS, have)), w)
        assert bits([g["score"]])[0] == bits([w["score"]])[0], (k, g["score"], w["score"])


def _reference(tmp_path, n_scans=6):
    laser = synth.Laser()
    a = _mapper(laser, _poses(n_scans), 31)
    return a, tm._submap_of(a, laser, tmp_path, "a")


@pytest.mark.parametrize("n_scans", [1, 3])
def test_scan_counts_whose_waves_do_not_fill_a_workgroup(kartohip_lib, tmp_path, n_scans):
    """1081 beams are 17 runs: 17 and 51 waves per candidate, so the last workgroup of a candidate is part empty -- it would hold the
    next candidate's first waves if workgroups were dealt across candidates.  1, 2 and 5 candidates in one call; the all-outside one
    in the middle puts zeros between non-zeros."""
    laser = synth.Laser()
    assert (n_scans * ((laser.n_beams + 63) // 64)) % 4 != 0
    a, sa = _reference(tmp_path)
    b = _mapper(laser, _poses(n_scans, first=1), 32)
    sb = tm._submap_of(b, laser, tmp_path, "b")
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    for cands in ([rule.IDENTITY], [tm.T1, NEAR], [rule.IDENTITY, NEAR, FAR, tm.T1, LOW]):
        got, want = mg.fit(ib, cands), fr.fit(sb, cands, [sa], [rule.IDENTITY], RES)
        _same(got, want)
        assert got[0]["known"] > 0 and got[-1]["known"] > 0
    assert all(int(got[2][name]) == 0 for name in fr.FIELDS[:-1]) and got[2]["score"] == 0.0
    assert got[0]["hits_occupied"] > 0 and got[0]["score"] > got[3]["score"]
    st = mg.fit_stats()
    assert st["fits"] == 3 and st["candidates_total"] == 8 and st["beam_candidates"] == 5 * n_scans * laser.n_beams and st["kernel_us"] > 0
    print(f"{n_scans} scan(s), 5 candidates: {st['kernel_us']} us, scores {[float(g['score']) for g in got]}")
    mg.close(); a.close(); b.close()


@pytest.mark.parametrize("laser", [LASER_65, LASER_40], ids=["65_beams", "40_beams"])
def test_partial_and_empty_runs(kartohip_lib, tmp_path, laser):
    """65 beams: a full run and a run of one beam; 40 beams: one partial run.  Three scans: 6 and 3 waves per candidate."""
    a, sa = _reference(tmp_path)
    b = _mapper(laser, _poses(3, first=1), 33)
    sb = tm._submap_of(b, laser, tmp_path, "b")
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    cands = [NEAR, FAR, rule.IDENTITY]
    got = mg.fit(ib, cands)
    _same(got, fr.fit(sb, cands, [sa], [rule.IDENTITY], RES))
    assert got[0]["known"] > 0 and got[1]["known"] == 0 and got[2]["hits_occupied"] > 0
    mg.close(); a.close(); b.close()


def test_negative_cell_indices_on_part_of_the_walk(kartohip_lib, tmp_path):
    a, sa = _reference(tmp_path)
    laser = synth.Laser()
    b = _mapper(laser, _poses(2), 34)
    sb = tm._submap_of(b, laser, tmp_path, "b")
    grid = fr.reference_grid([sa], [rule.IDENTITY], RES)
    # what the case is about: under LOW some sensor cells are inside the grid and many beam ends have negative cells
    sensors = np.array([rule.transformed_scan(LOW, s)["sensor"][:2] for s in sb["scans"]])
    ends = np.concatenate([rule.transform_points(LOW, s["points"])[np.isfinite(s["ranges"]) & (s["ranges"] < laser.range_threshold)]
                           for s in sb["scans"]])
    assert ((sensors - grid["offset"]) / RES > 1).all() and (((ends - grid["offset"]) / RES) < -1).any(axis=1).sum() > 100
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    below = np.array([rule.transformed_scan(BELOW, s)["sensor"][:2] for s in sb["scans"]])
    assert ((below - grid["offset"]) / RES < -1).any(axis=1).all()                 # every sensor cell has a negative index
    got = mg.fit(ib, [LOW, BELOW])
    _same(got, fr.fit_on(sb, [LOW, BELOW], grid, RES))
    assert got[0]["known"] > 0 and got[1]["known"] > 0
    mg.close(); a.close(); b.close()


def test_two_other_submaps_with_different_lasers_and_another_update_rule(kartohip_lib, tmp_path):
    a, sa = _reference(tmp_path, 4)
    c = _mapper(tm.SMALL_LASER, _poses(4, column=2), 35)
    sc = tm._submap_of(c, tm.SMALL_LASER, tmp_path, "c")
    laser = synth.Laser()
    b = _mapper(laser, _poses(3, first=1), 36)
    sb = tm._submap_of(b, laser, tmp_path, "b")
    mg = MapMerger(RES)
    ia, ib, ic = mg.add_submap(a), mg.add_submap(b), mg.add_submap(c)         # the moving submap in the middle of the id order
    mg.set_transform(ic, NEAR)
    mg.set_transform(ib, tm.T2)                                               # its own correction plays no part in a fit
    cands = [rule.IDENTITY, (4.0, 0.0, 0.0), tm.T1]
    _same(mg.fit(ib, cands), fr.fit(sb, cands, [sa, sc], [rule.IDENTITY, NEAR], RES))
    _same(mg.fit(ib, cands, min_pass_through=0, occupancy_threshold=0.3), fr.fit(sb, cands, [sa, sc], [rule.IDENTITY, NEAR], RES, 0, 0.3))
    # ... and the short laser as the moving one, against the two long ones
    _same(mg.fit(ic, cands), fr.fit(sc, cands, [sa, sb], [rule.IDENTITY, tm.T2], RES))
    mg.close(); a.close(); b.close(); c.close()


def test_a_fit_changes_nothing(kartohip_lib, tmp_path):
    """the same call twice gives the same answer; the corrections, the locations and a following merge are what they were"""
    a, _ = _reference(tmp_path)
    b = _mapper(synth.Laser(), _poses(3, first=1), 37)
    mg = MapMerger(RES)
    ia, ib = mg.add_submap(a), mg.add_submap(b)
    mg.set_transform(ib, NEAR)
    before = mg.merge()
    state = [(mg.transform(i), mg.location(i)) for i in (ia, ib)]
    cands = [rule.IDENTITY, FAR, tm.T1, NEAR]
    first, second = mg.fit(ib, cands), mg.fit(ib, cands)
    assert first.tobytes() == second.tobytes() and first[3]["known"] > 0
    for i, (t, loc) in zip((ia, ib), state):
        assert np.array_equal(bits(mg.transform(i)), bits(t)) and np.array_equal(bits(mg.location(i)), bits(loc))
    after = mg.merge()
    tm._assert_same_grid(after, before)
    assert mg.stats()["merges"] == 2                      # the fit's reference grids are not merges
    before.close(); after.close(); mg.close(); a.close(); b.close()


def test_errors_leave_the_merger_usable(kartohip_lib, tmp_path):
    from slam_toolbox_amd.mapper import Mapper
    a, sa = _reference(tmp_path, 2)
    mg = MapMerger(RES)
    ia = mg.add_submap(a)
    tm._error(lambda: mg.fit(ia, [rule.IDENTITY]), capi.KH_ERR_INVALID_ARG)           # no other submap
    empty = Mapper(synth.Laser())
    ie = mg.add_submap(empty)
    tm._error(lambda: mg.fit(ia, [rule.IDENTITY]), capi.KH_ERR_INVALID_ARG)           # no scan in any other submap
    tm._error(lambda: mg.fit(99, [rule.IDENTITY]), capi.KH_ERR_NOT_FOUND)
    tm._error(lambda: mg.fit(ia, [(0.0, float("nan"), 0.0)]), capi.KH_ERR_INVALID_ARG)
    assert mg.fit_stats()["fits"] == 0
    # a submap without scans fits nothing, anywhere
    got = mg.fit(ie, [rule.IDENTITY, NEAR])
    assert all(int(g[name]) == 0 for g in got for name in fr.FIELDS[:-1]) and (got["score"] == 0.0).all()
    assert mg.fit_stats()["fits"] == 1
    g = mg.merge()
    tm._assert_is(g, rule.merged_grid([sa], [rule.IDENTITY], RES))
    g.close(); mg.close(); a.close(); empty.close()
