"""GPU: mapping sessions -- kh_mapper_save / kh_mapper_load (a resumed run is the same run), the three start modes behind a
load, and kh_mapper_build_map (the occupancy map traced from the mapper's resident scans).

Yardsticks: the two queues tests/test_localization_gpu.py pins to the unmodified reference mapper (its `_reference` /
`_compare` are used as they stand: the log of part one followed by the log of part two must be line-identical to the
REFERENCE's log of the uninterrupted queue, the final poses bit-equal), and, for the map, the existing host-packed path
(kh_occupancy_compute_dimensions + _create + _add_scans + _update fed from kh_mapper_get_scan) that tests/test_occupancy_gpu.py
pins to the reference."""
import ctypes as C
import os

import numpy as np
import pytest

import test_localization_gpu as loc
from common import bits
from slam_toolbox_amd import capi, session, synth
from slam_toolbox_amd.occupancy_grid import OccupancyGrid

pytestmark = pytest.mark.gpu
N_QUEUE, LOOP_DIST, SWITCH, BUFFER = loc.N_QUEUE, loc.LOOP_DIST, loc.SWITCH, loc.BUFFER
_ref_cache = {}


def _mapper(log_path=None, **kw):
    from slam_toolbox_amd.mapper import Mapper
    return Mapper(synth.Laser(), loop_search_maximum_distance=LOOP_DIST, log_path=log_path, **kw)


def _solver_state(m):
    """solver nodes and constraints in insertion order, through the existing getters"""
    L = capi.lib()
    s = L.kh_mapper_solver(m._h)
    n, nc = L.kh_spa_num_nodes(s), L.kh_spa_num_constraints(s)
    ids, poses = np.zeros(max(n, 1), dtype=np.int32), np.zeros(3 * max(n, 1))
    capi.check(L.kh_spa_get_nodes(s, ids.ctypes.data, poses.ctypes.data), "kh_spa_get_nodes")
    a, b, z, info = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32), np.zeros((nc, 3)), np.zeros((nc, 6))
    for k in range(nc):
        ia, ib, zk, ik = C.c_int32(), C.c_int32(), np.zeros(3), np.zeros(6)
        capi.check(L.kh_spa_get_constraint(s, k, C.byref(ia), C.byref(ib), zk, ik), "kh_spa_get_constraint")
        a[k], b[k], z[k], info[k] = ia.value, ib.value, zk, ik
    return ids[:n], poses[:3 * n].reshape(n, 3), a, b, z, info


def _scan_state(m, i):
    s, b = m.scan(int(i))
    n = s.n
    return (np.ctypeslib.as_array(s.ranges, (n,)).copy(), np.ctypeslib.as_array(s.points_xy, (2 * n,)).copy(), np.array(s.sensor_pose[:]),
            np.array(b.barycenter[:]), np.array(b.bbox_size[:]), b.n_edges, b.score, b.n_points,
            np.ctypeslib.as_array(b.points_xy, (2 * b.n_points,)).copy() if b.n_points else np.zeros(0))


def _assert_same_mapper(a, b):
    assert a.num_scans() == b.num_scans() and a.num_edges() == b.num_edges()
    assert np.array_equal(a.alive(), b.alive()) and np.array_equal(a.localization_buffer(), b.localization_buffer())
    assert np.array_equal(bits(a.poses()), bits(b.poses()))                    # (NaN rows of removed scans compare as bits)
    for i in a.alive():
        assert np.array_equal(a.adjacency(i), b.adjacency(i)), i
        for x, y in zip(_scan_state(a, i), _scan_state(b, i)):
            assert np.array_equal(bits(np.asarray(x, dtype=np.float64)), bits(np.asarray(y, dtype=np.float64))), i
    for x, y in zip(_solver_state(a), _solver_state(b)):
        assert x.shape == y.shape and np.array_equal(bits(x.astype(np.float64)), bits(y.astype(np.float64)))


def test_round_trip_is_exact(kartohip_lib, tmp_path):
    """the lap map part-way (250 queue scans of mapping: one closed lap; then localization until the buffer is full and scans have
    been evicted): save, load, save again -- the two files are byte-identical and every getter answers the same bits"""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = loc._queue()
    m = _mapper()
    for i in range(SWITCH):
        m.Process(ranges[i], odom[i], 0.1 * i)
    i = SWITCH
    while m.stats()["nodes_removed"] < 3:
        m.ProcessLocalization(ranges[i], odom[i], 0.1 * i)
        i += 1
    m.RemoveNode(40)
    assert m.stats()["loop_closures"] >= 1 and len(m.localization_buffer()) == BUFFER
    f1, f2 = str(tmp_path / "one.khms"), str(tmp_path / "two.khms")
    m.save(f1)
    info = session.info(f1)
    assert info["n_scan_slots"] == m.num_scans() and info["n_alive"] == len(m.alive()) and info["n_edges"] == m.num_edges()
    assert info["n_localization_buffer"] == BUFFER and info["n_beams"] == synth.N_BEAMS and info["file_bytes"] == os.path.getsize(f1)
    m2 = Mapper.load(f1)
    m2.save(f2)
    with open(f1, "rb") as a, open(f2, "rb") as b:
        assert a.read() == b.read(), "save -> load -> save changed the file"
    _assert_same_mapper(m, m2)
    parsed = session.read(f1)
    assert np.array_equal(parsed["ids"], m.alive()) and np.array_equal(bits(parsed["corrected"]), bits(m.poses()[m.alive()]))
    print(f"round trip: {info['n_alive']} scans alive of {info['n_scan_slots']}, {info['n_solver_constraints']} constraints, "
          f"{info['n_supernodes']} cached supernodes, {info['file_bytes']} bytes")
    m.close(); m2.close()


# ---- a resumed run is the same run, judged against the reference ------------------------------------------------------------
def _reference_of(queue, tmp_path_factory):
    if queue not in _ref_cache:
        _, odom = loc._queue()
        accepted_at = loc._accepted_queue_indices(odom)
        n_map = 0 if queue == "pure" else sum(1 for a in accepted_at if a < SWITCH)
        schedule = loc._ring_schedule(accepted_at, n_map)
        ref, ref_log = loc._reference(tmp_path_factory.mktemp("ref_" + queue), schedule)
        _ref_cache[queue] = (ref, ref_log, n_map)
    return _ref_cache[queue]


# when to interrupt: (name, predicate over (queue index just processed, stats, mapper) -> cut behind this scan)
def _cut_rules(queue):
    if queue == "pure":
        # no closure can happen in this queue (ten scans alive): the three cuts are before the buffer is full, with the buffer
        # full and the first scans evicted, and deep into the run
        return {"buffer_filling": lambda i, st, m: len(m.localization_buffer()) == BUFFER // 2,
                "buffer_full_nodes_removed": lambda i, st, m: st["nodes_removed"] >= 3,
                "late": lambda i, st, m: i == 400}
    return {"before_first_closure": lambda i, st, m: i == 100,
            "right_after_correct_poses": lambda i, st, m: st["loop_closures"] >= 1,
            "localization_buffer_full_nodes_removed": lambda i, st, m: i >= SWITCH and st["nodes_removed"] >= 5}


@loc.needs_ref
@pytest.mark.parametrize("queue,cut", [(q, c) for q in ("pure", "map_then_localize") for c in _cut_rules(q)])
def test_resumed_run_equals_the_reference(kartohip_lib, tmp_path, tmp_path_factory, queue, cut):
    """save -> destroy -> load in the middle of the queue; log of part one + log of part two against the reference's log of the
    uninterrupted queue, final poses against its poses"""
    from slam_toolbox_amd.mapper import Mapper
    ref, ref_log, n_map = _reference_of(queue, tmp_path_factory)
    ranges, odom = loc._queue()
    rule = _cut_rules(queue)[cut]
    log1, log2, path = str(tmp_path / "one.log"), str(tmp_path / "two.log"), str(tmp_path / "cut.khms")

    def step(m, i):
        if queue == "pure" or i >= SWITCH:
            return m.ProcessLocalization(ranges[i], odom[i], 0.1 * i)[0]
        return m.Process(ranges[i], odom[i], 0.1 * i)[0]

    m = _mapper(log1)
    accepted, cut_at = 0, None
    for i in range(N_QUEUE):
        accepted += int(step(m, i))
        if rule(i, m.stats(), m):
            cut_at = i + 1
            break
    assert cut_at is not None and cut_at < N_QUEUE, "the cut rule never fired"
    st = m.stats()
    if cut == "before_first_closure":
        assert st["loop_closures"] == 0
    if cut == "right_after_correct_poses":
        m.set_log(None)
        assert loc._lines(log1)[-1] == "K", "the cut is not right behind a CorrectPoses"
    if "nodes_removed" in cut:
        assert st["nodes_removed"] >= 3 and len(m.localization_buffer()) == BUFFER
    m.save(path)
    m.set_log(None)
    m.close()
    del m
    m = Mapper.load(path, log_path=log2)
    for i in range(cut_at, N_QUEUE):
        accepted += int(step(m, i))
    alive = m.alive()
    poses = m.poses()[alive]
    m.set_log(None)
    hip_log = loc._lines(log1) + loc._lines(log2)
    print(f"{queue} / {cut}: cut behind queue scan {cut_at - 1}, {os.path.getsize(path)} bytes, {st['loop_closures']} closures and "
          f"{st['nodes_removed']} removals before it, {m.stats()['loop_closures']} closures after it")
    m.close()
    loc._compare(ref, ref_log, hip_log, accepted, alive, poses)


def test_resumed_lifelong_run_on_two_members(kartohip_lib, tmp_path):
    """A mapping queue with the node-decay policy on, interrupted after nodes have been removed, and loaded through a device list
    of two entries (two members on the one GPU, as tests/test_group_gpu.py does).  The reference's lifelong node cannot be built
    without rclcpp (tests/test_lifelong_policy_gpu.py), so the yardstick here is the uninterrupted run of the one-member mapper,
    whose policy that test pins to oracle/lifelong.py."""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = loc._queue()
    whole = _mapper(str(tmp_path / "whole.log"))
    whole.SetLifelong(True)
    for i in range(N_QUEUE):
        whole.Process(ranges[i], odom[i], 0.1 * i)
    whole.set_log(None)
    assert whole.stats()["nodes_removed"] >= 1 and whole.stats()["loop_closures"] >= 1
    m = _mapper(str(tmp_path / "one.log"))
    m.SetLifelong(True)
    cut_at = None
    for i in range(N_QUEUE):
        m.Process(ranges[i], odom[i], 0.1 * i)
        if m.stats()["nodes_removed"] >= 2 and m.stats()["loop_closures"] >= 1:
            cut_at = i + 1
            break
    assert cut_at is not None and cut_at < N_QUEUE - 50, "cut too late to show anything"
    path = str(tmp_path / "lifelong.khms")
    m.save(path)
    assert session.info(path)["lifelong"] == 1
    m.set_log(None)
    m.close()
    m = Mapper.load(path, devices=[0, 0], log_path=str(tmp_path / "two.log"))
    for i in range(cut_at, N_QUEUE):
        m.Process(ranges[i], odom[i], 0.1 * i)
    m.set_log(None)
    assert loc._lines(str(tmp_path / "one.log")) + loc._lines(str(tmp_path / "two.log")) == loc._lines(str(tmp_path / "whole.log"))
    assert np.array_equal(m.alive(), whole.alive()) and np.array_equal(bits(m.poses()), bits(whole.poses()))
    for i in m.alive():
        assert m.scan(int(i))[1].score == whole.scan(int(i))[1].score
    print(f"lifelong: cut behind queue scan {cut_at - 1}, {whole.stats()['nodes_removed']} nodes removed in all")
    m.close(); whole.close()


# ---- start modes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["given_pose", "first_node", "localize_at_pose"])
def test_start_modes(kartohip_lib, tmp_path, start):
    """After a load, the FIRST scan goes through the entry the start mode names, the second through the plain one: same log
    lines, pose and covariance as calling that entry by hand on a never-saved twin"""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = loc._queue()
    twin, queue_index = loc._build_map(str(tmp_path / "twin.log"))
    saved, _ = loc._build_map()
    path = str(tmp_path / "map.khms")
    saved.save(path)
    saved.close()
    map_poses = twin.poses()
    pose = map_poses[100].copy()
    pose[:2] += np.array([0.12, -0.08])
    scan = ranges[queue_index[100]]
    m = Mapper.load(path, start=start, pose=None if start == "first_node" else pose, log_path=str(tmp_path / "loaded.log"))
    assert np.array_equal(bits(m.poses()), bits(map_poses))
    twin.set_log(str(tmp_path / "twin.1")); m.set_log(str(tmp_path / "loaded.1"))
    localization = start == "localize_at_pose"
    dock_pose = map_poses[0] + np.array([0.1, -0.05, 0.02])
    if start == "first_node":
        got = m.Process(ranges[queue_index[0]], dock_pose, 100.0)
        want = twin.ProcessAgainstNode(ranges[queue_index[0]], dock_pose, 0, 100.0)
    else:
        got = (m.ProcessLocalization if localization else m.Process)(scan, odom[SWITCH], 100.0)      # the scan's own odometry is replaced
        want = twin.ProcessAgainstNodesNearBy(scan, pose, 100.0, add_to_localization_buffer=localization)
    assert got[0] and want[0]
    assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2]))
    # the second scan: the plain entry on both (the start mode is spent)
    nxt = got[1] + np.array([0.6 * np.cos(got[1][2]), 0.6 * np.sin(got[1][2]), 0.0])
    got2 = (m.ProcessLocalization if localization else m.Process)(scan, nxt, 100.1)
    want2 = (twin.ProcessLocalization if localization else twin.Process)(scan, nxt, 100.1)
    assert got2[0] and want2[0] and np.array_equal(bits(got2[1]), bits(want2[1])) and np.array_equal(bits(got2[2]), bits(want2[2]))
    twin.set_log(None); m.set_log(None)
    a, b = loc._lines(str(tmp_path / "twin.1")), loc._lines(str(tmp_path / "loaded.1"))
    assert a == b and sum(l.startswith("N ") for l in a) == 2
    assert np.array_equal(m.localization_buffer(), twin.localization_buffer())
    assert len(m.localization_buffer()) == (2 if localization else 0)
    assert np.array_equal(bits(m.poses()), bits(twin.poses()))
    m.close(); twin.close()


# ---- the map ----------------------------------------------------------------------------------------------------------------
def _yardstick_map(m, resolution):
    """the existing path: every scan pulled to the host with kh_mapper_get_scan, packed and sent back"""
    L, laser = capi.lib(), synth.Laser()
    ids = m.alive()
    scans = (capi.KhScan * len(ids))(*[m.scan(int(i))[0] for i in ids])
    w, h, off = C.c_int32(), C.c_int32(), np.zeros(2)
    capi.check(L.kh_occupancy_compute_dimensions(len(ids), scans, laser.min_range, laser.range_threshold, resolution, C.byref(w), C.byref(h), off),
               "kh_occupancy_compute_dimensions")
    g = OccupancyGrid(w.value, h.value, off, resolution)
    capi.check(L.kh_occupancy_add_scans(g._h, len(ids), scans, laser.range_threshold, laser.min_range, laser.max_range), "kh_occupancy_add_scans")
    g.Update(2, 0.1)
    return g


def _assert_same_map(got, want):
    assert (got.width, got.height, got.width_step) == (want.width, want.height, want.width_step)
    assert np.array_equal(bits(got.offset), bits(want.offset))
    assert np.array_equal(got.cells(), want.cells())
    for x, y in zip(got.counters(), want.counters()):
        assert np.array_equal(x, y)
    assert got.stats()["beams"] == want.stats()["beams"]
    hist = np.bincount(got.cells().reshape(-1), minlength=256)
    assert hist[100] > 0 and hist[255] > 0, "an empty map shows nothing"


def test_build_map_of_a_loaded_session(kartohip_lib, tmp_path):
    """the lap queue (450 of its 500 scans, then the rest), saved and loaded: build_map against the host-packed path; again after
    5 more accepted scans, with the upload counters showing that only new / re-posed scans moved"""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = loc._queue()
    m = _mapper()
    for i in range(450):
        m.Process(ranges[i], odom[i], 0.1 * i)
    path = str(tmp_path / "laps.khms")
    m.save(path)
    m.close()
    m = Mapper.load(path)
    n_alive = len(m.alive())
    for resolution in (0.05, 0.1):
        got, want = m.build_map(resolution), _yardstick_map(m, resolution)
        _assert_same_map(got, want)
        got.close(); want.close()
    st = m.map_stats()
    # (device copies are lazy after a load: the first build uploads every scan once, the second nothing)
    assert st["calls"] == 2 and st["scans_traced"] == n_alive
    assert st["point_uploads_total"] == n_alive and st["range_uploads_total"] == n_alive and st["point_uploads"] == 0 and st["range_uploads"] == 0
    before = m.poses()
    i, more = 450, 0
    while more < 5:
        more += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
        i += 1
    after = m.poses()
    moved = int(np.any(bits(after[:len(before)]) != bits(before), axis=1).sum())
    got, want = m.build_map(0.05), _yardstick_map(m, 0.05)
    _assert_same_map(got, want)
    st = m.map_stats()
    print(f"build_map: {n_alive} scans at first, then {st['scans_traced']}; rebuild uploaded {st['point_uploads']} point sets and "
          f"{st['range_uploads']} range sets ({moved} old scans re-posed); trace {got.stats()['trace_ms']:.3f} ms resident, "
          f"{want.stats()['trace_ms']:.3f} ms packed")
    assert st["scans_traced"] == n_alive + 5 and st["range_uploads"] == 5
    # the matcher has already made some of the new / re-posed scans resident for its own use: at most all of them are left
    assert st["point_uploads"] <= 5 + moved
    got.close(); want.close(); m.close()


def test_build_map_after_removals(kartohip_lib):
    """removed nodes leave the map: build, remove a fifth of the nodes outside the running window, build again"""
    m, _ = loc._build_map()
    first, want = m.build_map(0.05), _yardstick_map(m, 0.05)
    _assert_same_map(first, want)
    want.close()
    n = m.num_scans()
    for i in range(5, n - 2 * BUFFER, 5):
        m.RemoveNode(i)
    got, want = m.build_map(0.05), _yardstick_map(m, 0.05)
    _assert_same_map(got, want)
    assert m.map_stats()["scans_traced"] == len(m.alive()) < n and m.map_stats()["point_uploads"] == 0 and m.map_stats()["range_uploads"] == 0
    assert not np.array_equal(got.counters()[0], first.counters()[0]) or (got.width, got.height) != (first.width, first.height)
    first.close(); got.close(); want.close(); m.close()
