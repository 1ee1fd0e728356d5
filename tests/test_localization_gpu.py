"""GPU: localization mode of the mapper front end (kh_mapper_process_localization, _against_nodes_near_by, _against_node,
_clear_localization_buffer) and the near-by queries of the graph store behind it (kh_graph_find_near_by_scan / _vertices).

The reference mapper is reached through what the neighbouring tests use: oracle/_ref/libkarto_ref_slam.so driven by
tests/ref_slam_runner.py in a child process, with its removal schedule.  That driver calls Mapper::Process and removes the
scheduled nodes after a scan with RemoveNodeFromGraph + RemoveScan; Mapper::ProcessLocalization (Mapper.cpp:2831-2909) is
Process followed by exactly that eviction (AddScanToLocalizationBuffer, :2911-2937), so a ring-buffer schedule makes the
unmodified reference mapper perform a localization run.  The driver's scan_buffer_size is 10, so the tests use 10."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import near_by_rule
from common import bits
from slam_toolbox_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libkarto_ref_slam.so")
needs_ref = pytest.mark.skipif(not os.path.exists(LIB), reason="oracle/_ref/libkarto_ref_slam.so not built (needs the reference tree)")
BUFFER = 10            # scan_buffer_size of the reference driver (configure_offline) and of kh_mapper_params_default
N_QUEUE, LOOP_DIST, KIND, SWITCH = 500, 3.0, "laps", 250
_cache = {}


def _queue(n_scans=N_QUEUE, kind=KIND):
    if (n_scans, kind) not in _cache:
        world = synth.make_world(12345)
        truth, odom = synth.trajectory_laps(n_scans) if kind == "laps" else synth.trajectory(n_scans)
        rng = np.random.default_rng(4)
        ranges = np.ascontiguousarray(np.stack([synth.make_scan(world, truth[i], rng) for i in range(n_scans)]))
        _cache[(n_scans, kind)] = (ranges, np.ascontiguousarray(odom))
    return _cache[(n_scans, kind)]


def _lines(path):
    with open(path) as f:
        return [" ".join(l.split()[:2]) if l.startswith("X ") else l.rstrip("\n") for l in f if not l.startswith("Z ")]


def _normalize_angle(a):
    while a < -math.pi:
        a += 2.0 * math.pi
    while a > math.pi:
        a -= 2.0 * math.pi
    return a


def _accepted_queue_indices(odom, travel=0.5, heading=0.5):
    """Mapper::HasMovedEnough (Mapper.cpp:3110-3142) on the odometric poses alone (laser at the robot's centre, all time stamps
    inside minimum_time_interval): which scans of the queue a mapper accepts does not depend on any match."""
    out, last = [], None
    for i, p in enumerate(odom):
        if last is not None:
            dx, dy = last[0] - p[0], last[1] - p[1]
            if not (abs(_normalize_angle(p[2] - last[2])) >= heading or dx * dx + dy * dy >= travel * travel - 1e-06):
                continue
        out.append(i)
        last = p
    return out


def _ring_schedule(accepted_at, first_buffered):
    """The rule of AddScanToLocalizationBuffer: scan ids are the accepted scans' ordinals; the scan accepted as number j evicts
    number j - BUFFER once that one is a buffered scan (id >= first_buffered), at the queue index where j was accepted."""
    return [(at, j - BUFFER) for j, at in enumerate(accepted_at) if j - BUFFER >= first_buffered]


def _reference(tmp_path, schedule):
    prefix = str(tmp_path / "ref")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_slam_runner.py"), LIB, str(N_QUEUE), str(LOOP_DIST), prefix, KIND,
                    ",".join(f"{a}:{i}" for a, i in schedule)], check=True, timeout=900)
    ref_log = _lines(prefix + ".log")
    assert not any(l.startswith("!") for l in ref_log), [l for l in ref_log if l.startswith("!")]
    return np.load(prefix + ".npz"), ref_log


def _compare(ref, ref_log, hip_log, accepted, alive, poses):
    # (with a removal schedule the driver returns the scans still in its map; the accepted scans are its AddNode calls)
    assert int(ref["accepted"]) == len(alive) and sum(l.startswith("N ") for l in ref_log) == accepted
    for k, (a, b) in enumerate(zip(ref_log, hip_log)):
        assert a == b, f"solver-call logs diverge at line {k}:\n  reference: {a}\n  mapper   : {b}"
    assert len(ref_log) == len(hip_log)
    assert np.array_equal(ref["poses"][:, 0].astype(np.int32), alive)
    assert np.array_equal(ref["poses"][:, 1:], poses), "final corrected poses differ"


@needs_ref
def test_pure_localization_equals_the_reference(kartohip_lib, tmp_path):
    """Every scan of the 500-scan lap queue through ProcessLocalization; the reference mapper with the ring-buffer schedule.
    Closures are not required: with ten scans alive and loop_match_minimum_chain_size 10 a rolling buffer alone has nothing to
    close against."""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = _queue()
    accepted_at = _accepted_queue_indices(odom)
    schedule = _ring_schedule(accepted_at, 0)
    ref, ref_log = _reference(tmp_path, schedule)
    log = str(tmp_path / "hip.log")
    m = Mapper(synth.Laser(), loop_search_maximum_distance=LOOP_DIST, log_path=log)
    accepted = 0
    for i in range(N_QUEUE):
        ok = m.ProcessLocalization(ranges[i], odom[i], 0.1 * i)[0]
        assert ok == (i in accepted_at)
        accepted += int(ok)
        assert len(m.alive()) == min(accepted, BUFFER)
        assert np.array_equal(m.localization_buffer(), m.alive())
    alive, st = m.alive(), m.stats()
    poses = m.poses()[alive]
    m.set_log(None)
    hip_log = _lines(log)
    m.close()
    print(f"pure localization: accepted {accepted}, {st['nodes_removed']} evicted, {st['loop_closures']} closures, "
          f"Process total {st['process_ms']:.0f} ms")
    assert accepted > 4 * BUFFER
    assert sum(l.startswith("D ") for l in hip_log) == accepted - BUFFER == len(schedule) == st["nodes_removed"]
    _compare(ref, ref_log, hip_log, accepted, alive, poses)


@needs_ref
def test_map_then_localize_equals_the_reference(kartohip_lib, tmp_path):
    """kh_mapper_process for the first 250 queue scans (1.6 laps of the 152-scan circuit: the first lap is closed by then),
    ProcessLocalization for the rest; only scans of the second part are evicted, the map is permanent, and the later laps
    close loops against it."""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = _queue()
    accepted_at = _accepted_queue_indices(odom)
    n_map = sum(1 for a in accepted_at if a < SWITCH)            # ids below n_map are the map
    schedule = _ring_schedule(accepted_at, n_map)
    assert schedule and min(i for _, i in schedule) == n_map and min(a for a, _ in schedule) >= SWITCH
    ref, ref_log = _reference(tmp_path, schedule)
    log = str(tmp_path / "hip.log")
    m = Mapper(synth.Laser(), loop_search_maximum_distance=LOOP_DIST, log_path=log)
    accepted = 0
    for i in range(SWITCH):
        accepted += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
    assert accepted == n_map == m.num_scans() and len(m.localization_buffer()) == 0
    closures_before = m.stats()["loop_closures"]
    assert closures_before >= 1, "the first lap is still open at the switch"
    for i in range(SWITCH, N_QUEUE):
        ok = m.ProcessLocalization(ranges[i], odom[i], 0.1 * i)[0]
        accepted += int(ok)
        assert len(m.alive()) == n_map + min(accepted - n_map, BUFFER)
    alive, st = m.alive(), m.stats()
    poses = m.poses()[alive]
    m.set_log(None)
    hip_log = _lines(log)
    m.close()
    print(f"map then localize: map {n_map} scans, accepted {accepted}, {st['nodes_removed']} evicted, {closures_before} closures before "
          f"the switch, {st['loop_closures'] - closures_before} after")
    assert st["loop_closures"] - closures_before >= 1, "no closure against the permanent map after the switch"
    first_loc = next(k for k, l in enumerate(hip_log) if l.startswith(f"N {n_map} "))
    assert sum(l.startswith("X ") for l in hip_log[first_loc:]) >= 1
    assert np.array_equal(alive[:n_map], np.arange(n_map)) and len(alive) == n_map + BUFFER
    assert sum(l.startswith("D ") for l in hip_log) == accepted - n_map - BUFFER == len(schedule)
    _compare(ref, ref_log, hip_log, accepted, alive, poses)


def _build_map(log_path=None):
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = _queue()
    m = Mapper(synth.Laser(), loop_search_maximum_distance=LOOP_DIST, log_path=log_path)
    queue_index = [i for i in range(SWITCH) if m.Process(ranges[i], odom[i], 0.1 * i)[0]]
    return m, queue_index


def _standalone_match(ranges, pose, base_scan):
    """kh_matcher_match of the scan at `pose` against ONE base scan with the mapper's sequential matcher parameters
    (Mapper::Initialize, Mapper.cpp:2606-2631); the query's readings come from a mapper of its own that takes the scan as its
    first one (no match, LocalizedRangeScan::Update at the given pose)."""
    from slam_toolbox_amd.mapper import Mapper
    L = capi.lib()
    p = capi.KhMapperParams()
    L.kh_mapper_params_default(C.byref(p))
    holder = Mapper(synth.Laser())
    assert holder.Process(ranges, pose, 0.0)[0]
    query = holder.scan(0)[0]
    h = C.c_void_p()
    capi.check(L.kh_matcher_create(p.correlation_search_space_dimension, p.correlation_search_space_resolution,
                                   p.correlation_search_space_smear_deviation, synth.Laser().range_threshold, 0, 1, C.byref(h)),
               "kh_matcher_create")
    capi.check(L.kh_matcher_set_params(h, C.byref(p.match)), "kh_matcher_set_params")
    mean, cov, resp = np.zeros(3), np.zeros(9), C.c_double(0.0)
    base = (capi.KhScan * 1)(base_scan)
    capi.check(L.kh_matcher_match(h, C.byref(query), base, 1, 1, 1, mean, cov, C.byref(resp)), "kh_matcher_match")
    L.kh_matcher_destroy(h)
    holder.close()
    return mean, cov.reshape(3, 3)


def test_near_by_entry_points(kartohip_lib, tmp_path):
    """ProcessAgainstNodesNearBy picks the node the numpy rule picks; its result equals ProcessAgainstNode with that id on an
    identically built mapper and a stand-alone match against that node's scan alone; the next scan's odometry is measured from
    the corrected pose (Mapper.cpp:2792, 3065).

    The links: MapperGraph::AddEdges links the new scan to the scan with state id - 1 FIRST, whichever entry point ran
    (Mapper.cpp:1441-1449: previousScanNum = GetStateId() - 1), and then, through LinkChainToScan over the re-seeded running
    scans, to the node.  So `C <node> <new>` is the first link out of the running scans and the second link of the log, behind
    `C <new - 1> <new>`; it is literally the first line where the node is the newest scan of the map, which the last part of
    this test exercises."""
    ranges, odom = _queue()
    log_a, log_b = str(tmp_path / "a.log"), str(tmp_path / "b.log")
    a, queue_index = _build_map(log_a)
    b, _ = _build_map(log_b)
    n_map = a.num_scans()
    map_poses = a.poses()
    assert np.array_equal(map_poses, b.poses())
    # a pose between node 100 and node 101 (40 % of the way, 0.15 m to the side), with the readings taken at node 100
    node_a, node_b = 100, 101
    step = map_poses[node_b][:2] - map_poses[node_a][:2]
    side = np.array([-step[1], step[0]]) / np.hypot(*step)
    pose = map_poses[node_a].copy()
    pose[:2] += 0.4 * step + 0.15 * side
    want, _ = near_by_rule.find_near_by_scan(map_poses[:, :2], pose)
    assert want == node_a and near_by_rule.best_two_differ(map_poses[:, :2], pose)
    scan_ranges = ranges[queue_index[node_a]]
    a.set_log(log_a + ".1"); b.set_log(log_b + ".1")           # a log of its own for the call
    ok_a, pose_a, cov_a = a.ProcessAgainstNodesNearBy(scan_ranges, pose, 100.0, add_to_localization_buffer=False)
    ok_b, pose_b, cov_b = b.ProcessAgainstNode(scan_ranges, pose, want, 100.0)
    assert ok_a and ok_b
    assert np.array_equal(bits(pose_a), bits(pose_b)) and np.array_equal(bits(cov_a), bits(cov_b))
    a.set_log(log_a + ".2"); b.set_log(log_b + ".2")           # (closes and flushes)
    new_a, new_b = _lines(log_a + ".1"), _lines(log_b + ".1")
    assert new_a == new_b
    new_id = n_map
    assert new_a[0].startswith(f"N {new_id} ")
    links = [l.split()[1:3] for l in new_a if l.startswith("C ")]
    assert links[0] == [str(new_id - 1), str(new_id)], links         # AddEdges' link to state id - 1 (Mapper.cpp:1441-1449)
    assert links[1] == [str(want), str(new_id)], links               # the first link out of the running scans = the node
    # the vertex carries the pose of the match (AddVertex precedes AddEdges): the stand-alone match of the same scan against the node's scan alone
    mean, cov = _standalone_match(scan_ranges, pose, b.scan(want)[0])
    n_pose = np.array([float(v) for v in new_a[0].split()[2:5]])
    assert np.array_equal(bits(n_pose), bits(mean)), (n_pose, mean)
    assert np.array_equal(bits(cov_a), bits(cov))
    assert not np.array_equal(cov_a, np.eye(3))
    assert len(a.localization_buffer()) == 0 and len(a.alive()) == n_map + 1
    # the next scan's odometry delta starts at the corrected pose: 0.3 m on is dropped, 0.6 m on is accepted (minimum travel 0.5)
    print(f"near-by entry: node {want}, requested pose {pose}, corrected pose {pose_a}, moved {np.hypot(*(pose_a[:2] - pose[:2])):.3f} m")
    away = pose_a[:2] - pose[:2]
    away = away / np.hypot(*away) if np.hypot(*away) > 0 else np.array([1.0, 0.0])
    near = np.array([pose_a[0] + 0.3 * away[0], pose_a[1] + 0.3 * away[1], pose_a[2]])
    far = np.array([pose_a[0] + 0.6 * away[0], pose_a[1] + 0.6 * away[1], pose_a[2]])
    # (validity of the probe, not a bound on the match: measured from the REQUESTED pose the 0.3 m scan would have travelled enough)
    assert np.hypot(*(near[:2] - pose[:2])) >= 0.5 and np.hypot(*(near[:2] - pose_a[:2])) < 0.5 - 1e-3
    for mapper in (a, b):
        assert not mapper.ProcessLocalization(scan_ranges, near, 100.1)[0]
        assert mapper.ProcessLocalization(scan_ranges, far, 100.2)[0]
        assert list(mapper.localization_buffer()) == [new_id + 1]
    # ProcessAtDock == ProcessAgainstNode(0)
    dock_pose = map_poses[0] + np.array([0.1, -0.05, 0.02])
    ok_a, pose_a, cov_a = a.ProcessAtDock(ranges[queue_index[0]], dock_pose, 101.0)
    ok_b, pose_b, cov_b = b.ProcessAgainstNode(ranges[queue_index[0]], dock_pose, 0, 101.0)
    assert ok_a and ok_b and np.array_equal(bits(pose_a), bits(pose_b)) and np.array_equal(bits(cov_a), bits(cov_b))
    # the nearest node is the newest scan: `C <node> <new>` is the first link of the call
    newest = a.num_scans() - 1
    at = a.poses()[newest]
    a.set_log(log_a + ".3")
    assert a.ProcessAgainstNodesNearBy(ranges[queue_index[0]], at + np.array([0.02, 0.0, 0.0]), 102.0, add_to_localization_buffer=True)[0]
    assert list(a.localization_buffer()) == [new_id + 1, newest + 1]
    a.set_log(None)
    first_link = next(l for l in _lines(log_a + ".3") if l.startswith("C "))
    assert first_link.split()[1:3] == [str(newest), str(newest + 1)]
    # a removed or unknown id
    b.RemoveNode(50)
    for gone in (50, b.num_scans(), -1):
        with pytest.raises(capi.KartoHipError) as err:
            b.ProcessAgainstNode(scan_ranges, pose, gone, 103.0)
        assert f"status {capi.KH_ERR_NOT_FOUND} " in str(err.value)
    a.close(); b.close()


def test_near_by_on_an_empty_graph_makes_the_first_vertex(kartohip_lib):
    """Mapper.cpp:2772-2779, 2785: no vertex, no last scan, no match"""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = _queue()
    m = Mapper(synth.Laser())
    ok, pose, cov = m.ProcessAgainstNodesNearBy(ranges[0], odom[0], 0.0, add_to_localization_buffer=True)
    assert ok and np.array_equal(bits(pose), bits(odom[0])) and np.array_equal(cov, np.eye(3))
    assert m.stats()["matches"] == 0 and list(m.alive()) == [0] and list(m.localization_buffer()) == [0]
    m.close()


def test_clear_localization_buffer(kartohip_lib):
    """Mapper::ClearLocalizationBuffer (Mapper.cpp:2939-2962): the buffered scans leave, the map stays, the running scans and the
    last scan are cleared, so the next scan is a first scan: accepted without the gate and without a match (stats.matches
    unchanged, and so are the sequential matcher's own counters); the one after matches again."""
    ranges, odom = _queue()
    m, _ = _build_map()
    n_map = m.num_scans()
    done = 0
    i = SWITCH
    while done < 30:
        done += int(m.ProcessLocalization(ranges[i], odom[i], 0.1 * i)[0])
        i += 1
    assert len(m.alive()) == n_map + BUFFER and len(m.localization_buffer()) == BUFFER
    assert m.stats()["nodes_removed"] == 30 - BUFFER
    m.ClearLocalizationBuffer()
    assert np.array_equal(m.alive(), np.arange(n_map)) and len(m.localization_buffer()) == 0
    assert m.stats()["nodes_removed"] == 30

    def sequential(st):
        return st["fused_matches"] + st["fused_declined"]
    before = m.stats()
    # not moved at all since the last accepted scan: only a first scan gets past HasMovedEnough
    ok, pose, cov = m.ProcessLocalization(ranges[i - 1], odom[i - 1], 0.1 * i)
    after = m.stats()
    print(f"after the clear: matches {before['matches']} -> {after['matches']}, loop candidates {before['loop_candidates']} -> "
          f"{after['loop_candidates']}, sequential {sequential(before)} -> {sequential(after)}")
    assert ok and np.array_equal(cov, np.eye(3))
    assert sequential(after) == sequential(before)
    assert after["matches"] == before["matches"]
    assert list(m.localization_buffer()) == [m.num_scans() - 1]
    j = i
    while not m.ProcessLocalization(ranges[j], odom[j], 0.1 * j + 1.0)[0]:
        j += 1
    last = m.stats()
    assert sequential(last) == sequential(after) + 1 and last["matches"] > after["matches"]
    assert len(m.localization_buffer()) == 2 and len(m.alive()) == n_map + 2
    m.close()


def test_near_by_query_kernels(kartohip_lib):
    """kh_graph_find_near_by_scan / _vertices against tests/near_by_rule.py: 256 queries over 50 000 random vertices in one call,
    again after a third of the vertices left (compact indices) and after a few were re-posed; radius hits as ordered lists."""
    from slam_toolbox_amd.loop_search import MapperGraphSearch
    rng = np.random.default_rng(7)
    n, nq = 50000, 256
    points = rng.uniform(-60.0, 60.0, size=(n, 2))
    queries = rng.uniform(-65.0, 65.0, size=(nq, 2))
    empty_ptr = np.zeros(n + 1, dtype=np.int32)
    g = MapperGraphSearch()
    assert g.FindNearByScan((0.0, 0.0)) == (-1, np.inf) and g.FindNearByVertices((0.0, 0.0), 5.0).size == 0       # empty store

    def check(pts, radii=(0.5, 4.0, 30.0)):
        want = [near_by_rule.find_near_by_scan(pts, q) for q in queries]
        assert all(near_by_rule.best_two_differ(pts, q) for q in queries), "exact tie: change the seed"
        nearest, dist_sq = g.FindNearByScan(queries)
        assert np.array_equal(nearest, np.array([w[0] for w in want], dtype=np.int32))
        assert np.array_equal(bits(dist_sq), bits(np.array([w[1] for w in want])))
        one = g.FindNearByScan(queries[5])
        assert one[0] == want[5][0] and bits(one[1]) == bits(want[5][1])
        n_hits = 0
        for q in queries[:24]:
            for r in radii:
                assert near_by_rule.hits_are_distinct(pts, q, r), "tie among the hits or a hit at the radius: change the seed"
                hits = g.FindNearByVertices(q, r)
                assert np.array_equal(hits, near_by_rule.find_near_by_vertices(pts, q, r))
                n_hits += hits.size
        return n_hits

    g.SetGraph(points, empty_ptr, np.zeros(0, dtype=np.int32))
    with pytest.raises(capi.KartoHipError):                    # a store without poses does not answer from the reference points
        g.FindNearByScan(queries)
    g.SetPoses(points)
    hits = check(points)
    print(f"near-by kernels: 256 queries over {n} vertices {g.last_near_by_kernel_ms():.3f} ms (device), {hits} radius hits checked")
    assert hits > 100
    # a third of the vertices leave: the store is rebuilt over the rest, indices are positions in the new list
    keep = np.ones(n, dtype=bool)
    keep[rng.choice(n, n // 3, replace=False)] = False
    rest = np.ascontiguousarray(points[keep])
    g.SetGraph(rest, np.zeros(rest.shape[0] + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    g.SetPoses(rest)
    check(rest)
    # a few are re-posed, one is appended
    for k in rng.choice(rest.shape[0], 5, replace=False):
        rest[k] = queries[int(k) % nq] + rng.uniform(-0.01, 0.01, size=2)
        g.SetPose(int(k), rest[k])
    extra = queries[200] + np.array([0.003, -0.002])
    g.AppendScan(extra, extra)
    rest = np.vstack([rest, extra])
    check(rest)
    assert g.FindNearByScan(queries[200])[0] == rest.shape[0] - 1
    # the library's tie rule: equal distances -> the lower index
    tie = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [3.0, 3.0]])
    g.SetGraph(tie, np.zeros(6, dtype=np.int32), np.zeros(0, dtype=np.int32))
    g.SetPoses(tie)
    assert g.FindNearByScan((0.0, 0.0)) == (0, 1.0)
    assert list(g.FindNearByVertices((0.0, 0.0), 1.0)) == [] and list(g.FindNearByVertices((0.0, 0.0), 1.5)) == [0, 1, 2, 3]
    g.close()
