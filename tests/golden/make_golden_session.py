"""Writes tests/golden/session_small.khms and session_small.npz (needs the GPU): a mapping session small enough to commit --
a laser with few beams on the lap queue until the first loop closure and a little further, one node removed, a few scans of
localization so that the rolling buffer is not empty -- saved with kh_mapper_save, together with the same state dumped through
the getters that existed before session files did.  tests/test_session_format.py reads both on a machine without a GPU.

    python tests/golden/make_golden_session.py [output directory]
"""
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from slam_toolbox_amd import capi, synth  # noqa: E402
from slam_toolbox_amd.mapper import Mapper  # noqa: E402

N_QUEUE, LOOP_DIST = 500, 3.0


def small_laser(n_beams):
    res = math.radians(270.0) / (n_beams - 1)
    return synth.Laser(n_beams=n_beams, ang_res=res)


def build(n_beams):
    laser = small_laser(n_beams)
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(N_QUEUE)
    rng = np.random.default_rng(4)
    m = Mapper(laser, loop_search_maximum_distance=LOOP_DIST)
    i, after = 0, 0
    while i < N_QUEUE and after < 6:                       # mapping until six scans behind the first closure
        ok = m.Process(synth.make_scan(world, truth[i], rng, laser), odom[i], 0.1 * i)[0]
        after += int(ok and m.stats()["loop_closures"] >= 1)
        i += 1
    if m.stats()["loop_closures"] < 1:
        m.close()
        return None
    m.RemoveNode(20)
    done = 0
    while i < N_QUEUE and done < 4:                        # four buffered scans
        done += int(m.ProcessLocalization(synth.make_scan(world, truth[i], rng, laser), odom[i], 0.1 * i)[0])
        i += 1
    assert done == 4
    return m


def dump(m):
    L = capi.lib()
    alive = m.alive()
    n_beams = m.n_beams
    out = {"alive": alive, "poses": m.poses()[alive], "n_scan_slots": np.int64(m.num_scans()), "n_edges": np.int64(m.num_edges()),
           "localization_buffer": m.localization_buffer()}
    out["ranges"] = np.stack([np.ctypeslib.as_array(m.scan(int(i))[0].ranges, (n_beams,)).copy() for i in alive])
    out["score"] = np.array([m.scan(int(i))[1].score for i in alive])
    adj = [m.adjacency(int(i)) for i in alive]
    out["adj_count"] = np.array([len(a) for a in adj], dtype=np.int32)
    out["adj"] = np.concatenate(adj).astype(np.int32)
    s = L.kh_mapper_solver(m._h)
    n, nc = L.kh_spa_num_nodes(s), L.kh_spa_num_constraints(s)
    ids, poses = np.zeros(n, dtype=np.int32), np.zeros(3 * n)
    capi.check(L.kh_spa_get_nodes(s, ids.ctypes.data, poses.ctypes.data), "kh_spa_get_nodes")
    out["node_ids"], out["node_poses"] = ids, poses.reshape(n, 3)
    a, b, z, info = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32), np.zeros((nc, 3)), np.zeros((nc, 6))
    for k in range(nc):
        ia, ib, zk, ik = C.c_int32(), C.c_int32(), np.zeros(3), np.zeros(6)
        capi.check(L.kh_spa_get_constraint(s, k, C.byref(ia), C.byref(ib), zk, ik), "kh_spa_get_constraint")
        a[k], b[k], z[k], info[k] = ia.value, ib.value, zk, ik
    out["constraint_a"], out["constraint_b"], out["constraint_z"], out["constraint_information"] = a, b, z, info
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
    os.makedirs(out_dir, exist_ok=True)
    for n_beams in (181, 271, 541):                        # the fewest beams with which the first lap still closes
        m = build(n_beams)
        if m is not None:
            break
        print(f"{n_beams} beams: no loop closure, trying more")
    assert m is not None, "no laser closed the loop"
    state = dump(m)
    path = os.path.join(out_dir, "session_small.khms")
    m.save(path)
    np.savez_compressed(os.path.join(out_dir, "session_small.npz"), n_beams=np.int64(m.n_beams), **state)
    st = m.stats()
    print(f"session_small: {m.n_beams} beams, {len(state['alive'])} scans alive of {m.num_scans()}, {st['loop_closures']} closures, "
          f"{st['nodes_removed']} removed, buffer {list(state['localization_buffer'])}, {os.path.getsize(path)} bytes")
    m.close()


if __name__ == "__main__":
    main()
