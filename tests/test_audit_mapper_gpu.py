"""GPU: single-edge edits, the audit and the rejection loop on a mapper (kh_mapper_add_edge, kh_mapper_remove_edge,
kh_mapper_correct_poses, kh_mapper_audit, kh_mapper_reject_outliers).

The mapper takes the lap queue of tests/test_localization_gpu.py (the queue tests/test_merge_align_gpu.py maps) until it has
accepted N_SCANS = 60 scans: of the first 60 QUEUE scans the travel gate accepts 39 (steps of 0.5 m against
minimum_travel_distance 0.5), so a scan 55 exists only once 60 scans are in the map.  A false edge 2 -> 55 is added by hand, its
mean the true sensor pose of scan 55 moved by (1.0, -0.7, 0.4), and corrected; RejectOutliers must remove exactly that edge and
leave the graph, the solver's constraint list and the session file as they were.  The second mapper is taken through the same
steps -- the solve that opens a rejection round included -- with the edge removed by hand: the poses must agree bit for bit, which
pins the audit's neutrality and the removal path at once."""
import ctypes as C

import numpy as np
import pytest

import audit_rule as ar
import test_localization_gpu as loc
from slam_toolbox_amd import capi, synth

pytestmark = pytest.mark.gpu
N_SCANS = 60
FALSE_FROM, FALSE_TO = 2, 55
OFFSET = np.array([1.0, -0.7, 0.4])
FALSE_COV = np.diag([1e-3, 1e-3, 4e-4])


def _build():
    """(mapper, queue index of every accepted scan)"""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = loc._queue()
    m = Mapper(synth.Laser(), loop_search_maximum_distance=loc.LOOP_DIST)
    taken = []
    for i in range(len(ranges)):
        if m.Process(ranges[i], odom[i], 0.1 * i)[0]:
            taken.append(i)
        if len(taken) == N_SCANS:
            break
    assert m.num_scans() == N_SCANS
    return m, taken


def _constraints(m):
    L = capi.lib()
    s = L.kh_mapper_solver(m._h)
    out, a, b = [], C.c_int32(), C.c_int32()
    for k in range(L.kh_spa_num_constraints(s)):
        z, w = np.zeros(3), np.zeros(6)
        capi.check(L.kh_spa_get_constraint(s, k, C.byref(a), C.byref(b), z, w), "kh_spa_get_constraint")
        out.append((a.value, b.value, z.tobytes(), w.tobytes()))
    return out


def _adjacency(m):
    return [m.adjacency(i).tolist() for i in range(N_SCANS)]


def _components(adj):
    return ar.components(len(adj), [(i, j) for i, row in enumerate(adj) for j in row])


@pytest.fixture(scope="module")
def pair(kartohip_lib):
    (a, taken), (b, _) = _build(), _build()
    yield a, b, taken
    a.close(); b.close()


def test_rejection_removes_the_false_edge_and_nothing_else(pair, tmp_path):
    a, b, taken = pair
    assert a.poses().tobytes() == b.poses().tobytes()
    adjacency, n_edges, constraints = _adjacency(a), a.num_edges(), _constraints(a)
    n_components = _components(adjacency)
    assert n_edges == len(constraints)

    # ---- the untouched mapper: nothing is removed, and the poses are those of one plain CorrectPoses
    removed = a.RejectOutliers()
    s = a.reject_summary
    print("[audit mapper] untouched:", s)
    assert len(removed) == 0 and s["rounds"] == 1 and s["n_removed"] == 0 and s["max_chi2_loo"] <= ar.CHI2_999
    b.CorrectPoses()
    assert a.poses().tobytes() == b.poses().tobytes()
    assert _adjacency(a) == adjacency and a.num_edges() == n_edges and _constraints(a) == constraints

    # ---- a missing edge: NOT_FOUND, nothing changes (the direction counts)
    before = a.poses().tobytes()
    for missing in ((FALSE_FROM, FALSE_TO), (1, 0), (0, N_SCANS + 5), (-1, 3)):
        with pytest.raises(capi.KartoHipError) as err:
            a.RemoveEdge(*missing)
        assert err.value.code == capi.KH_ERR_NOT_FOUND, missing
    assert _adjacency(a) == adjacency and a.num_edges() == n_edges and _constraints(a) == constraints and a.poses().tobytes() == before
    with pytest.raises(capi.KartoHipError) as err:
        a.AddEdge(FALSE_FROM, N_SCANS + 5, [0.0, 0.0, 0.0], FALSE_COV)
    assert err.value.code == capi.KH_ERR_NOT_FOUND and a.num_edges() == n_edges

    # ---- the false closure, by hand on both mappers
    truth, _ = synth.trajectory_laps(loc.N_QUEUE)
    mean = np.asarray(truth[taken[FALSE_TO]], dtype=np.float64) + OFFSET        # (the laser sits at the robot's centre)
    for m in (a, b):
        m.AddEdge(FALSE_FROM, FALSE_TO, mean, FALSE_COV, correct=True)
        assert m.num_edges() == n_edges + 1 and FALSE_TO in m.adjacency(FALSE_FROM) and FALSE_FROM in m.adjacency(FALSE_TO)
    assert a.poses().tobytes() == b.poses().tobytes() and _constraints(a)[-1][:2] == (FALSE_FROM, FALSE_TO)
    a.AddEdge(FALSE_FROM, FALSE_TO, mean, FALSE_COV, correct=False)               # LinkScans' duplicate test: nothing is attached
    assert a.num_edges() == n_edges + 1 and len(_constraints(a)) == len(constraints) + 1
    rec = a.audit()
    cand = ar.candidates(rec["id_a"], rec["id_b"], rec["verifiable"], 2)
    print("[audit mapper] false edge:", rec[-1], "candidates", int(cand.sum()), "verifiable", int(rec["verifiable"].sum()), "of", len(rec))
    assert len(rec) == n_edges + 1 and (rec["id_a"][-1], rec["id_b"][-1]) == (FALSE_FROM, FALSE_TO)

    removed = a.RejectOutliers()
    s = a.reject_summary
    print("[audit mapper] rejection:", s, removed)
    assert [(int(r["id_a"]), int(r["id_b"]), int(r["index"])) for r in removed] == [(FALSE_FROM, FALSE_TO, n_edges)]
    assert removed[0]["verifiable"] == 1 and removed[0]["chi2_loo"] > ar.CHI2_999
    assert s["rounds"] == 2 and s["n_removed"] == 1 and s["max_chi2_loo"] <= ar.CHI2_999
    assert s["solve_ms"] > 0.0 and s["audit_ms"] > 0.0 and s["total_ms"] >= s["solve_ms"] + s["audit_ms"] - 1e-6
    assert _adjacency(a) == adjacency and a.num_edges() == n_edges and _constraints(a) == constraints
    assert _components(_adjacency(a)) == n_components

    # ---- the same steps with the edge removed by hand
    b.CorrectPoses()
    b.RemoveEdge(FALSE_FROM, FALSE_TO)
    b.CorrectPoses()
    assert _adjacency(b) == adjacency and _constraints(b) == constraints
    assert a.poses().tobytes() == b.poses().tobytes()

    # ---- a mapper saves and loads as before after edge edits
    from slam_toolbox_amd.mapper import Mapper
    first, second = tmp_path / "a.session", tmp_path / "b.session"
    a.save(first)
    again = Mapper.load(first)
    again.save(second)
    assert first.read_bytes() == second.read_bytes()
    assert again.poses().tobytes() == a.poses().tobytes() and _adjacency(again) == adjacency and _constraints(again) == constraints
    again.close()
