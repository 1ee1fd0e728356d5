"""GPU: the pose-graph covariances of the solver (kh_spa_compute_covariances: the selected inverse of the factor, walked back down
the assembly tree on the device) against the dense rule of tests/covariance_rule.py, evaluated at the poses the solver holds.

Every diagonal block, every edge's joint 6 x 6 and the gauge's zeros are checked.  A block's relative Frobenius error may be at
most 8 * ref_err(case), floor 64 * 2^-52 (covariance_rule.tolerance): ref_err is what float64 itself loses on the case, measured
by the rule alone.  The graphs are the smallest that reach each branch of the kernels: one front (2 / 1, 12 / 11, 12 / 20); a
root supernode of 177 pivots split into a chain by the 128-pivot limit, with fronts whose pivot count is no multiple of 16
(complete graph on 60 nodes); many levels, fronts with more than three children and deferred update blocks (60 / 120 and
200 / 500, as they are and with KH_SPA_LEAF=4); wide levels and the boundary where a level's small fronts leave for the fused
update kernel (1000 / 3000).  Which FRONT SHAPES the kernels see (pivot counts above 90, update blocks above 128 rows, chains of more
than two fronts) is not decided here: the table in DESIGN.md, section 7e ("Front shapes"), is the authority, and its cases run in
tests/test_covariance_shapes_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import covariance_rule as cr
from oracle import spa
from slam_toolbox_amd import capi, synth

pytestmark = pytest.mark.gpu


def make_solver(g, options=None, debug=None, compute=True):
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    sol = HipSpaSolver(options=options)
    if debug:
        sol.set_debug(**debug)
    sol.load(g["init"], g["edges"], g["z"], g["cov"])
    if compute:
        assert sol.Compute()["usable"] == 1 and sol.last_warning == ""
    return sol


def current_poses(sol, n):
    ids, poses = sol.node_arrays()
    x = np.zeros((n, 3))
    x[ids] = poses
    return x


def worst_error(sol, r, edges):
    """largest relative Frobenius error of a diagonal block / of an edge's joint 6 x 6 against rule (a); the gauge must be zeros"""
    p = r.problem
    nodes = np.concatenate([p.free_nodes, [p.fixed]]).astype(np.int32)
    got = sol.Covariances(nodes)
    assert not got[-1].any(), "the gauge node's covariance is not zero"
    assert not sol.Covariance(p.fixed).any()
    worst_diag = max(cr.rel_fro(got[k], cr.diag_block(r, node)) for k, node in enumerate(p.free_nodes))
    worst_joint = 0.0
    for a, b in edges:
        j = sol.JointCovariance(int(a), int(b))
        assert np.array_equal(j, j.T), "the joint covariance is not bit-wise symmetric"
        worst_joint = max(worst_joint, cr.rel_fro(j, cr.joint_block(r, a, b)))
    return worst_diag, worst_joint


def check(sol, g, tol, name, **rule_args):
    """tol = None: the case's own bound"""
    n = np.asarray(g["init"]).shape[0]
    r = cr.rule(current_poses(sol, n), g["edges"], g["z"], cov=g["cov"], reference=tol is None, **rule_args)
    if tol is None:
        tol = cr.tolerance(cr.ref_err(r))
    worst_diag, worst_joint = worst_error(sol, r, g["edges"])
    print(f"[covariance] {name}: diagonal blocks {worst_diag:.3e}, joint blocks {worst_joint:.3e}, bound {tol:.3e}")
    assert worst_diag <= tol and worst_joint <= tol, (name, worst_diag, worst_joint, tol)
    return r


GRAPHS = {
    "2/1": (lambda: cr.chain(2), None),
    "12/11": (lambda: synth.make_pose_graph(12, 11, seed=2), None),
    "12/20": (lambda: synth.make_pose_graph(12, 20, seed=2), None),
    "complete 60": (lambda: cr.complete_graph(60), None),
    "60/120": (lambda: synth.make_pose_graph(60, 120, seed=4), None),
    "60/120 leaf 4": (lambda: synth.make_pose_graph(60, 120, seed=4), "4"),
    "200/500": (lambda: synth.make_pose_graph(200, 500, seed=4), None),
    "200/500 leaf 4": (lambda: synth.make_pose_graph(200, 500, seed=4), "4"),
    "1000/3000": (lambda: synth.make_pose_graph(1000, 3000, seed=4), None),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_covariances_match_the_rule(kartohip_lib, monkeypatch, name):
    build, leaf = GRAPHS[name]
    g = build()
    if leaf:
        monkeypatch.setenv("KH_SPA_LEAF", leaf)          # read by the handle's analysis
    sol = make_solver(g)
    summ = sol.ComputeCovariances()
    n = g["init"].shape[0]
    r = cr.rule(current_poses(sol, n), g["edges"], g["z"], cov=g["cov"])
    err = cr.ref_err(r)
    tol = cr.tolerance(err)
    assert summ["n_free"] == r.problem.nfree and summ["levels"] >= 1 and summ["inverse_flops"] >= 0 and summ["total_ms"] > 0.0
    worst_diag, worst_joint = worst_error(sol, r, g["edges"])
    print(f"[covariance] {name}: ref_err {err:.3e}, diagonal blocks {worst_diag:.3e}, joint blocks {worst_joint:.3e}, bound {tol:.3e}, "
          f"levels {summ['levels']}")
    assert worst_diag <= tol and worst_joint <= tol, (name, err, worst_diag, worst_joint, tol)
    # all nodes at once, insertion order
    every = sol.Covariances()
    assert every.shape == (n, 3, 3) and np.array_equal(every[r.problem.free_nodes[0]], sol.Covariance(r.problem.free_nodes[0]))
    sol.close()


# ---- variants on 200 / 500: all under the bound of the plain case -----------------------------------------------------------
@pytest.fixture(scope="module")
def g200():
    return synth.make_pose_graph(200, 500, seed=4)


@pytest.fixture(scope="module")
def tol200(kartohip_lib, g200):
    sol = make_solver(g200)
    r = cr.rule(current_poses(sol, 200), g200["edges"], g200["z"], cov=g200["cov"])
    sol.close()
    return cr.tolerance(cr.ref_err(r))


def test_variant_jacobi_scaling_off(g200, tol200):
    sol = make_solver(g200, options=dict(jacobi_scaling=0))
    sol.ComputeCovariances()
    check(sol, g200, tol200, "200/500 without Jacobi scaling", jacobi=False)
    sol.close()


def test_variant_huber_loss_with_yaw_noise(g200, tol200):
    g = dict(g200, z=g200["z"].copy())
    g["z"][::7, 2] += 0.3                                   # 15 sigma of yaw: these edges sit on the linear branch of the loss
    sol = make_solver(g, options=dict(loss_function="HuberLoss", loss_scale=0.7))
    sol.ComputeCovariances()
    r = check(sol, g, tol200, "200/500 HuberLoss", loss="HuberLoss", loss_scale=0.7)
    res, _ = spa._residuals(current_poses(sol, 200), g["edges"][:, 0], g["edges"][:, 1], g["z"], r.problem.U)
    sq = np.sum(res * res, axis=1)
    assert (sq > 0.49).any() and (sq < 0.49).any(), "the case must have edges on both branches of the loss"
    sol.close()


@pytest.mark.parametrize("debug", [dict(gather_children=True), dict(extend_add_pass=True)], ids=["bit 8", "bit 9"])
def test_variant_gather_and_extend_add_forms(g200, tol200, debug):
    sol = make_solver(g200, debug=debug)
    sol.ComputeCovariances()
    check(sol, g200, tol200, f"200/500 {debug}")
    sol.close()


def _still_connected_without(n, edges, k):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    keep = (edges[:, 0] != k) & (edges[:, 1] != k)
    a = sp.coo_matrix((np.ones(keep.sum()), (edges[keep, 0], edges[keep, 1])), shape=(n, n))
    _, label = connected_components(a, directed=False)
    return len(set(np.delete(label, k).tolist())) == 1


def test_variant_after_remove_node(g200, tol200):
    k = next(k for k in range(90, 150) if _still_connected_without(200, g200["edges"], k))
    sol = make_solver(g200)
    sol.ComputeCovariances()
    sol.RemoveNode(k)
    with pytest.raises(capi.KartoHipError) as e:
        sol.Covariance(5)
    assert e.value.code == capi.KH_ERR_SOLVER and "stale" in str(e.value)
    assert sol.Compute()["usable"] == 1
    sol.ComputeCovariances()
    keep = (g200["edges"][:, 0] != k) & (g200["edges"][:, 1] != k)
    g = dict(g200, edges=g200["edges"][keep], z=g200["z"][keep], cov=g200["cov"][keep])
    check(sol, g, tol200, f"200/500 after RemoveNode({k})")
    with pytest.raises(capi.KartoHipError) as e:
        sol.Covariance(k)
    assert e.value.code == capi.KH_ERR_NOT_FOUND
    sol.close()


def test_variant_incremental_analysis_after_twenty_more_nodes(tol200):
    g = synth.make_pose_graph(220, 560, seed=4)
    old = (g["edges"][:, 0] < 200) & (g["edges"][:, 1] < 200)
    first = dict(init=g["init"][:200], edges=g["edges"][old], z=g["z"][old], cov=g["cov"][old])
    sol = make_solver(first)
    sol.ComputeCovariances()
    for i in range(200, 220):
        sol.AddNode(i, g["init"][i])
    sol._ids = list(range(220))
    for e in np.flatnonzero(~old):
        sol.AddConstraint(int(g["edges"][e, 0]), int(g["edges"][e, 1]), g["z"][e], g["cov"][e])
    summ = sol.Compute()
    assert summ["usable"] == 1 and summ["analysis"] == 2, summ
    assert sol.ComputeCovariances()["analysis"] == 0
    order = np.concatenate([np.flatnonzero(old), np.flatnonzero(~old)])
    check(sol, dict(g, edges=g["edges"][order], z=g["z"][order], cov=g["cov"][order]), tol200, "220/560 after an incremental analysis")
    sol.close()


def test_variant_before_any_compute(g200, tol200):
    sol = make_solver(g200, compute=False)
    summ = sol.ComputeCovariances()
    assert summ["analysis"] == 1
    check(sol, g200, tol200, "200/500 before any Compute")
    assert np.array_equal(current_poses(sol, 200), g200["init"])
    sol.close()


# ---- the pass leaves a Compute() as it found it -----------------------------------------------------------------------------
COUNTERS = ("iterations", "successful_steps", "termination", "usable", "initial_cost", "final_cost", "nnz_factor", "factor_flops",
            "factorizations", "levels", "analysis")


@pytest.mark.parametrize("debug", [dict(), dict(gather_children=True), dict(extend_add_pass=True)], ids=["default", "bit 8", "bit 9"])
def test_covariance_pass_does_not_interfere_with_compute(g200, debug):
    # (bit 0: every Compute and the covariance pass count the non-zero entries the self-cleaning fronts were left with)
    a = make_solver(g200, debug=dict(check_linear_solves=True, **debug), compute=False)
    b = make_solver(g200, debug=dict(check_linear_solves=True, **debug), compute=False)
    bump = np.array([0.3, -0.2, 0.05])
    for sol in (a, b):
        first = sol.Compute()
        assert first["usable"] == 1 and sol.last_warning == ""
        sol.first = (first, sol.iteration_log().copy(), sol.poses().copy())
        sol.ModifyNode(7, sol.poses()[7][:3] * [1, 1, 0] + bump)
        if sol is b:
            sol.ComputeCovariances()
            assert np.isfinite(sol.Covariances()).all()
        second = sol.Compute()
        assert second["usable"] == 1 and sol.last_warning == "", sol.last_warning
        sol.second = (second, sol.iteration_log().copy(), sol.poses().copy())
    for ra, rb in ((a.first, b.first), (a.second, b.second)):
        assert [ra[0][k] for k in COUNTERS] == [rb[0][k] for k in COUNTERS]
        assert ra[1].tobytes() == rb[1].tobytes() and ra[2].tobytes() == rb[2].tobytes()
    assert a.second[0]["iterations"] >= 1
    a.close()
    b.close()


# ---- states -----------------------------------------------------------------------------------------------------------------
def raises(code, fn, *args, text=None):
    with pytest.raises(capi.KartoHipError) as e:
        fn(*args)
    assert e.value.code == code, e.value
    if text:
        assert text in str(e.value), e.value


def test_getters_follow_the_state_of_the_graph(kartohip_lib):
    g = synth.make_pose_graph(12, 20, seed=2)
    sol = make_solver(g)
    raises(capi.KH_ERR_SOLVER, sol.Covariance, 3, text="stale")                   # nothing computed yet
    raises(capi.KH_ERR_SOLVER, sol.JointCovariance, 0, 1, text="stale")
    p, n = C.c_void_p(), C.c_int64()
    assert kartohip_lib.kh_spa_covariance_device(sol._h, C.byref(p), C.byref(n)) == capi.KH_ERR_SOLVER
    sol.ComputeCovariances()
    assert kartohip_lib.kh_spa_covariance_device(sol._h, C.byref(p), C.byref(n)) == capi.KH_OK and p.value and n.value >= 11
    have = {(int(a), int(b)) for a, b in g["edges"]} | {(int(b), int(a)) for a, b in g["edges"]}
    a, b = next((a, b) for a in range(1, 12) for b in range(1, 12) if a != b and (a, b) not in have)
    raises(capi.KH_ERR_NOT_FOUND, sol.JointCovariance, a, b, text="pattern")
    raises(capi.KH_ERR_NOT_FOUND, sol.Covariance, 99)
    sol.ModifyNode(3, [0.0, 0.0, 0.0])
    raises(capi.KH_ERR_SOLVER, sol.Covariance, 3, text="stale")
    sol.ComputeCovariances()
    sol.Covariance(3)
    sol.AddConstraint(a, b, np.zeros(3), np.eye(3) * 0.01)
    raises(capi.KH_ERR_SOLVER, sol.Covariances, text="stale")
    sol.ComputeCovariances()
    sol.JointCovariance(a, b)
    sol.AddNode(50, [0.0, 0.0, 0.0])                                                 # no constraint touches it
    sol.ComputeCovariances()
    raises(capi.KH_ERR_NOT_FOUND, sol.Covariance, 50, text="no constraints")
    sol.close()


def test_factor_mode_two_is_refused(kartohip_lib):
    sol = make_solver(synth.make_pose_graph(12, 20, seed=2), debug=dict(factor_kernels=2))
    raises(capi.KH_ERR_SOLVER, sol.ComputeCovariances, text="level pipeline")
    raises(capi.KH_ERR_SOLVER, sol.Covariance, 3, text="stale")
    sol.close()


def test_component_not_tied_to_the_gauge_is_refused_and_the_handle_recovers(kartohip_lib):
    g = cr.chain(6)
    cut = np.array([0, 1, 3, 4])                                                   # 0-1-2 and 3-4-5
    parts = dict(init=g["init"], edges=g["edges"][cut], z=g["z"][cut], cov=g["cov"][cut])
    sol = make_solver(parts)
    raises(capi.KH_ERR_SOLVER, sol.ComputeCovariances, text="not tied to the gauge")
    raises(capi.KH_ERR_SOLVER, sol.Covariance, 1, text="stale")
    sol.AddConstraint(2, 3, g["z"][2], g["cov"][2])
    assert sol.Compute()["usable"] == 1
    sol.ComputeCovariances()
    order = np.array([0, 1, 3, 4, 2])
    check(sol, dict(g, edges=g["edges"][order], z=g["z"][order], cov=g["cov"][order]), None, "chain of 6, repaired")
    sol.close()


# ---- mapper -----------------------------------------------------------------------------------------------------------------
def test_mapper_covariances_are_the_solvers_and_lazy(kartohip_lib):
    from slam_toolbox_amd.mapper import Mapper
    n_scans = 40
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_scans)
    rng = np.random.default_rng(4)
    m = Mapper(synth.Laser())
    for i in range(n_scans):
        m.Process(synth.make_scan(world, truth[i], rng), odom[i], 0.1 * i)
    L = kartohip_lib
    solver = L.kh_mapper_solver(m._h)
    n = L.kh_spa_num_nodes(solver)
    assert n > 10
    ids = np.zeros(n, dtype=np.int32)
    assert L.kh_spa_get_nodes(solver, ids.ctypes.data_as(C.c_void_p), None) == capi.KH_OK
    every = m.covariances()
    assert m.cov_summary["total_ms"] > 0.0 and m.cov_summary["n_free"] == n - 1
    own = np.zeros((n, 3, 3))
    assert L.kh_spa_get_covariances(solver, n, None, own.ctypes.data_as(C.c_void_p)) == capi.KH_OK
    assert np.array_equal(every, own) and not every[0].any() and np.isfinite(every).all()
    assert all(np.linalg.eigvalsh(c).min() > 0.0 for c in every[1:])
    some = m.covariances(ids[[3, 1, n - 1]])
    assert m.cov_summary["total_ms"] == 0.0 and m.cov_summary["n_free"] == 0           # answered from the resident result
    assert np.array_equal(some, own[[3, 1, n - 1]])
    m.close()
