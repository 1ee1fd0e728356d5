"""GPU: the covariance columns of the solver (kh_spa_compute_covariance_columns: A X = E_q through the multifrontal factor while a
covariance pass has it in the fronts) against the dense rule of tests/covariance_rule.py, evaluated at the poses the solver holds.

A block's error is taken relative to sqrt(|Sigma_ii|_F |Sigma_qq|_F) (tests/covariance_columns_rule.py) and may be at most
covariance_rule.tolerance(ref_err) = max(8 ref_err, 64 * 2^-52), ref_err the same measure between rule (a) and rule (b).  The
graphs are those of tests/test_covariance_gpu.py, the smallest that reach each branch: one front and one free node (2 / 1); a
177-pivot root split into a chain, pivot counts no multiple of 16 (complete 60); many levels and merging paths (60 / 120 with leaves
of 4); 3, 15, 18, 48, 51 and 192 right-hand-side columns, inside, across and exactly on the 16-column tile (200 / 500); wide levels
(1000 / 3000)."""
import ctypes as C

import numpy as np
import pytest

import covariance_columns_rule as ccr
import covariance_rule as cr
from slam_toolbox_amd import capi, synth
from slam_toolbox_amd.scan_solver import relative_covariance
from test_covariance_gpu import COUNTERS, _still_connected_without, current_poses, make_solver, raises

pytestmark = pytest.mark.gpu


def rule_at(sol, g, **rule_args):
    """rule (a) at the poses the solver holds"""
    n = np.asarray(g["init"]).shape[0]
    return cr.rule(current_poses(sol, n), g["edges"], g["z"], cov=g["cov"], reference=False, **rule_args)


def columns_of(sol, r, query_nodes):
    """{query node: (n_free, 3, 3)} rows in the rule's block order"""
    return {int(q): sol.CovarianceColumn(int(q), r.problem.free_nodes.astype(np.int32)) for q in query_nodes}


def worst_error(r, got):
    scale = ccr.scales(r.sigma)
    n = r.problem.nfree
    return max(ccr.column_error(col, ccr.blocks(r.sigma, range(n), r.problem.col_of[q]), scale, r.problem.col_of[q]) for q, col in got.items())


def three_queries(r):
    f = r.problem.free_nodes
    return [int(f[0]), int(f[len(f) // 2]), int(f[-1])]


# ---- the full inverse: every free node a query, every combination of paths ---------------------------------------------------
@pytest.mark.parametrize("name", ["complete 60", "60/120 leaf 4"])
def test_every_column_of_the_inverse(kartohip_lib, monkeypatch, name):
    g = cr.complete_graph(60) if name == "complete 60" else synth.make_pose_graph(60, 120, seed=4)
    if name.endswith("leaf 4"):
        monkeypatch.setenv("KH_SPA_LEAF", "4")             # read by the handle's analysis
    sol = make_solver(g)
    r = rule_at(sol, g)
    nodes = [int(v) for v in r.problem.free_nodes]
    assert len(nodes) == 59
    summ = sol.ComputeCovarianceColumns(nodes)
    assert summ["n_queries"] == 59 and summ["path_fronts"] >= 1 and summ["column_flops"] > 0 and summ["total_ms"] > 0.0
    assert summ["cov"]["n_free"] == 59 and summ["path_fronts"] <= 59 * summ["cov"]["levels"]
    err, _ = ccr.ref_err(r, list(range(59)))
    tol = cr.tolerance(err)
    got = columns_of(sol, r, nodes)
    worst = worst_error(r, got)
    # block (i, q) of column q against the transpose of block (q, i) of column i
    scale = ccr.scales(r.sigma)
    full = np.stack([got[q] for q in nodes])                                      # [q][i]
    d = full - np.transpose(full, (1, 0, 3, 2))
    asym = float(np.max(np.sqrt(np.sum(d * d, axis=(2, 3))) / np.sqrt(np.outer(scale, scale))))
    print(f"[covariance columns] {name}: ref_err {err:.3e}, worst block {worst:.3e}, column q against column i transposed {asym:.3e}, "
          f"bound {tol:.3e}, levels {summ['cov']['levels']}, path fronts {summ['path_fronts']}")
    assert worst <= tol and asym <= tol, (name, err, worst, asym, tol)
    sol.close()


# ---- 200 / 500: the plain case, whose bound the variants share ---------------------------------------------------------------
@pytest.fixture(scope="module")
def g200():
    return synth.make_pose_graph(200, 500, seed=4)


@pytest.fixture(scope="module")
def plain200(kartohip_lib, g200):
    """rule (a) at the solved poses, the bound from the first 64 free nodes' columns"""
    sol = make_solver(g200)
    r = rule_at(sol, g200)
    sol.close()
    err, _ = ccr.ref_err(r, list(range(64)))
    return r, cr.tolerance(err), err


def test_column_tiles_and_columns_do_not_depend_on_the_company(g200, plain200):
    r, tol, err = plain200
    sol = make_solver(g200)
    seen = {}
    for count in (1, 5, 6, 16, 17, 64):                     # 3, 15, 18, 48, 51, 192 columns of right-hand sides
        nodes = [int(v) for v in r.problem.free_nodes[:count]]
        summ = sol.ComputeCovarianceColumns(nodes)
        assert summ["n_queries"] == count
        got = columns_of(sol, r, nodes)
        worst = worst_error(r, got)
        print(f"[covariance columns] 200/500, {count} queries: ref_err {err:.3e}, worst block {worst:.3e}, bound {tol:.3e}, "
              f"path fronts {summ['path_fronts']}")
        assert worst <= tol, (count, worst, tol)
        for q, col in got.items():
            assert seen.setdefault(q, col).tobytes() == col.tobytes(), f"column of node {q} changed with {count} queries"
    sol.close()


# ---- gauge and edge rows -----------------------------------------------------------------------------------------------------
def test_one_free_node_and_the_gauge_as_query_and_as_row(kartohip_lib):
    g = cr.chain(2)
    sol = make_solver(g)
    r = rule_at(sol, g)
    err, _ = ccr.ref_err(r, [0])
    tol = cr.tolerance(err)
    sol.ComputeCovarianceColumns([1, 0])
    col = sol.CovarianceColumn(1)                           # all nodes, insertion order: the gauge first
    assert col.shape == (2, 3, 3) and not col[0].any(), "the gauge as a row is not zeros"
    marginal = sol.Covariance(1)
    scale = ccr.scales(r.sigma)
    e_rule = ccr.column_error(col[1:], ccr.blocks(r.sigma, [0], 0), scale, 0)
    e_marg = ccr.column_error(col[1:], marginal[None], scale, 0)
    print(f"[covariance columns] 2/1: against the rule {e_rule:.3e}, against the marginal {e_marg:.3e}, bound {tol:.3e}")
    assert e_rule <= tol and e_marg <= tol
    assert not sol.CovarianceColumn(0).any(), "the gauge as a query is not zeros"
    assert not sol.CovarianceColumn(0, [1]).any()
    sol.close()
    g = synth.make_pose_graph(12, 20, seed=2)
    sol = make_solver(g)
    sol.ComputeCovarianceColumns([0, 5])
    assert not sol.CovarianceColumn(0).any() and not sol.CovarianceColumn(5, [0]).any() and sol.CovarianceColumn(5, [5]).any()
    j = sol.JointCovarianceAny(5, 0)
    assert not j[3:].any() and not j[:, 3:].any() and np.array_equal(j[:3, :3], sol.Covariance(5))
    sol.close()


# ---- wide levels -------------------------------------------------------------------------------------------------------------
def test_wide_levels_against_numpy_inverse(kartohip_lib):
    g = synth.make_pose_graph(1000, 3000, seed=4)
    sol = make_solver(g)
    r = rule_at(sol, g)
    nodes = three_queries(r)
    err, _ = ccr.ref_err(r, [int(r.problem.col_of[q]) for q in nodes])
    tol = cr.tolerance(err)
    summ = sol.ComputeCovarianceColumns(nodes)
    worst = worst_error(r, columns_of(sol, r, nodes))
    print(f"[covariance columns] 1000/3000: ref_err {err:.3e}, worst block {worst:.3e}, bound {tol:.3e}, levels {summ['cov']['levels']}, "
          f"path fronts {summ['path_fronts']}")
    assert worst <= tol, (err, worst, tol)
    sol.close()


# ---- variants on 200 / 500: all under the bound of the plain case ------------------------------------------------------------
def check_variant(sol, g, tol, name, **rule_args):
    r = rule_at(sol, g, **rule_args)
    nodes = three_queries(r)
    sol.ComputeCovarianceColumns(nodes)
    worst = worst_error(r, columns_of(sol, r, nodes))
    print(f"[covariance columns] {name}: worst block {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol, (name, worst, tol)
    return r


def test_variant_jacobi_scaling_off(g200, plain200):
    sol = make_solver(g200, options=dict(jacobi_scaling=0))
    check_variant(sol, g200, plain200[1], "200/500 without Jacobi scaling", jacobi=False)
    sol.close()


def test_variant_huber_loss_with_yaw_noise(g200, plain200):
    g = dict(g200, z=g200["z"].copy())
    g["z"][::7, 2] += 0.3                                   # 15 sigma of yaw: these edges sit on the linear branch of the loss
    sol = make_solver(g, options=dict(loss_function="HuberLoss", loss_scale=0.7))
    check_variant(sol, g, plain200[1], "200/500 HuberLoss", loss="HuberLoss", loss_scale=0.7)
    sol.close()


@pytest.mark.parametrize("debug", [dict(gather_children=True), dict(extend_add_pass=True)], ids=["bit 8", "bit 9"])
def test_variant_gather_and_extend_add_forms(g200, plain200, debug):
    sol = make_solver(g200, debug=debug)
    check_variant(sol, g200, plain200[1], f"200/500 {debug}")
    sol.close()


def test_variant_before_any_compute(g200, plain200):
    sol = make_solver(g200, compute=False)
    check_variant(sol, g200, plain200[1], "200/500 before any Compute")
    assert sol.cov_columns_summary["cov"]["analysis"] == 1
    assert np.array_equal(current_poses(sol, 200), g200["init"])
    sol.close()


def test_variant_after_remove_node(g200, plain200):
    k = next(k for k in range(90, 150) if _still_connected_without(200, g200["edges"], k))
    sol = make_solver(g200)
    sol.ComputeCovarianceColumns([5, k])
    sol.RemoveNode(k)
    raises(capi.KH_ERR_SOLVER, sol.CovarianceColumn, 5, text="stale")
    assert sol.Compute()["usable"] == 1
    keep = (g200["edges"][:, 0] != k) & (g200["edges"][:, 1] != k)
    g = dict(g200, edges=g200["edges"][keep], z=g200["z"][keep], cov=g200["cov"][keep])
    check_variant(sol, g, plain200[1], f"200/500 after RemoveNode({k})")
    raises(capi.KH_ERR_NOT_FOUND, sol.ComputeCovarianceColumns, [5, k])
    sol.close()


def test_variant_incremental_analysis_after_twenty_more_nodes(plain200):
    g = synth.make_pose_graph(220, 560, seed=4)
    old = (g["edges"][:, 0] < 200) & (g["edges"][:, 1] < 200)
    first = dict(init=g["init"][:200], edges=g["edges"][old], z=g["z"][old], cov=g["cov"][old])
    sol = make_solver(first)
    sol.ComputeCovarianceColumns([3])
    for i in range(200, 220):
        sol.AddNode(i, g["init"][i])
    sol._ids = list(range(220))
    for e in np.flatnonzero(~old):
        sol.AddConstraint(int(g["edges"][e, 0]), int(g["edges"][e, 1]), g["z"][e], g["cov"][e])
    summ = sol.Compute()
    assert summ["usable"] == 1 and summ["analysis"] == 2, summ
    order = np.concatenate([np.flatnonzero(old), np.flatnonzero(~old)])
    check_variant(sol, dict(g, edges=g["edges"][order], z=g["z"][order], cov=g["cov"][order]), plain200[1], "220/560 after an incremental analysis")
    assert sol.cov_columns_summary["cov"]["analysis"] == 0
    sol.close()


# ---- joint and relative ------------------------------------------------------------------------------------------------------
def test_joint_any_and_relative_covariances(g200, plain200):
    tol = plain200[1]
    sol = make_solver(g200)
    r = rule_at(sol, g200)
    have = {(int(a), int(b)) for a, b in g200["edges"]} | {(int(b), int(a)) for a, b in g200["edges"]}
    ref = 17
    far = next(b for b in range(199, 0, -1) if (ref, b) not in have)
    linked = next(b for a, b in sorted(have) if a == ref and b not in (0, 60))
    assert far not in (ref, 60)
    sol.ComputeCovarianceColumns([ref, 60])
    scale = ccr.scales(r.sigma)
    for a, b in ((ref, far), (far, ref), (ref, linked), (linked, ref), (ref, 60), (60, ref)):
        j = sol.JointCovarianceAny(a, b)
        assert np.array_equal(j, j.T), "the joint covariance is not bit-wise symmetric"
        assert np.array_equal(j[:3, :3], sol.Covariance(a)) and np.array_equal(j[3:, 3:], sol.Covariance(b))
        ca, cb = r.problem.col_of[a], r.problem.col_of[b]
        e = float(np.sqrt(np.sum((j[:3, 3:] - ccr.blocks(r.sigma, [ca], cb)[0]) ** 2)) / np.sqrt(scale[ca] * scale[cb]))
        print(f"[covariance columns] joint ({a}, {b}): cross block {e:.3e}, bound {tol:.3e}")
        assert e <= tol
    # a pair WITH a constraint: the column's cross block against the selected inverse's
    on_pattern = sol.JointCovariance(ref, linked)
    d = sol.JointCovarianceAny(ref, linked) - on_pattern
    cr_, cl = r.problem.col_of[ref], r.problem.col_of[linked]
    e = float(np.sqrt(np.sum(d[:3, 3:] ** 2)) / np.sqrt(scale[cr_] * scale[cl]))
    print(f"[covariance columns] joint ({ref}, {linked}) against JointCovariance: {e:.3e}, bound {tol:.3e}")
    assert e <= tol and np.array_equal(d[:3, :3], np.zeros((3, 3))) and np.array_equal(d[3:, 3:], np.zeros((3, 3)))
    # off the pattern the selected inverse still has nothing; neither node a query: nothing either
    raises(capi.KH_ERR_NOT_FOUND, sol.JointCovariance, ref, far, text="pattern")
    raises(capi.KH_ERR_NOT_FOUND, sol.JointCovarianceAny, far, linked)
    # the kernel against the host's first-order rule on the same joint blocks: the project's rounding floor carried through the
    # two 3 x 6 products
    ids, poses = sol.node_arrays()
    pose_of = {int(i): p for i, p in zip(ids, poses)}
    listed = [0, ref, far, linked, 60, 199, 1]
    rel = sol.RelativeCovariances(ref, listed)
    worst = 0.0
    for k, i in enumerate(listed):
        joint = sol.JointCovarianceAny(ref, i)
        want = relative_covariance(pose_of[ref], pose_of[i], joint)
        jac = np.zeros((3, 6))
        cth, sth = np.cos(pose_of[ref][2]), np.sin(pose_of[ref][2])
        dx, dy = pose_of[i][0] - pose_of[ref][0], pose_of[i][1] - pose_of[ref][1]
        jac[:, :3] = [[-cth, -sth, -sth * dx + cth * dy], [sth, -cth, -cth * dx - sth * dy], [0.0, 0.0, -1.0]]
        jac[:, 3:] = [[cth, sth, 0.0], [-sth, cth, 0.0], [0.0, 0.0, 1.0]]
        bound = 64.0 * cr.EPS * np.sum(jac * jac) * np.sqrt(np.sum(joint * joint))
        diff = float(np.sqrt(np.sum((rel[k] - want) ** 2)))
        worst = max(worst, diff / bound if bound > 0.0 else (0.0 if diff == 0.0 else np.inf))
        if i == ref:
            assert not rel[k].any(), "the reference against itself is not exact zeros"
    print(f"[covariance columns] RelativeCovariances({ref}): largest |got - host| / bound over {len(listed)} nodes {worst:.3e}")
    assert worst <= 1.0
    every = sol.RelativeCovariances(ref)
    assert every.shape == (200, 3, 3) and np.array_equal(every[listed], rel)
    sol.close()


# ---- neutral for what surrounds it -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("debug", [dict(), dict(gather_children=True), dict(extend_add_pass=True)], ids=["default", "bit 8", "bit 9"])
def test_column_pass_does_not_interfere_with_compute_or_the_marginals(g200, debug):
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
            sol.ComputeCovarianceColumns(list(range(1, 30)))           # (with bit 0 the pass itself checks that the fronts are all zeros)
            assert np.isfinite(sol.CovarianceColumn(29)).all()
            with_columns = sol.Covariances().copy()
        sol.ComputeCovariances()
        sol.marginals = sol.Covariances().copy()
        if sol is b:
            assert with_columns.tobytes() == sol.marginals.tobytes()
            raises(capi.KH_ERR_NOT_FOUND, sol.CovarianceColumn, 29)     # a plain pass leaves no columns
        second = sol.Compute()
        assert second["usable"] == 1 and sol.last_warning == "", sol.last_warning
        sol.second = (second, sol.iteration_log().copy(), sol.poses().copy())
    assert a.marginals.tobytes() == b.marginals.tobytes()
    for ra, rb in ((a.first, b.first), (a.second, b.second)):
        assert [ra[0][k] for k in COUNTERS] == [rb[0][k] for k in COUNTERS]
        assert ra[1].tobytes() == rb[1].tobytes() and ra[2].tobytes() == rb[2].tobytes()
    assert a.second[0]["iterations"] >= 1
    a.close()
    b.close()


# ---- states ------------------------------------------------------------------------------------------------------------------
def test_getters_follow_the_state_of_the_graph(kartohip_lib):
    g = synth.make_pose_graph(12, 20, seed=2)
    sol = make_solver(g)
    getters = ((sol.CovarianceColumn, (3,)), (sol.JointCovarianceAny, (3, 5)), (sol.RelativeCovariances, (3,)))
    for fn, args in getters:
        raises(capi.KH_ERR_SOLVER, fn, *args, text="stale")                       # nothing computed yet
    sol.ComputeCovariances()
    raises(capi.KH_ERR_NOT_FOUND, sol.CovarianceColumn, 3, text="not a query")      # marginals only
    sol.ComputeCovarianceColumns([3])
    for fn, args in getters:
        fn(*args)
    raises(capi.KH_ERR_NOT_FOUND, sol.CovarianceColumn, 4, text="not a query")
    raises(capi.KH_ERR_NOT_FOUND, sol.RelativeCovariances, 4)
    raises(capi.KH_ERR_NOT_FOUND, sol.CovarianceColumn, 3, [99])
    raises(capi.KH_ERR_NOT_FOUND, sol.ComputeCovarianceColumns, [3, 99])
    for fn, args in getters:
        raises(capi.KH_ERR_SOLVER, fn, *args, text="stale")                       # a refused pass leaves nothing
    for change in (lambda: sol.ModifyNode(3, [0.0, 0.0, 0.0]), lambda: sol.AddNode(50, [0.0, 0.0, 0.0]), sol.Compute):
        sol.ComputeCovarianceColumns([3])
        sol.CovarianceColumn(3, [3])
        change()
        for fn, args in getters:
            raises(capi.KH_ERR_SOLVER, fn, *args, text="stale")
    sol.ComputeCovarianceColumns([3])
    raises(capi.KH_ERR_NOT_FOUND, sol.ComputeCovarianceColumns, [50], text="no constraints")
    raises(capi.KH_ERR_INVALID_ARG, sol.ComputeCovarianceColumns, [3, 4, 3], text="twice")
    raises(capi.KH_ERR_INVALID_ARG, sol.ComputeCovarianceColumns, [])
    sol.close()


def test_factor_mode_two_is_refused(kartohip_lib):
    sol = make_solver(synth.make_pose_graph(12, 20, seed=2), debug=dict(factor_kernels=2))
    raises(capi.KH_ERR_SOLVER, sol.ComputeCovarianceColumns, [3], text="level pipeline")
    raises(capi.KH_ERR_SOLVER, sol.CovarianceColumn, 3, text="stale")
    sol.set_debug()
    sol.ComputeCovarianceColumns([3])
    assert sol.CovarianceColumn(3, [3]).any()
    sol.close()


def test_component_not_tied_to_the_gauge_is_refused_and_the_handle_recovers(kartohip_lib):
    g = cr.chain(6)
    cut = np.array([0, 1, 3, 4])                                                   # 0-1-2 and 3-4-5
    parts = dict(init=g["init"], edges=g["edges"][cut], z=g["z"][cut], cov=g["cov"][cut])
    sol = make_solver(parts)
    raises(capi.KH_ERR_SOLVER, sol.ComputeCovarianceColumns, [1, 4], text="not tied to the gauge")
    raises(capi.KH_ERR_SOLVER, sol.CovarianceColumn, 1, text="stale")
    sol.AddConstraint(2, 3, g["z"][2], g["cov"][2])
    assert sol.Compute()["usable"] == 1
    order = np.array([0, 1, 3, 4, 2])
    gg = dict(g, edges=g["edges"][order], z=g["z"][order], cov=g["cov"][order])
    r = rule_at(sol, gg)
    err, _ = ccr.ref_err(r, [0, 3])
    sol.ComputeCovarianceColumns([1, 4])
    worst = worst_error(r, columns_of(sol, r, [1, 4]))
    print(f"[covariance columns] chain of 6, repaired: worst block {worst:.3e}, bound {cr.tolerance(err):.3e}")
    assert worst <= cr.tolerance(err)
    sol.close()


# ---- mapper ------------------------------------------------------------------------------------------------------------------
def test_mapper_relative_covariances_are_the_solvers_and_lazy(kartohip_lib):
    from slam_toolbox_amd.mapper import Mapper
    n_scans = 40
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_scans + 5)
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
    ref = int(ids[n // 2])
    every = m.relative_covariances(ref)
    assert m.cov_columns_summary["total_ms"] > 0.0 and m.cov_columns_summary["n_queries"] == 1 and m.cov_columns_summary["cov"]["n_free"] == n - 1
    own = np.zeros((n, 3, 3))
    assert L.kh_spa_get_relative_covariances(solver, ref, n, None, own.ctypes.data_as(C.c_void_p)) == capi.KH_OK
    assert np.array_equal(every, own) and np.isfinite(every).all() and not every[n // 2].any()
    assert all(np.linalg.eigvalsh(0.5 * (c + c.T)).min() > 0.0 for k, c in enumerate(every) if k != n // 2)
    some = m.relative_covariances(ref, ids[[3, 1, n - 1]])
    s = m.cov_columns_summary
    assert s["total_ms"] == 0.0 and s["n_queries"] == 0 and s["path_fronts"] == 0 and s["column_flops"] == 0 and s["cov"]["n_free"] == 0
    assert np.array_equal(some, own[[3, 1, n - 1]])                               # answered from the resident column
    for i in range(n_scans, n_scans + 5):                                          # until a scan is taken: the graph has changed
        m.Process(synth.make_scan(world, truth[i], rng), odom[i], 0.1 * i)
        if L.kh_spa_num_nodes(solver) > n:
            break
    assert L.kh_spa_num_nodes(solver) > n
    m.relative_covariances(ref, ids[[3]])
    assert m.cov_columns_summary["total_ms"] > 0.0 and m.cov_columns_summary["n_queries"] == 1
    m.close()
