"""GPU: the edge-case table of tests/spa_cases.py through the HIP pose-graph solver, next to oracle/spa.py (the CPU side of the same
table: tests/test_edge_cases_oracle.py for the edges, tests/test_spa_oracle.py for the second reference, the decision margins and
the tolerances used here -- see the header of tests/spa_cases.py for the figures).

Every case runs with factor_kernels=3 (the level pipeline: k_potrf / k_trsm / k_syrk / k_front_update -- this is the DEFAULT route,
kh_spa_set_debug's 0 means 3) and with factor_kernels=2 (the panel-pair kernel k_factor)."""
import ctypes as C

import numpy as np
import pytest

import spa_cases as sc
from test_spa_gpu import POSE_TOL, _diff
from test_spa_oracle import step_error

pytestmark = pytest.mark.gpu

SPA = list(sc.all_cases())
FAIL = list(sc.failure_cases())
ROUTES = (3, 2)
TERMINATION = {"CONVERGENCE": 0, "NO_CONVERGENCE": 1, "FAILURE": 2}


def answers(case):
    return sc.split(case)[1]


def load(sol, case):
    """AddNode / AddConstraint[Information] in the case's order; every return code must be what the arguments alone say"""
    from slam_toolbox_amd import capi
    L = capi.lib()
    want = {"ok": capi.KH_OK, "not_found": capi.KH_ERR_NOT_FOUND, "invalid": capi.KH_ERR_INVALID_ARG}
    sol.Reset()
    sol._ids = []
    for i, p in case.nodes:
        sol.AddNode(i, p)
        sol._ids.append(i)
    n_ok = 0
    for (a, b, z, w), ans in zip(case.cons, answers(case)):
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        z = np.ascontiguousarray(z, dtype=np.float64)
        before = (L.kh_spa_num_nodes(sol._h), L.kh_spa_num_constraints(sol._h))
        fn = L.kh_spa_add_constraint if w.size == 9 else L.kh_spa_add_constraint_information
        rc = fn(sol._h, int(a), int(b), z, w)
        assert rc == want[ans], (case.name, a, b, rc, ans)
        n_ok += ans == "ok"
        assert (L.kh_spa_num_nodes(sol._h), L.kh_spa_num_constraints(sol._h)) == (before[0], before[1] + (ans == "ok"))
    assert L.kh_spa_num_constraints(sol._h) == n_ok


def compute(sol, case, route):
    sol.set_debug(check_linear_solves=True, factor_kernels=route)
    sol.Configure({})                     # back to the defaults: the handle may come from another case
    sol.Configure(dict(case.options))
    load(sol, case)
    summ = sol.Compute()
    return summ, sol.node_arrays()[1].copy(), sol.iteration_log().copy()


def fresh(case, route):
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    sol = HipSpaSolver()
    out = compute(sol, case, route)
    sol.close()
    return out


def close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


def compare_rows(log, ref, tol, name):
    assert log.shape == ref.shape, (name, log[:, 7], ref[:, 7])
    assert np.array_equal(log[:, 0], ref[:, 0]) and np.array_equal(log[:, 7], ref[:, 7]), (name, log[:, 7], ref[:, 7])
    for row, want in zip(log, ref):
        cols = (1, 4, 5) if want[7] == -1.0 else (1, 2, 3, 4, 5, 6)          # an invalid step has no candidate
        for q in cols:
            print(f"{name}: row {int(want[0])} column {q}: {row[q]!r} oracle {want[q]!r}")
            assert close(row[q], want[q], tol), (name, int(want[0]), q, row[q], want[q])


@pytest.fixture(scope="module")
def oracle_runs():
    return {c.name: sc.oracle_run(c) for c in SPA}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", sc.modes(SPA, "zero"), ids=lambda c: c.name)
def test_zero_cases_initial_cost(kartohip_lib, oracle_runs, case, route):
    ref = oracle_runs[case.name]
    summ, x, log = fresh(case, route)
    print(f"{case.name}: initial_cost {summ['initial_cost']!r} oracle {ref.info['initial_cost']!r}")
    assert summ["usable"] == 1 and summ["iterations"] == 0 and summ["termination"] == 0 and len(log) == 0
    assert close(summ["initial_cost"], ref.info["initial_cost"], sc.COST_TOL)
    assert np.array_equal(x.view(np.uint64), ref.x0.view(np.uint64)), "nothing moves at iteration 0"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", sc.modes(SPA, "one"), ids=lambda c: c.name)
def test_one_cases_step_and_log_row(kartohip_lib, oracle_runs, case, route):
    ref = oracle_runs[case.name]
    summ, x, log = fresh(case, route)
    assert summ["usable"] == 1 and summ["iterations"] == 1
    assert summ["termination"] == TERMINATION[ref.info["termination"]] and summ["successful_steps"] == ref.info["successful_steps"]
    assert close(summ["initial_cost"], ref.info["initial_cost"], sc.COST_TOL)
    compare_rows(log, ref.info["log"], sc.STEP_TOL, case.name)
    assert 0.0 < summ["worst_linear_residual"] < 1e-9, summ
    moved = not np.array_equal(ref.x, ref.x0)
    assert np.array_equal(x, ref.x0) == (not moved)
    if moved:
        err = step_error(ref.x0, x, ref.x)
        print(f"{case.name}: step error {err:.3e}")
        assert err <= sc.STEP_TOL
    assert np.array_equal(np.isfinite(x), np.isfinite(ref.x0))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", sc.modes(SPA, "run"), ids=lambda c: c.name)
def test_run_cases_log_row_by_row(kartohip_lib, oracle_runs, case, route):
    ref = oracle_runs[case.name]
    la = ref.info["log"]
    tol = sc.run_tol(case.name)              # 8 x this case's own order_err (tests/test_spa_oracle.py holds the figure to the table)
    summ, x, log = fresh(case, route)
    print(f"{case.name}: tolerance {tol:.3e}, summary {summ}")
    assert summ["usable"] == 1 and summ["iterations"] == ref.info["iterations"], (summ, ref.info["iterations"], log[:, 7], la[:, 7])
    assert summ["successful_steps"] == ref.info["successful_steps"] and summ["termination"] == TERMINATION[ref.info["termination"]]
    compare_rows(log, la, tol, case.name)
    assert _diff(x, ref.x) < POSE_TOL
    assert close(summ["final_cost"], ref.info["final_cost"], tol) or summ["final_cost"] == ref.info["final_cost"]


def rejected_graph():
    return next(c for c in SPA if c.name.startswith("rejected:"))


def test_rejected_constraints_leave_the_solve_unchanged(kartohip_lib):
    """the solve after KH_ERR_INVALID_ARG / KH_ERR_NOT_FOUND answers equals, bit for bit, the solve of the graph without those calls"""
    case = rejected_graph()
    clean = case._replace(cons=[c for c, a in zip(case.cons, answers(case)) if a == "ok"])
    assert len(clean.cons) < len(case.cons)
    (sa, xa, la), (sb, xb, lb) = fresh(case, 3), fresh(clean, 3)
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)) and np.array_equal(la, lb) and sa["final_cost"] == sb["final_cost"]


@pytest.mark.parametrize("options", sc.REJECTED_OPTIONS, ids=lambda o: f"{o['loss_function']} {o['loss_scale']}")
def test_invalid_loss_scale_is_rejected_and_the_handle_stays_usable(kartohip_lib, options):
    from slam_toolbox_amd import capi
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    case = next(c for c in SPA if c.name == sc.REJECTED_OPTIONS_GRAPH)
    sol = HipSpaSolver()
    sol.Configure({**case.options, **options})
    load(sol, case)
    before = sol.node_arrays()[1].copy()
    s = capi.KhSpaSummary()
    assert capi.lib().kh_spa_compute(sol._h, C.byref(s)) == capi.KH_ERR_INVALID_ARG
    assert np.array_equal(sol.node_arrays()[1].view(np.uint64), before.view(np.uint64)) and sol.GetCorrections() == []
    # squared loss does not read the scale
    sol.Configure({**case.options, **sc.ACCEPTED_OPTIONS})
    assert sol.Compute()["usable"] == 1
    got = compute(sol, case, 3)
    want = fresh(case, 3)
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)) and np.array_equal(got[2], want[2])
    sol.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case,repair", FAIL, ids=lambda v: v.name if isinstance(v, sc.Case) else "")
def test_failure_exits_keep_the_old_state(kartohip_lib, case, repair, route):
    """usable == 0, termination == 2, KH_ERR_SOLVER and the plugin's warning; poses and corrections untouched bit for bit; the same
    handle solves again once the input is repaired.  (`iterations` is compared only where the failure comes from three invalid
    steps: a cost that is not finite ends the library at iteration zero, as in Ceres, while the oracle goes on to count steps.)"""
    from slam_toolbox_amd import capi
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    good = next(c for c in SPA if c.name == "topology: pairs doubled as (a, b) twice and as (a, b) + (b, a), three parallel constraints [one]")
    sol = HipSpaSolver()
    first = compute(sol, good, route)               # (the handle has solved before: buffers, analysis and log of another graph)
    sol.set_debug(factor_kernels=route)
    sol.Configure({})
    sol.Configure(dict(case.options))
    load(sol, case)
    before = sol.node_arrays()[1].copy()
    corr = sol.GetCorrections()                     # (empty: loading the case went through Reset)
    s = capi.KhSpaSummary()
    rc = capi.lib().kh_spa_compute(sol._h, C.byref(s))
    assert rc == capi.KH_ERR_SOLVER and s.usable == 0 and s.termination == 2
    sol.last_warning = ""
    summ = sol.Compute()
    assert summ["usable"] == 0 and "could not find a usable solution" in sol.last_warning
    if "three invalid steps" in case.name:
        log = sol.iteration_log()
        assert summ["iterations"] == 3 and np.array_equal(log[:, 7], [-1.0, -1.0, -1.0])
        assert np.array_equal(log[:, 4], sc.oracle_run(case).info["log"][:, 4])
    after = sol.node_arrays()[1]
    assert np.array_equal(after.view(np.uint64), before.view(np.uint64))
    now = sol.GetCorrections()
    assert [i for i, _ in now] == [i for i, _ in corr] and all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for (_, p), (_, q) in zip(now, corr))
    # repair and solve on the same handle: equal to a fresh solver's answer
    if repair is not None:
        i, pose = repair
        stored = dict(case.nodes)[i]
        sol.ModifyNode(i, [pose[0], pose[1], pose[2] - stored[2]])          # ModifyNode adds the stored yaw
        fixed = case._replace(nodes=[(k, (np.array([pose[0], pose[1], (pose[2] - stored[2]) + stored[2]]) if k == i else p)) for k, p in case.nodes])
        summ = sol.Compute()
        got = (summ, sol.node_arrays()[1].copy(), sol.iteration_log().copy())
    else:
        fixed = case._replace(options={}, cons=[c for c in good.cons], nodes=good.nodes)
        got = compute(sol, fixed, route)
    want = fresh(fixed, route)
    assert got[0]["usable"] == 1 and got[0]["iterations"] == want[0]["iterations"] > 0
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)) and np.array_equal(got[2], want[2])
    assert first[0]["usable"] == 1
    sol.close()


@pytest.mark.parametrize("route", ROUTES)
def test_one_handle_across_a_run_a_failure_and_a_launch_shape(kartohip_lib, route):
    """the fail word, reuse_diagonal, the step evaluator's state and the decrease factor belong to one Compute(): a run with rejected
    steps, then three invalid steps, then a launch-shape case on ONE handle, each equal to a fresh handle's answer bit for bit"""
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    names = {c.name: c for c in SPA + [c for c, _ in FAIL]}
    seq = [names[n] for n in sc.REUSE_SEQUENCE]
    sol = HipSpaSolver()
    for case in seq:
        got, want = compute(sol, case, route), fresh(case, route)
        assert got[0]["usable"] == want[0]["usable"] and got[0]["iterations"] == want[0]["iterations"], (case.name, got[0], want[0])
        assert np.array_equal(got[2], want[2], equal_nan=True), case.name
        assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), case.name
    sol.close()
