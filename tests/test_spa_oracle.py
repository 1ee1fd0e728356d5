"""CPU: independent checks of the SPA oracle (oracle/spa.py).  The Ceres boundary is "parity unpinned"
(Ceres is not in the reference tree); what can be pinned is pinned here: LinkInfo::Update and
Matrix3::Inverse against known answers from the reference build, the optimum against scipy's generic
least-squares, and noise-free graphs against their ground truth."""
import os

import numpy as np
import pytest

from oracle import spa
from slam_toolbox_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "link_info.npz")


def _diff(a, b):
    d = np.asarray(a) - np.asarray(b)
    d[:, 2] = (d[:, 2] + np.pi) % (2 * np.pi) - np.pi
    return float(np.abs(d).max())


def test_link_info_and_inverse_against_reference_known_answers():
    g = np.load(GOLD)
    for i in range(g["pose1"].shape[0]):
        d, c = spa.link_info(g["pose1"][i], g["pose2"][i], g["cov"][i])
        assert np.array_equal(d, g["diff"][i])
        assert np.array_equal(c, g["cov_out"][i])
        assert np.array_equal(spa.matrix3_inverse(g["cov_out"][i]), g["inverse"][i])


def test_tight_solution_is_the_least_squares_optimum():
    from scipy.optimize import least_squares
    g = synth.make_pose_graph(120, 260, seed=21)
    xt, info = spa.solve(g["init"], g["edges"], g["z"], g["cov"], spa.Options.tight())
    prob = spa.Problem(g["init"], g["edges"], g["z"], g["cov"])

    def fun(v):
        xx = g["init"].copy()
        xx[prob.free_nodes] = v.reshape(-1, 3)
        r, _ = spa._residuals(xx, prob.edges[:, 0], prob.edges[:, 1], prob.z, prob.U)
        return r.reshape(-1)
    res = least_squares(fun, g["init"][prob.free_nodes].reshape(-1), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    xs = g["init"].copy()
    xs[prob.free_nodes] = res.x.reshape(-1, 3)
    assert _diff(xs, xt) < 1e-6          # scipy's trf stops at ~1e-7; the costs agree to 1e-9 below
    assert abs(res.cost - info["final_cost"]) < 1e-9 * info["final_cost"]


def test_noise_free_graph_returns_ground_truth():
    g = synth.make_pose_graph(200, 450, seed=22)
    z = np.asarray([spa.link_info(g["truth"][a], g["truth"][b], np.eye(3))[0] for a, b in g["edges"]])
    x, info = spa.solve(g["init"], g["edges"], z, g["cov"], spa.Options.tight())
    assert _diff(x, g["truth"]) < 1e-9


def test_ceres_like_options_stop_early_and_gauge_is_fixed():
    g = synth.make_pose_graph(300, 700, seed=5)
    x, info = spa.solve(g["init"], g["edges"], g["z"], g["cov"])
    assert info["termination"] == "CONVERGENCE" and info["iterations"] < 50
    assert np.array_equal(x[0], g["init"][0])                 # first node constant (ceres_solver.cpp:228-241)
    assert info["final_cost"] < info["initial_cost"]


def _with_outliers(g, n_bad, seed):
    """Corrupt n_bad non-odometry constraints (false loop closures)."""
    rng = np.random.default_rng(seed)
    z = g["z"].copy()
    loops = np.flatnonzero(np.abs(g["edges"][:, 0] - g["edges"][:, 1]) > 1)
    bad = rng.choice(loops, size=min(n_bad, len(loops)), replace=False)
    z[bad, :2] += rng.normal(0, 1.5, (len(bad), 2))
    z[bad, 2] += rng.normal(0, 0.4, len(bad))
    return z, bad


@pytest.mark.parametrize("loss", ["HuberLoss", "CauchyLoss"])
def test_robust_loss_gradient_and_optimum(loss):
    """ceres_solver.cpp:82-94.  The corrected linearisation must be the gradient of 0.5 sum rho(|U r|^2)
    (checked by central differences, both branches of the loss active), the LM run must end at a stationary
    point of that cost, and false loop closures must pull the result less than under the squared loss."""
    g = synth.make_pose_graph(150, 330, seed=31)
    z, bad = _with_outliers(g, 12, seed=32)
    prob = spa.Problem(g["init"], g["edges"], z, g["cov"], loss=loss)
    r, _ = spa._residuals(g["init"], prob.edges[:, 0], prob.edges[:, 1], prob.z, prob.U)
    sq = np.sum(r * r, axis=1)
    assert (sq > 0.49).any() and (sq < 0.49).any()
    _, grad, H = prob.linearize(g["init"])
    g0 = np.abs(grad).max()
    rng = np.random.default_rng(1)
    for k in rng.choice(grad.size, 25, replace=False):
        d = np.zeros(grad.size); d[k] = 1e-6
        num = (prob.cost(prob.plus(g["init"], d)) - prob.cost(prob.plus(g["init"], -d))) / 2e-6
        assert abs(num - grad[k]) <= 1e-5 * max(1.0, abs(grad[k]))
    assert abs(H - H.T).max() < 1e-9
    opt = spa.Options.tight(); opt.loss_function = loss
    x, info = spa.solve(g["init"], g["edges"], z, g["cov"], opt)
    _, grad, _ = spa.Problem(x, g["edges"], z, g["cov"], loss=loss).linearize(x)
    assert np.abs(grad).max() < 1e-6 * g0     # Gauss-Newton on a robustified cost converges linearly
    x2, _ = spa.solve(g["init"], g["edges"], z, g["cov"], spa.Options.tight())
    err_robust = np.abs(x[:, :2] - g["truth"][:, :2]).max()
    err_square = np.abs(x2[:, :2] - g["truth"][:, :2]).max()
    assert err_robust < err_square


# ==== the edge-case table of tests/spa_cases.py: a second reference, decision margins, and the tolerances of the GPU side ==========
import spa_cases as sc      # noqa: E402

SPA = list(sc.all_cases())
LD = np.longdouble
PI_D, TWO_PI_D = LD(np.pi), LD(2.0 * np.pi)          # the float64 constants the solver uses, not 80-bit pi


def _ld_chol3(info):
    """upper factor U (U^T U = info) of a 3 x 3 float64 information matrix, in np.longdouble"""
    a = info.astype(LD)
    L = np.zeros((3, 3), dtype=LD)
    for j in range(3):
        d = a[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 3):
            v = a[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    return L.T


def _ld_information(w):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size == 6:
        return np.array([[w[0], w[1], w[2]], [w[1], w[3], w[4]], [w[2], w[4], w[5]]])
    p = spa.matrix3_inverse(w.reshape(3, 3))         # Karto's float64 operations are the definition of the information
    return np.array([[p[0, 0], p[0, 1], p[0, 2]], [p[0, 1], p[1, 1], p[1, 2]], [p[0, 2], p[1, 2], p[2, 2]]])


def _ld_wrap(a, a64):
    """normalize_angle in np.longdouble; the number of turns is the float64 evaluation's (at the cut the count is the case's
    subject and one rounding decides it: the GPU side compares it with the oracle, this reference only the arithmetic around it)"""
    return a - TWO_PI_D * LD(np.floor((a64 + np.pi) / (2.0 * np.pi)))


def ld_linearize(case, x):
    """cost, g, H (dense, over the free parameters) and the free nodes, every operation in np.longdouble, edge by edge"""
    acc, _ = sc.split(case)
    infos = [_ld_information(w) for (a, b, z, w), ans in zip(case.cons, sc.split(case)[1]) if ans == "ok"]
    n = x.shape[0]
    used = np.zeros(n, dtype=bool)
    for a, b, _, _ in acc:
        used[a] = used[b] = True
    free = [i for i in range(n) if used[i] and not (i == 0 and used[0])]
    col = {i: k for k, i in enumerate(free)}
    loss, scale = case.options.get("loss_function", "None"), LD(case.options.get("loss_scale", 0.7))
    g = np.zeros(3 * len(free), dtype=LD)
    H = np.zeros((3 * len(free), 3 * len(free)), dtype=LD)
    cost = LD(0.0)
    xl = x.astype(LD)
    for (a, b, z, _), info in zip(acc, infos):
        U = _ld_chol3(info)
        c, s = np.cos(xl[a, 2]), np.sin(xl[a, 2])
        dx, dy = xl[b, 0] - xl[a, 0], xl[b, 1] - xl[a, 1]
        zl = z.astype(LD)
        raw = [c * dx + s * dy - zl[0], -s * dx + c * dy - zl[1],
               _ld_wrap((xl[b, 2] - xl[a, 2]) - zl[2], (x[b, 2] - x[a, 2]) - z[2])]
        J = np.zeros((3, 6), dtype=LD)
        J[0] = [-c, -s, -s * dx + c * dy, c, s, 0.0]
        J[1] = [s, -c, -c * dx - s * dy, -s, c, 0.0]
        J[2] = [0.0, 0.0, -1.0, 0.0, 0.0, 1.0]
        f = np.zeros(3, dtype=LD)
        UJ = np.zeros((3, 6), dtype=LD)
        for i in range(3):
            for k in range(i, 3):
                f[i] = f[i] + U[i, k] * raw[k]
                for q in range(6):
                    UJ[i, q] = UJ[i, q] + U[i, k] * J[k, q]
        sq = f[0] * f[0] + f[1] * f[1] + f[2] * f[2]
        rho, w = sq, LD(1.0)
        if loss == "HuberLoss" and sq > scale * scale:
            rho, w = LD(2.0) * scale * np.sqrt(sq) - scale * scale, scale / np.sqrt(sq)
        elif loss == "CauchyLoss":
            tot = LD(1.0) + sq / (scale * scale)
            rho, w = scale * scale * np.log(tot), LD(1.0) / tot
        cost = cost + LD(0.5) * rho
        where = [3 * col[a] + q if a in col else -1 for q in range(3)] + [3 * col[b] + q if b in col else -1 for q in range(3)]
        for p in range(6):
            if where[p] < 0:
                continue
            for i in range(3):
                g[where[p]] = g[where[p]] + w * UJ[i, p] * f[i]
            for q in range(6):
                if where[q] < 0:
                    continue
                for i in range(3):
                    H[where[p], where[q]] = H[where[p], where[q]] + w * UJ[i, p] * UJ[i, q]
    return cost, g, H, free


def ld_step(case, x):
    """the first LM step in np.longdouble: Jacobi scale, clamped diagonal / radius, dense Cholesky, Plus -> the log row's numbers"""
    opt = sc.oracle_options(case.options)
    cost, g, H, free = ld_linearize(case, x)
    n3 = g.size
    scale = LD(1.0) / (LD(1.0) + np.sqrt(np.diag(H)))
    A = np.zeros_like(H)
    for i in range(n3):
        A[i] = scale[i] * H[i] * scale
    Hs = A.copy()
    gs = scale * g
    for i in range(n3):
        d = min(max(A[i, i], LD(opt.min_lm_diagonal)), LD(opt.max_lm_diagonal))
        A[i, i] = A[i, i] + d / LD(opt.initial_trust_region_radius)
    L = np.zeros_like(A)
    for j in range(n3):                           # column Cholesky
        d = A[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        L[j, j] = np.sqrt(d)
        if j + 1 < n3:
            v = A[j + 1:, j].copy()
            for k in range(j):
                v = v - L[j + 1:, k] * L[j, k]
            L[j + 1:, j] = v / L[j, j]
    y = gs.copy()
    for i in range(n3):
        for k in range(i):
            y[i] = y[i] - L[i, k] * y[k]
        y[i] = y[i] / L[i, i]
    for i in range(n3 - 1, -1, -1):
        for k in range(i + 1, n3):
            y[i] = y[i] - L[k, i] * y[k]
        y[i] = y[i] / L[i, i]
    step = -y
    sHs = LD(0.0)
    for i in range(n3):
        row = LD(0.0)
        for k in range(n3):
            row = row + Hs[i, k] * step[k]
        sHs = sHs + step[i] * row
    sg = LD(0.0)
    for i in range(n3):
        sg = sg + step[i] * gs[i]
    model = -(sg + LD(0.5) * sHs)
    delta = step * scale
    cand = x.astype(LD)
    for k, i in enumerate(free):
        cand[i, 0] = cand[i, 0] + delta[3 * k]
        cand[i, 1] = cand[i, 1] + delta[3 * k + 1]
        t = cand[i, 2] + delta[3 * k + 2]
        cand[i, 2] = t - TWO_PI_D * np.floor((t + PI_D) / TWO_PI_D)
    moved = (x.astype(LD) - cand)[free].reshape(-1)
    step_norm = np.sqrt(np.sum(moved * moved))
    cand64 = cand.astype(np.float64)
    cand_cost = ld_linearize(case, cand64)[0]       # (at the float64 rounding of the candidate, 1e-16 away)
    return dict(cost=cost, cand_cost=cand_cost, model=model, step_norm=step_norm, cand=cand, free=free)


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


def step_error(x0, xa, xb):
    """largest difference of two steps from x0, relative to the largest component of the step"""
    da, db = np.asarray(xa, dtype=np.float64) - x0, np.asarray(xb, dtype=np.float64) - x0
    for d in (da, db):
        d[:, 2] = (d[:, 2] + np.pi) % (2 * np.pi) - np.pi
    return float(np.abs(da - db).max() / max(np.abs(db).max(), 1e-300))


@pytest.fixture(scope="module")
def measured():
    """ref_err of cost and step over the zero / one cases, once for the tests below"""
    cost_err, step_err = {}, {}
    for c in SPA:
        if c.mode not in ("zero", "one"):
            continue
        run = sc.oracle_run(c)
        if c.mode == "zero":
            cost_err[c.name] = _rel(run.info["initial_cost"], ld_linearize(c, run.x0)[0])
            continue
        ref = ld_step(c, run.x0)
        row = run.info["log"][0]
        errs = [_rel(row[1], ref["cost"]), _rel(row[2], ref["cand_cost"]), _rel(row[3], ref["model"]), _rel(row[6], ref["step_norm"])]
        if row[7] == 1.0 and row[2] < row[1]:
            errs.append(step_error(run.x0, run.x, ref["cand"]))
        cost_err[c.name] = errs[0]
        step_err[c.name] = max(errs)
    return cost_err, step_err


def test_float64_oracle_agrees_with_the_longdouble_restatement(measured):
    cost_err, step_err = measured
    worst_cost, worst_step = max(cost_err, key=cost_err.get), max(step_err, key=step_err.get)
    print(f"ref_err cost {cost_err[worst_cost]:.3e} ({worst_cost}); step {step_err[worst_step]:.3e} ({worst_step})")
    assert len(cost_err) > 40 and len(step_err) > 20
    assert cost_err[worst_cost] <= sc.REF_ERR_COST, (worst_cost, cost_err[worst_cost])
    assert step_err[worst_step] <= sc.REF_ERR_STEP, (worst_step, step_err[worst_step])
    assert sc.COST_TOL == 1e-12 and sc.STEP_TOL == 8 * sc.REF_ERR_STEP > 64 * sc.EPS


@pytest.mark.parametrize("case", sc.modes(SPA, "run"), ids=lambda c: c.name)
def test_run_case_verdicts_do_not_depend_on_the_elimination_order(case):
    """every `run` case gives the same verdicts, iteration count and termination under two column orderings of the oracle's sparse
    factorisation, no step quality lies within 1e-6 relative of min_relative_decrease, and the rows differ by at most the case's
    own ORDER_ERR (from which sc.run_tol derives the bound of the GPU comparison)"""
    a, b = sc.oracle_run(case, "MMD_AT_PLUS_A"), sc.oracle_run(case, "COLAMD")
    assert a.info["iterations"] == b.info["iterations"] and a.info["termination"] == b.info["termination"]
    assert a.info["successful_steps"] == b.info["successful_steps"] and a.info["message"] == b.info["message"]
    la, lb = a.info["log"], b.info["log"]
    assert np.array_equal(la[:, 7], lb[:, 7]) and np.array_equal(la[:, 0], lb[:, 0])
    mrd = sc.oracle_options(case.options).min_relative_decrease
    for q in a.info["quality"] + b.info["quality"]:
        assert abs(q - mrd) > 1e-6 * mrd
    if len(la):
        err = np.abs(la[:, 1:7] - lb[:, 1:7]) / np.abs(lb[:, 1:7])
        print(f"order_err {err.max():.3e}")
        assert err.max() <= sc.ORDER_ERR[case.name], err.max(axis=0)
        assert err.max() >= 0.5 * sc.ORDER_ERR[case.name], "the recorded figure is stale: measure it again"
    else:
        assert sc.ORDER_ERR[case.name] == 0.0
    assert sc.run_tol(case.name) == max(8 * sc.ORDER_ERR[case.name], sc.STEP_TOL)
