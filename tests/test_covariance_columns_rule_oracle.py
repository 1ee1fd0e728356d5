"""CPU: the rule of the covariance columns (tests/covariance_columns_rule.py) against what is known without it: a column of the
inverse solves H X = E_q; rule (a) stays within the project's bound of rule (b) in the Cauchy-Schwarz measure; along an OPEN chain at
consistent poses the relative covariance of two nodes (scan_solver.relative_covariance of their joint block, constraint or none) is
the odometry between them compounded (marginalize_rule.compose, w = 1); closing the chain shrinks the relative covariance of its
two ends."""
import numpy as np
import pytest

import covariance_columns_rule as ccr
import covariance_rule as cr
import marginalize_rule as mr
from oracle import spa
from slam_toolbox_amd import synth
from slam_toolbox_amd.scan_solver import relative_covariance

CASES = {
    "12/20": lambda: synth.make_pose_graph(12, 20, seed=2),
    "complete 60": lambda: cr.complete_graph(60),
    "60/120": lambda: synth.make_pose_graph(60, 120, seed=4),
}


@pytest.mark.parametrize("name", list(CASES))
def test_columns_of_rule_a_within_the_bound_of_rule_b_and_of_a_solve(name):
    g = CASES[name]()
    r = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"], reference=False)
    n = r.problem.nfree
    queries = [0, n // 2, n - 1]
    err, _ = ccr.ref_err(r, queries)
    tol = cr.tolerance(err)
    scale = ccr.scales(r.sigma)
    worst = 0.0
    for q in queries:
        e = np.zeros((3 * n, 3))
        e[3 * q:3 * q + 3] = np.eye(3)
        x = np.linalg.solve(r.H, e)
        solved = np.stack([x[3 * i:3 * i + 3] for i in range(n)])
        worst = max(worst, ccr.column_error(ccr.blocks(r.sigma, range(n), q), solved, scale, q))
    print(f"[covariance columns rule] {name}: ref_err {err:.3e}, (a) against np.linalg.solve {worst:.3e}, bound {tol:.3e}")
    assert 0.0 <= err < 1e-9
    assert worst <= tol, (name, worst, tol)


def curved_chain(n, closed=False):
    """n poses along an arc, every odometry constraint the exact difference of its two poses (zero residuals), one full 3 x 3
    covariance for all of them; `closed` adds the exact constraint from the last pose back to the first"""
    poses = np.zeros((n, 3))
    for i in range(1, n):
        th = poses[i - 1, 2]
        step = np.array([0.9 + 0.03 * i, 0.12 - 0.02 * i, 0.21 - 0.015 * i])
        poses[i] = [poses[i - 1, 0] + np.cos(th) * step[0] - np.sin(th) * step[1],
                    poses[i - 1, 1] + np.sin(th) * step[0] + np.cos(th) * step[1], th + step[2]]
    edges = [(i, i + 1) for i in range(n - 1)] + ([(n - 1, 0)] if closed else [])
    z = np.array([np.asarray(spa.link_info(poses[a], poses[b], np.eye(3))[0]) for a, b in edges])
    sigma = np.array([[0.012, 0.003, -0.001], [0.003, 0.008, 0.0015], [-0.001, 0.0015, 0.002]])
    cov = np.tile(sigma.reshape(1, 9), (len(edges), 1))
    return dict(init=poses, edges=np.array(edges), z=z, cov=cov), sigma


def test_relative_covariance_along_an_open_chain_is_the_compounded_odometry():
    n = 12
    g, sigma = curved_chain(n)
    r = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"], reference=False)
    worst = 0.0
    for a in range(n - 1):
        z, s = g["z"][a].copy(), sigma.copy()
        for b in range(a + 1, n):
            if b > a + 1:
                z, s = mr.compose(z, s, g["z"][b - 1].copy(), sigma.copy(), 1)
            got = relative_covariance(g["init"][a], g["init"][b], ccr.joint_any(r, a, b))
            worst = max(worst, cr.rel_fro(got, s))
    print(f"[covariance columns rule] open chain of {n}: relative covariance against compounded odometry {worst:.3e}")
    # exact to first order at consistent poses; 1e-10 is the bound of test_marginalize_oracle.py's exactness check
    assert worst <= 1e-10, worst


def test_closing_the_chain_shrinks_the_relative_covariance_of_its_ends():
    n = 12
    g, _ = curved_chain(n)
    r_open = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"], reference=False)
    gc, _ = curved_chain(n, closed=True)
    r_closed = cr.rule(gc["init"], gc["edges"], gc["z"], cov=gc["cov"], reference=False)
    # node 1 against node n - 1: no constraint joins them in either graph (the gauge, node 0, sits between them in the closed one)
    open_ = relative_covariance(g["init"][1], g["init"][n - 1], ccr.joint_any(r_open, 1, n - 1))
    closed = relative_covariance(gc["init"][1], gc["init"][n - 1], ccr.joint_any(r_closed, 1, n - 1))
    print(f"[covariance columns rule] trace of the ends' relative covariance: open {np.trace(open_):.4e}, closed {np.trace(closed):.4e}")
    assert np.trace(closed) < np.trace(open_)
    assert np.linalg.eigvalsh(0.5 * (open_ + open_.T) - 0.5 * (closed + closed.T)).min() > 0.0
