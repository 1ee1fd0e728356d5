"""CPU: the covariance rule (tests/covariance_rule.py) against what is known about (J^T J)^-1 without it -- numpy's general
inverse, symmetry and positive definiteness of every block, the closed form of the two-node graph, and how the uncertainty behaves
along an open chain and when the chain is closed.  Also scan_solver.relative_covariance (plain numpy) against central differences."""
import numpy as np
import pytest

import covariance_rule as cr
from oracle import spa
from slam_toolbox_amd import synth

CASES = {
    "2/1": lambda: cr.chain(2),
    "12/11": lambda: synth.make_pose_graph(12, 11, seed=2),
    "12/20": lambda: synth.make_pose_graph(12, 20, seed=2),
    "60/120": lambda: synth.make_pose_graph(60, 120, seed=4),
}


@pytest.fixture(scope="module", params=list(CASES))
def ruled(request):
    g = CASES[request.param]()
    return g, cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"])


def test_float64_route_agrees_with_numpy_inverse(ruled):
    _, r = ruled
    inv = np.linalg.inv(r.H)
    # both are float64 inverses of the same matrix: they differ by the conditioning of H times eps; 1e-9 relative to the largest
    # entry leaves four digits over the 4.9e-12 measured on the 60 / 120 graph
    assert np.abs(r.sigma - inv).max() <= 1e-9 * np.abs(inv).max()
    assert np.abs(r.sigma @ r.H - np.eye(r.H.shape[0])).max() < 1e-7


def test_longdouble_route_bounds_the_float64_error(ruled):
    _, r = ruled
    err = cr.ref_err(r)
    print("ref_err", err)
    assert 0.0 <= err < 1e-9


def test_blocks_are_symmetric_and_positive_definite(ruled):
    g, r = ruled
    for node in r.problem.free_nodes:
        b = cr.diag_block(r, node)
        assert np.abs(b - b.T).max() <= 1e-12 * np.abs(b).max()
        assert np.linalg.eigvalsh(0.5 * (b + b.T)).min() > 0.0
    for a, b in g["edges"]:
        j = cr.joint_block(r, a, b)
        assert np.abs(j - j.T).max() <= 1e-12 * np.abs(j).max()
        if r.problem.col_of[a] >= 0 and r.problem.col_of[b] >= 0:
            assert np.linalg.eigvalsh(0.5 * (j + j.T)).min() > 0.0


def test_two_nodes_match_the_closed_form():
    g = cr.chain(2)
    g["init"][1] = [1.3, -0.4, 0.7]
    g["cov"][0] = np.array([[0.02, 0.004, 0.0], [0.004, 0.01, 0.001], [0.0, 0.001, 0.003]]).reshape(9)
    r = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"])
    U = spa.sqrt_information(g["cov"][0].reshape(3, 3))
    _, (c, s, dx, dy) = spa._residuals(g["init"], g["edges"][:, 0], g["edges"][:, 1], g["z"], U[None])
    _, Jb = spa._jacobians(c, s, dx, dy, U[None])
    want = np.linalg.inv(Jb[0].T @ Jb[0])                       # (Jb^T U^T U Jb)^-1 with U folded into the Jacobian
    assert cr.rel_fro(cr.diag_block(r, 1), want) < 1e-12
    assert not cr.diag_block(r, 0).any()


def test_trace_grows_along_an_open_chain_and_drops_when_it_closes():
    n = 12
    g = cr.chain(n)
    r_open = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"])
    tr_open = np.array([np.trace(cr.diag_block(r_open, i)) for i in range(n)])
    assert tr_open[0] == 0.0 and np.all(np.diff(tr_open) > 0.0)
    g = cr.chain(n, closed=True)
    r_closed = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"])
    tr_closed = np.array([np.trace(cr.diag_block(r_closed, i)) for i in range(n)])
    assert tr_closed[1] < tr_open[1] and tr_closed[n - 1] < tr_open[n - 1]
    assert np.all(tr_closed[1:] < tr_open[1:])


def test_gauge_row_is_absent():
    g = synth.make_pose_graph(12, 20, seed=2)
    r = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"])
    assert r.problem.col_of[0] == -1 and r.sigma.shape == (3 * 11, 3 * 11)
    assert 0 not in r.problem.free_nodes
    assert not cr.diag_block(r, 0).any() and not cr.cross_block(r, 0, 1).any()


def test_relative_covariance_is_the_first_order_rule():
    from slam_toolbox_amd.scan_solver import relative_covariance
    rng = np.random.default_rng(8)
    a, b = np.array([1.0, -2.0, 0.8]), np.array([2.5, 0.5, -1.1])
    m = rng.normal(size=(6, 6))
    joint = m @ m.T * 1e-3

    def rel(p):
        d, _ = spa.link_info(p[:3], p[3:], np.eye(3))          # b in a's frame (LinkInfo::Update)
        return np.asarray(d)

    x = np.concatenate([a, b])
    jac = np.zeros((3, 6))
    for k in range(6):
        h = np.zeros(6)
        h[k] = 1e-6
        jac[:, k] = (rel(x + h) - rel(x - h)) / 2e-6
    want = jac @ joint @ jac.T
    got = relative_covariance(a, b, joint)
    # central differences with a step of 1e-6 leave about 1e-10 relative; 1e-7 keeps three digits of margin
    assert cr.rel_fro(got, want) < 1e-7 and np.array_equal(got.shape, (3, 3))
    # the gauge as a: its rows and columns are zero, what is left is b's marginal turned into a's frame
    sb = joint[3:, 3:]
    only_b = np.zeros((6, 6))
    only_b[3:, 3:] = sb
    c, s = np.cos(a[2]), np.sin(a[2])
    r = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    assert cr.rel_fro(relative_covariance(a, b, only_b), r @ sb @ r.T) < 1e-14
