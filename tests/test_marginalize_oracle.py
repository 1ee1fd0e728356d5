"""CPU: the marginalization rule of tests/marginalize_rule.py on its own, judged by the covariances of tests/covariance_rule.py.

The graphs are CONSISTENT (z computed from the poses, so the linearisation point is exact), 9 to 30 nodes, random SPD covariances.
  - a degree-2 node: the marginal of every remaining node is unchanged, relative Frobenius error <= 1e-10, for the four ways its
    two constraints can be stored (the rule reaches about 1e-13; noise of 0.02 on z gives about 1e-3 from linearisation alone, and
    a wrong sign or a transposed Jacobian breaks the consistent case at that scale or worse);
  - a node of degree >= 3, with and without an existing constraint between the hub and a neighbour: conservative, the smallest
    eigenvalue of Sigma_after - Sigma_before is >= -1e-10 times the largest eigenvalue of Sigma_before for every remaining node;
  - every emitted information matrix is SPD, the number of components does not grow, a list is processed in list order."""
import numpy as np
import pytest

import covariance_rule as cr
import marginalize_rule as mr
from oracle import spa


def rel_pose(pa, pb):
    c, s = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, spa.normalize_angle(pb[2] - pa[2])])


def random_spd(rng):
    A = rng.normal(size=(3, 3))
    return A @ A.T * 0.01 + np.diag([0.004, 0.004, 0.001]) * rng.uniform(0.5, 2.0)


def graph(n, edges, seed):
    rng = np.random.default_rng(seed)
    poses = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-3, 3, n)])
    cons = [(a, b, rel_pose(poses[a], poses[b]), np.linalg.inv(random_spd(rng))) for a, b in edges]
    return poses, mr.make(cons)


def ring(n, chords=()):
    return [(i, (i + 1) % n) for i in range(n)] + list(chords)


def marginals(poses, cons, nodes):
    edges = np.array([(c[0], c[1]) for c in cons])
    z = np.array([c[2] for c in cons])
    U = np.array([spa.sqrt_information_from_upper([c[3][0, 0], c[3][0, 1], c[3][0, 2], c[3][1, 1], c[3][1, 2], c[3][2, 2]]) for c in cons])
    r = cr.rule(poses, edges, z, U=U, reference=False)
    return {n: cr.diag_block(r, n) for n in nodes}


def check_spd(cons):
    for a, b, z, O in cons:
        assert np.all(np.isfinite(z)) and np.array_equal(O, O.T)
        assert np.linalg.eigvalsh(O).min() > 0.0, (a, b)


@pytest.mark.parametrize("flip_first,flip_second", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_degree_two_is_the_exact_marginal(flip_first, flip_second, seed):
    n, v = 9, 4
    edges = ring(n, [(0, 6), (2, 7)])
    edges[3] = (4, 3) if flip_first else (3, 4)
    edges[4] = (5, 4) if flip_second else (4, 5)
    poses, cons = graph(n, edges, seed)
    rest = [k for k in range(1, n) if k != v]
    before = marginals(poses, cons, rest)
    info = mr.marginalize(cons, v)
    assert info["d"] == 2 and len(info["added"]) == 1 and not info["fused"] and len(cons) == len(edges) - 1
    check_spd(cons)
    after = marginals(poses, cons, rest)
    worst = max(cr.rel_fro(after[k], before[k]) for k in rest)
    print(f"[marginalize] degree 2, directions {flip_first}{flip_second}, seed {seed}: worst relative error {worst:.3e}")
    assert worst <= 1e-10


CONSERVATIVE = {
    # name: (nodes, edges, the node that leaves, its degree, constraints fused into existing ones at least)
    "degree 3": (12, ring(12, [(5, 9), (1, 7)]), 5, 3, 0),
    "degree 4, triangle edges": (12, ring(12, [(5, 9), (2, 5), (4, 6), (9, 6), (2, 4), (1, 7)]), 5, 4, 1),
    "degree 6 of 30": (30, ring(30, [(10, 3), (10, 17), (25, 10), (10, 28), (3, 17), (11, 9), (4, 20)]), 10, 6, 0),
    "parallel constraints": (9, ring(9, [(4, 3), (4, 7), (7, 4), (5, 4)]), 4, 3, 0),
}


@pytest.mark.parametrize("name", list(CONSERVATIVE))
@pytest.mark.parametrize("seed", [1, 2])
def test_higher_degree_is_conservative(name, seed):
    n, edges, v, degree, min_fused = CONSERVATIVE[name]
    poses, cons = graph(n, edges, seed)
    rest = [k for k in range(1, n) if k != v]
    before = marginals(poses, cons, rest)
    comps = mr.components(cons, rest)
    info = mr.marginalize(cons, v)
    assert info["d"] == degree and len(info["added"]) + len(info["fused"]) == degree - 1 and len(info["fused"]) >= min_fused
    assert all(v not in (c[0], c[1]) for c in cons)
    check_spd(cons)
    assert mr.components(cons, rest) <= comps
    after = marginals(poses, cons, rest)
    worst = min(np.linalg.eigvalsh(after[k] - before[k]).min() / np.linalg.eigvalsh(before[k]).max() for k in rest)
    print(f"[marginalize] {name}, seed {seed}: smallest eigenvalue of the growth, relative: {worst:.3e}")
    assert worst >= -1e-10


def test_hub_is_the_largest_determinant_and_ties_go_to_the_lowest_id():
    poses, cons = graph(9, [(4, 7), (4, 2), (4, 6), (0, 2), (0, 6), (0, 7), (0, 1), (1, 3), (3, 5), (5, 8), (8, 0)], 5)
    for k in range(3):
        cons[k][3] = cons[0][3].copy()
    assert mr.marginalize([list(c) for c in cons], 4)["hub"] == 2
    cons[2][3] = cons[2][3] * 1.5
    assert mr.marginalize([list(c) for c in cons], 4)["hub"] == 6


def test_leaf_and_lone_node_transfer_nothing():
    poses, cons = graph(9, [(0, 1), (1, 2), (2, 3), (5, 6)], 7)
    before = [(c[0], c[1]) for c in cons]
    assert mr.marginalize(cons, 3)["d"] == 1 and [(c[0], c[1]) for c in cons] == before[:2] + before[3:]
    assert mr.marginalize(cons, 8)["d"] == 0 and len(cons) == 3


def test_a_list_is_processed_in_order():
    n = 9
    poses, cons = graph(n, ring(n, [(0, 5)]), 9)
    by_hand = [list(c) for c in cons]
    first = mr.marginalize(by_hand, 3)
    second = mr.marginalize(by_hand, 4)
    assert first["d"] == 2 and second["d"] == 2          # 4's second constraint is the one 3 left behind
    both = [list(c) for c in cons]
    mr.marginalize_list(both, [3, 4])
    other = [list(c) for c in cons]
    mr.marginalize_list(other, [4, 3])
    assert [(c[0], c[1]) for c in both] == [(c[0], c[1]) for c in by_hand]
    assert all(np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) for a, b in zip(both, by_hand))
    # (the other order composes through the other node first: the same graph to first order, not the same numbers)
    assert any(not np.array_equal(a[3], b[3]) for a, b in zip(both, other) if (a[0], a[1]) == (b[0], b[1])) or \
        [(c[0], c[1]) for c in both] != [(c[0], c[1]) for c in other]
    rest = [k for k in range(1, n) if k not in (3, 4)]
    assert mr.components(both, rest) == 1
    check_spd(both)
    # two exact steps are exact
    before, after = marginals(poses, cons, rest), marginals(poses, both, rest)
    assert max(cr.rel_fro(after[k], before[k]) for k in rest) <= 1e-10


def test_long_double_restatement_agrees():
    poses, cons = graph(12, ring(12, [(5, 9), (2, 5), (4, 6), (9, 6)]), 3)
    ld = mr.make(cons, dtype=mr.LD)
    mr.marginalize_list(cons, [5, 8])
    mr.marginalize_list(ld, [5, 8])
    err = mr.ref_err(cons, ld)
    print(f"[marginalize] float64 against long double: {err:.3e}")
    assert err < 1e-12 and all(c[3].dtype == mr.LD for c in ld)
