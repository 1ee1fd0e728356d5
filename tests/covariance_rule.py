"""The rule the pose-graph covariances are pinned to (the reference never asks Ceres for a Covariance, so there is no reference
figure to compare with): Sigma = (J^T J)^-1 over the free nodes at the given poses, with J^T J = H as oracle.spa.Problem.linearize
builds it (loss reweighting included), restated densely two ways:

  (a) float64, the way the device does it: Jacobi scale, dense Cholesky, L^-T L^-1, unscale;
  (b) the same in np.longdouble with a hand-written dense Cholesky, as tests/test_spa_oracle.py does for the LM step.

ref_err(rule) is the largest relative Frobenius difference of a 3 x 3 block (diagonal blocks and the cross blocks of the edges)
between (a) and (b): the error float64 itself makes on the case, which the tolerance of the GPU tests is a multiple of (the
convention of tests/spa_cases.py).  Above LD_MAX_FREE free nodes (b) is too slow and (a) is laid against np.linalg.inv(H)."""
from collections import namedtuple

import numpy as np

from oracle import spa

LD = np.longdouble
EPS = 2.0 ** -52
LD_MAX_FREE = 200

Rule = namedtuple("Rule", "problem sigma sigma_ref H")       # sigma: (a); sigma_ref: (b), or np.linalg.inv(H) on large cases


def inverse_float64(H, jacobi=True):
    """(a)"""
    n3 = H.shape[0]
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H))) if jacobi else np.ones(n3)
    A = scale[:, None] * H * scale[None, :]
    L = np.linalg.cholesky(A)
    Linv = np.linalg.solve(L, np.eye(n3))            # (a triangular system: LAPACK's general solve is exact enough and always there)
    Z = Linv.T @ Linv
    return scale[:, None] * Z * scale[None, :]


def inverse_longdouble(H, jacobi=True, pairs=None):
    """(b); pairs: the (block row, block column) pairs wanted (None: the whole matrix), the others are NaN"""
    n3 = H.shape[0]
    Hl = H.astype(LD)
    scale = LD(1.0) / (LD(1.0) + np.sqrt(np.diag(Hl))) if jacobi else np.ones(n3, dtype=LD)
    A = scale[:, None] * Hl * scale[None, :]
    L = np.zeros_like(A)
    for j in range(n3):                               # column Cholesky
        d = A[j, j] - np.sum(L[j, :j] * L[j, :j])
        L[j, j] = np.sqrt(d)
        if j + 1 < n3:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Linv = np.zeros_like(A)
    for i in range(n3):                               # forward substitution on the identity, row by row (L^-1 is lower triangular)
        Linv[i, :i] = -(L[i, :i] @ Linv[:i, :i]) / L[i, i]
        Linv[i, i] = LD(1.0) / L[i, i]
    if pairs is None:
        Z = Linv.T @ Linv
    else:
        Z = np.full_like(A, np.nan)
        for bi, bj in pairs:
            lo = 3 * max(bi, bj)
            Z[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3] = Linv[lo:, 3 * bi:3 * bi + 3].T @ Linv[lo:, 3 * bj:3 * bj + 3]
    return scale[:, None] * Z * scale[None, :]


def rule(poses, edges, z, U=None, cov=None, loss="None", loss_scale=0.7, fixed=0, jacobi=True, reference=True):
    """reference=False: (a) only (sigma_ref is None), for a case whose bound is another case's"""
    p = spa.Problem(poses, edges, z, cov, fixed=fixed, loss=loss, loss_scale=loss_scale, U=U)
    _, _, H = p.linearize(np.asarray(poses, dtype=np.float64))
    H = np.asarray(H.todense())
    sigma = inverse_float64(H, jacobi)
    ref = None
    if reference and p.nfree <= LD_MAX_FREE:
        # (only the blocks ref_err looks at: the diagonal and the edges)
        pairs = {(c, c) for c in range(p.nfree)}
        for a, b in p.edges:
            if p.col_of[a] >= 0 and p.col_of[b] >= 0:
                pairs.add((int(p.col_of[a]), int(p.col_of[b])))
        ref = inverse_longdouble(H, jacobi, sorted(pairs))
    elif reference:
        ref = np.linalg.inv(H)
    return Rule(p, sigma, ref, H)


def diag_block(r, node, which="sigma"):
    """3 x 3 marginal of `node` (zeros for the gauge node; KeyError for a node that is not in the problem)"""
    c = r.problem.col_of[node]
    if c < 0:
        if node == r.problem.fixed and node in r.problem.edges:
            return np.zeros((3, 3))
        raise KeyError(node)
    return np.asarray(getattr(r, which)[3 * c:3 * c + 3, 3 * c:3 * c + 3])


def cross_block(r, a, b, which="sigma"):
    ca, cb = r.problem.col_of[a], r.problem.col_of[b]
    if ca < 0 or cb < 0:
        return np.zeros((3, 3))
    return np.asarray(getattr(r, which)[3 * ca:3 * ca + 3, 3 * cb:3 * cb + 3])


def joint_block(r, a, b, which="sigma"):
    """6 x 6 [[aa ab], [ba bb]]"""
    return np.block([[diag_block(r, a, which), cross_block(r, a, b, which)], [cross_block(r, b, a, which), diag_block(r, b, which)]])


def rel_fro(got, want):
    want = np.asarray(want)
    d = np.asarray(got) - want
    den = float(np.sqrt(np.sum(want * want)))
    num = float(np.sqrt(np.sum(d * d)))
    return num / den if den > 0.0 else (0.0 if num == 0.0 else np.inf)


def ref_err(r):
    worst = 0.0
    for node in r.problem.free_nodes:
        worst = max(worst, rel_fro(diag_block(r, node), diag_block(r, node, "sigma_ref")))
    for a, b in r.problem.edges:
        if r.problem.col_of[a] >= 0 and r.problem.col_of[b] >= 0:
            worst = max(worst, rel_fro(cross_block(r, a, b), cross_block(r, a, b, "sigma_ref")))
    return worst


def inverse_float64_reversed(H, jacobi=True):
    """(a) on the same H with the free nodes eliminated in the reverse of the given order, handed back in the given order"""
    n = H.shape[0] // 3
    perm = (3 * np.arange(n - 1, -1, -1)[:, None] + np.arange(3)[None, :]).reshape(-1)
    back = np.empty_like(perm)
    back[perm] = np.arange(3 * n)
    Z = inverse_float64(np.ascontiguousarray(H[np.ix_(perm, perm)]), jacobi)
    return np.ascontiguousarray(Z[np.ix_(back, back)])


def order_err(r, jacobi=True, reversed_sigma=None):
    """what the elimination order alone changes in float64: rule (a) under the given node order against rule (a) under its
    reverse (reversed_sigma: inverse_float64_reversed(r.H), where the caller has it already), block by block in the measure of
    ref_err (diagonal blocks and the cross blocks of the edges)"""
    return ref_err(r._replace(sigma_ref=inverse_float64_reversed(r.H, jacobi) if reversed_sigma is None else reversed_sigma))


def tolerance(err):
    """a block of the library may be this far (relative Frobenius) from (a): the factor 8 covers another elimination order and the
    reciprocal-square-root pivots of the device"""
    return max(8.0 * err, 64.0 * EPS)


def complete_graph(n, seed=3):
    """every pair of n poses joined by a noisy measurement of their true difference: one root supernode holds all of them"""
    rng = np.random.default_rng(seed)
    truth = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-3, 3, n)])
    edges = np.array([(i, j) for i in range(n) for j in range(i + 1, n)])
    cov = np.tile(np.diag([0.01, 0.01, 0.004]).reshape(1, 9), (len(edges), 1))
    z = np.zeros((len(edges), 3))
    for e, (i, j) in enumerate(edges):
        d, _ = spa.link_info(truth[i], truth[j], np.eye(3))
        z[e] = np.asarray(d) + rng.normal(0, [0.02, 0.02, 0.01])
    init = truth + rng.normal(0, 0.02, truth.shape)
    init[0] = truth[0]
    return dict(init=init, edges=edges, z=z, cov=cov)


def chain(n, closed=False):
    """n poses one metre apart along x, odometry constraints; `closed` adds the constraint from the last pose back to the first"""
    poses = np.column_stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)])
    edges = [(i, i + 1) for i in range(n - 1)] + ([(n - 1, 0)] if closed else [])
    z = np.array([[poses[b, 0] - poses[a, 0], 0.0, 0.0] for a, b in edges])
    cov = np.tile(np.diag([0.01, 0.01, 0.002]).reshape(1, 9), (len(edges), 1))
    return dict(init=poses, edges=np.array(edges), z=z, cov=cov)
