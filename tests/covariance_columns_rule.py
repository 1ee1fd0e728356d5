"""What the covariance columns (kh_spa_compute_covariance_columns) are pinned to: the block columns Sigma(:, q) of the dense rule of
tests/covariance_rule.py, for pairs of nodes with or without a constraint between them.

A cross block can be small against the two marginals it sits between (two poses at opposite ends of a map are almost
independent), so a block's error is not taken relative to the block but to the scale Cauchy-Schwarz gives it:

    err(i, q) = |got - want|_F / sqrt(|Sigma_ii|_F |Sigma_qq|_F)

ref_err is that measure between rule (a), covariance_rule.inverse_float64, and rule (b), inverse_longdouble on the pairs (i, q) (or
np.linalg.inv above LD_MAX_FREE free nodes); the bound on the library is covariance_rule.tolerance(ref_err), as for the marginals."""
import numpy as np

import covariance_rule as cr


def blocks(sigma, rows, col):
    """(len(rows), 3, 3): the blocks (i, col) of a dense matrix, i over `rows` (block indices)"""
    return np.stack([np.asarray(sigma[3 * i:3 * i + 3, 3 * col:3 * col + 3], dtype=np.float64) for i in rows])


def scales(sigma):
    """|Sigma_ii|_F per block row"""
    n = sigma.shape[0] // 3
    return np.array([np.sqrt(np.sum(np.asarray(sigma[3 * i:3 * i + 3, 3 * i:3 * i + 3], dtype=np.float64) ** 2)) for i in range(n)])


def column_error(got, want, scale, q):
    """largest err(i, q) over the rows of a column; got, want: (n, 3, 3) in block order, scale = scales(sigma of rule (a))"""
    d = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    num = np.sqrt(np.sum(d * d, axis=(1, 2)))
    return float(np.max(num / np.sqrt(scale * scale[q])))


def reference_columns(H, queries, jacobi=True):
    """rule (b) for the block columns `queries` (block indices): {q: (n, 3, 3)}"""
    n = H.shape[0] // 3
    if n <= cr.LD_MAX_FREE:
        # (every column asked for: the whole matrix in one product)
        ref = cr.inverse_longdouble(H, jacobi, pairs=None if len(set(queries)) == n else [(i, q) for q in queries for i in range(n)])
    else:
        ref = np.linalg.inv(H)
    return {q: blocks(ref, range(n), q) for q in queries}


def ref_err(r, queries, jacobi=True):
    """largest err(i, q) between rule (a) (r.sigma) and rule (b), and rule (b)'s columns"""
    n = r.problem.nfree
    ref = reference_columns(r.H, queries, jacobi)
    scale = scales(r.sigma)
    return max(column_error(blocks(r.sigma, range(n), q), ref[q], scale, q) for q in queries), ref


def joint_any(r, a, b):
    """6 x 6 [[aa ab], [ba bb]] of ANY two nodes of the problem from rule (a); rows and columns of the gauge are zeros"""
    return cr.joint_block(r, a, b)
