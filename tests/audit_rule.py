"""The rule the constraint audit (kh_spa_audit_constraints, k_edge_audit) is pinned to: a dense numpy
restatement on oracle.spa.Problem.  For constraint e between a and b, with r (3) the whitened, loss-weighted residual and
A = [Ja Jb] (3 x 6) of the linearisation at the given poses (spa._residuals, spa._jacobians, spa._loss; a gauge end has no Jacobian)
and Sigma = (J^T J)^-1 over the free nodes:

  chi2 = r^T r                   H_e = A Sigma(ab, ab) A^T (upper triangle, mirrored)          M = I - H_e
  redundancy = trace(M)          lower Cholesky of M in the order 0, 1, 2, pivots = the values under the square roots; it stops at
  the first pivot that is not > min_redundancy: the edge is unverifiable, chi2_loo = -1, min_pivot = the smallest pivot formed so
  far (the failing one included); otherwise chi2_loo = r^T x with L y = r, L^T x = y.

Every quantity is computed twice, as tests/covariance_rule.py does: (a) in float64 with Sigma from its inverse_float64, the way the
device does it, and (b) in np.longdouble from the same inputs, Sigma from its inverse_longdouble.  ref_err is what (a) loses
against (b), per quantity, the largest over the edges -- the error float64 itself makes on the case, which the tolerance of the GPU
tests is a multiple of (covariance_rule.tolerance: 8 ref_err, floor 64 * 2^-52).

How an error is measured, per quantity (error()): chi2 and chi2_loo are quadratic forms that scale with r, so their error is
relative -- against max(|want|, CHI2_FLOOR): the residual of a tree edge at the optimum is a rounding residue of z - z (1e-14 of
a whitened residual, 1e-28 of a chi-square) whose digits are noise in any arithmetic, and a chi-square below 1e-12 is zero for
every purpose the statistic has (the thresholds it meets are of order 10).  -1 against -1 is no error.  redundancy and min_pivot
are entries and pivots of M = I - H_e whose natural scale is the 1 of the identity -- the pivot of a bridge is a rounding residue
of 1 - 1 -- so their error is absolute.

The rejection policy of kh_mapper_reject_outliers is restated on the dense solve (reject_outliers)."""
from collections import namedtuple

import numpy as np

import covariance_rule as cr
from oracle import spa

LD = np.longdouble
QUANTITIES = ("chi2", "redundancy", "min_pivot", "chi2_loo")
RELATIVE = {"chi2": True, "redundancy": False, "min_pivot": False, "chi2_loo": True}
CHI2_FLOOR = 1e-12
CHI2_999 = 16.266                 # 99.9 % of chi-square with 3 degrees of freedom

Audit = namedtuple("Audit", "chi2 redundancy min_pivot chi2_loo verifiable pivots r A H sigma problem")


def linearization(p, x, dtype):
    """r (E, 3) and A (E, 3, 6) with the loss weights, zero columns for a gauge end; H = J^T J dense over the free nodes"""
    xs = np.asarray(x, dtype=dtype)
    ea, eb = p.edges[:, 0], p.edges[:, 1]
    U = p.U.astype(dtype)
    r, (c, s, dx, dy) = spa._residuals(xs, ea, eb, p.z.astype(dtype), U)
    Ja, Jb = spa._jacobians(c, s, dx, dy, U)
    Ja, Jb = Ja.astype(dtype), Jb.astype(dtype)
    if p.loss not in (None, "None"):
        _, rho1 = spa._loss(np.sum(r * r, axis=1), p.loss, dtype(p.loss_scale))
        w = np.sqrt(rho1)
        r, Ja, Jb = r * w[:, None], Ja * w[:, None, None], Jb * w[:, None, None]
    E = len(ea)
    A = np.zeros((E, 3, 6), dtype=dtype)
    H = np.zeros((3 * p.nfree, 3 * p.nfree), dtype=dtype)
    for e in range(E):
        ca, cb = int(p.col_of[ea[e]]), int(p.col_of[eb[e]])
        if ca >= 0:
            A[e, :, :3] = Ja[e]
        if cb >= 0:
            A[e, :, 3:] = Jb[e]
        J = np.zeros((3, 3 * p.nfree), dtype=dtype)
        if ca >= 0:
            J[:, 3 * ca:3 * ca + 3] += Ja[e]
        if cb >= 0:
            J[:, 3 * cb:3 * cb + 3] += Jb[e]
        H += J.T @ J
    return r, A, H


def joint_sigma(p, sigma, a, b, dtype):
    """6 x 6 [[aa ab], [ba bb]] of Sigma; zeros in the rows and columns of a gauge end"""
    out = np.zeros((6, 6), dtype=dtype)
    cols = [int(p.col_of[a]), int(p.col_of[b])]
    for i in range(2):
        for j in range(2):
            if cols[i] >= 0 and cols[j] >= 0:
                out[3 * i:3 * i + 3, 3 * j:3 * j + 3] = sigma[3 * cols[i]:3 * cols[i] + 3, 3 * cols[j]:3 * cols[j] + 3]
    return out


def factor(M, threshold):
    """the pivots formed (1 to 3), whether all three are > threshold, and L (valid when they are)"""
    dtype = M.dtype.type
    L = np.zeros((3, 3), dtype=dtype)
    pivots = []
    for j in range(3):
        d = M[j, j] - np.sum(L[j, :j] * L[j, :j])
        pivots.append(d)
        if not d > threshold:
            return pivots, False, L
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 3):
            L[i, j] = (M[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    return pivots, True, L


def audit(p, x, min_redundancy=1e-6, dtype=np.float64):
    """the audit of every edge of Problem p at the poses x, in `dtype` (np.float64: route (a); np.longdouble: route (b))"""
    r, A, H = linearization(p, x, dtype)
    if dtype is np.float64:
        sigma = cr.inverse_float64(H)
    else:
        sigma = cr.inverse_longdouble(H)
    E = len(p.edges)
    out = {q: np.zeros(E, dtype=dtype) for q in QUANTITIES}
    verifiable = np.zeros(E, dtype=np.int32)
    all_pivots = []
    for e, (a, b) in enumerate(p.edges):
        He = A[e] @ joint_sigma(p, sigma, a, b, dtype) @ A[e].T
        He = np.triu(He) + np.triu(He, 1).T
        M = np.eye(3, dtype=dtype) - He
        pivots, ok, L = factor(M, dtype(min_redundancy))
        all_pivots.append(pivots)
        out["chi2"][e] = r[e] @ r[e]
        out["redundancy"][e] = np.trace(M)
        out["min_pivot"][e] = min(pivots)
        verifiable[e] = 1 if ok else 0
        if ok:
            y = np.zeros(3, dtype=dtype)
            for i in range(3):
                y[i] = (r[e, i] - np.sum(L[i, :i] * y[:i])) / L[i, i]
            xx = np.zeros(3, dtype=dtype)
            for i in (2, 1, 0):
                xx[i] = (y[i] - np.sum(L[i + 1:, i] * xx[i + 1:])) / L[i, i]
            out["chi2_loo"][e] = r[e] @ xx
        else:
            out["chi2_loo"][e] = -1.0
    return Audit(out["chi2"], out["redundancy"], out["min_pivot"], out["chi2_loo"], verifiable, all_pivots, r, A, H, sigma, p)


def problem(g, loss="None", loss_scale=0.7):
    return spa.Problem(g["init"], g["edges"], g["z"], g.get("cov"), loss=loss, loss_scale=loss_scale, U=g.get("U"))


def error(quantity, got, want):
    """per edge: how far `got` is from `want` in the measure of the quantity (see the module's docstring)"""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    d = np.abs(got - want)
    if not RELATIVE[quantity]:
        return d.astype(np.float64)
    return (d / np.maximum(np.abs(want), LD(CHI2_FLOOR))).astype(np.float64)


def ref_err(a64, ald):
    """{quantity: the largest error of route (a) against route (b) over the edges}; chi2_loo over the edges verifiable in both"""
    out = {}
    for q in QUANTITIES:
        err = error(q, getattr(a64, q), getattr(ald, q))
        if q == "chi2_loo":
            both = (a64.verifiable == 1) & (ald.verifiable == 1)
            err = err[both]
        out[q] = float(err.max()) if err.size else 0.0
    return out


def actual_leave_one_out(ald, e):
    """What the identity claims, done the long way in long double: edge e dropped, the remaining linearised system solved once,
    the residual the dropped edge is predicted to have and that prediction's covariance.  Returns (chi2, e_loo, cov)."""
    p, r, A, H = ald.problem, ald.r, ald.A, ald.H
    n3 = H.shape[0]
    a, b = p.edges[e]

    def embed(Ae):
        J = np.zeros((3, n3), dtype=LD)
        for end, node in enumerate((a, b)):
            c = int(p.col_of[node])
            if c >= 0:
                J[:, 3 * c:3 * c + 3] += Ae[:, 3 * end:3 * end + 3]
        return J
    g = np.zeros(n3, dtype=LD)
    for k, (ka, kb) in enumerate(p.edges):
        if k == e:
            continue
        for end, node in enumerate((ka, kb)):
            c = int(p.col_of[node])
            if c >= 0:
                g[3 * c:3 * c + 3] += ald.A[k][:, 3 * end:3 * end + 3].T @ r[k]
    Je = embed(A[e])
    H_rest = H - Je.T @ Je
    inv = cr.inverse_longdouble(H_rest)
    delta = -(inv @ g)
    e_loo = r[e] + Je @ delta
    cov = np.eye(3, dtype=LD) + Je @ inv @ Je.T
    # (a 3 x 3 solve by the adjugate would do; the long-double Cholesky of this file is already there)
    pivots, ok, L = factor(cov, LD(0))
    assert ok
    y = np.zeros(3, dtype=LD)
    for i in range(3):
        y[i] = (e_loo[i] - np.sum(L[i, :i] * y[:i])) / L[i, i]
    return y @ y, e_loo, cov


def candidates(rec_a, rec_b, verifiable, min_id_gap):
    return (np.asarray(verifiable) == 1) & (np.abs(np.asarray(rec_a, dtype=np.int64) - np.asarray(rec_b, dtype=np.int64)) >= min_id_gap)


def pick(chi2_loo, cand, chi2=CHI2_999, tie=1e-6):
    """the policy of one round: (index to remove or -1, top).  Among the candidates within (1 - tie) of the largest chi2_loo, the
    one with the highest constraint index, when that largest exceeds chi2."""
    idx = np.flatnonzero(cand)
    if idx.size == 0:
        return -1, 0.0
    top = float(np.max(chi2_loo[idx]))
    if not top > chi2:
        return -1, top
    tied = idx[chi2_loo[idx] >= (1.0 - tie) * top]
    return int(tied.max()), top


def reject_outliers(g, chi2=CHI2_999, min_redundancy=1e-6, tie=1e-6, min_id_gap=2, max_rounds=8, options=None):
    """kh_mapper_reject_outliers on the dense solve: rounds of (solve, audit, remove one).  Returns (removed, rounds, g_left,
    poses, top): removed = [(a, b, index, chi2_loo)] in order, top = the largest candidate chi2_loo of the last audit."""
    g = dict(g)
    removed, rounds, top = [], 0, 0.0
    x = np.asarray(g["init"], dtype=np.float64)
    solved = True
    for _ in range(max_rounds):
        rounds += 1
        x, _ = spa.solve(x, g["edges"], g["z"], g["cov"], options or spa.Options.tight())
        solved = True
        a = audit(spa.Problem(x, g["edges"], g["z"], g["cov"]), x, min_redundancy)
        cand = candidates(g["edges"][:, 0], g["edges"][:, 1], a.verifiable, min_id_gap)
        k, top = pick(a.chi2_loo, cand, chi2, tie)
        if k < 0:
            break
        removed.append((int(g["edges"][k, 0]), int(g["edges"][k, 1]), k, float(a.chi2_loo[k])))
        keep = np.arange(len(g["edges"])) != k
        g["edges"], g["z"], g["cov"] = g["edges"][keep], g["z"][keep], g["cov"][keep]
        solved = False
    if not solved:
        x, _ = spa.solve(x, g["edges"], g["z"], g["cov"], options or spa.Options.tight())
    g["init"] = x
    return removed, rounds, g, x, top


def components(n_nodes, edges):
    """number of connected components among the nodes that have an edge"""
    root = list(range(n_nodes))

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i
    used = set()
    for a, b in np.asarray(edges).reshape(-1, 2):
        root[find(int(a))] = find(int(b))
        used.update((int(a), int(b)))
    return len({find(i) for i in used})
