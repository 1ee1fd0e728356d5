"""GPU: the selected inverse (k_selinv_head / _z21 / _z11) and the covariance columns (k_cov_columns_forward / _backward) at the
front shapes of tests/covariance_cases.py, where each kernel's handling of partial tiles, its last waves and its second loop
rounds are live: one test per case, every comparison at the poses the solver holds, against the dense rule of
tests/covariance_rule.py.

Per case: every diagonal block and every edge's cross block relative to the block, every edge's joint 6 x 6 (in these families every
block on the pattern of L is an edge), the gauge's zeros, bit-wise symmetric joints; then the WHOLE inverse by columns (every free
node a query, batches of at most 64; three queries on the wide level) in the measure of tests/covariance_columns_rule.py, column q's
block i against the transpose of column i's block q, and block (q, q) against the marginal; for the petals, two nodes of different
petals (no constraint between them) through JointCovarianceAny and RelativeCovariances.

Bounds (covariance_cases.bounds, from the rule alone at the same poses): max(8 * max(ref_err, order_err), 64 * 2^-52), ref_err rule (a)
against rule (b), order_err rule (a) under the given node order against its reverse; once in the marginals' measure (diagonal and
edge blocks, relative to the block) and once in the columns' measure (every block, relative to sqrt(|Sigma_ii| |Sigma_qq|)).  Never
from what the library returns.  The cases, their front shapes and the figures seen are in DESIGN.md (covariance section).

Besides the cases: a column's bytes do not depend on its company (alone, sixth of 6, 43rd of 64: its three right-hand sides then sit
in one 16-column tile, across 15 | 16 and across 127 | 128), on the chain of five fronts; and one handle taken through four graphs
of different front shapes in turn equals a fresh handle bit for bit at every step (stale zbuf, winv, G left in the fronts, B rows)."""
import numpy as np
import pytest

import covariance_cases as cc
import covariance_columns_rule as ccr
import covariance_rule as cr
from slam_toolbox_amd import capi, synth
from slam_toolbox_amd.scan_solver import relative_covariance
from test_covariance_gpu import COUNTERS, current_poses, make_solver, raises

pytestmark = pytest.mark.gpu


def padded(sigma):
    """sigma with a block row and column of zeros behind it: where col_of = -1 (the gauge) points"""
    out = np.zeros((sigma.shape[0] + 3, sigma.shape[0] + 3))
    out[:-3, :-3] = sigma
    return out


def blocks_of(dense, rows, cols):
    """(len(rows), 3, 3): block (rows[k], cols[k]) of a dense matrix"""
    idx = np.arange(3)
    return dense[(3 * np.asarray(rows))[:, None, None] + idx[None, :, None], (3 * np.asarray(cols))[:, None, None] + idx[None, None, :]]


def fro(a):
    return np.sqrt(np.sum(a * a, axis=tuple(range(1, a.ndim))))


def marginals_and_joints(sol, r, g):
    """-> (worst diagonal block, worst cross block of an edge, worst joint 6 x 6 of an edge, each relative to what it is compared
    with; the free nodes' marginals).  The gauge's zeros and the joints' bit-wise symmetry are asserted here."""
    p = r.problem
    nodes = np.concatenate([p.free_nodes, [p.fixed]]).astype(np.int32)
    got = sol.Covariances(nodes)
    assert not got[-1].any(), "the gauge node's covariance is not zero"
    assert not sol.Covariance(p.fixed).any()
    want = blocks_of(r.sigma, range(p.nfree), range(p.nfree))
    worst_diag = float(np.max(fro(got[:-1] - want) / fro(want)))
    edges = np.asarray(g["edges"])
    joints = np.stack([sol.JointCovariance(int(a), int(b)) for a, b in edges])
    assert np.array_equal(joints, np.transpose(joints, (0, 2, 1))), "a joint covariance is not bit-wise symmetric"
    sp = padded(r.sigma)
    ca, cb = p.col_of[edges[:, 0]], p.col_of[edges[:, 1]]          # (-1: the zeros behind the matrix)
    want = np.zeros_like(joints)
    want[:, :3, :3], want[:, :3, 3:] = blocks_of(sp, ca, ca), blocks_of(sp, ca, cb)
    want[:, 3:, :3], want[:, 3:, 3:] = blocks_of(sp, cb, ca), blocks_of(sp, cb, cb)
    worst_joint = float(np.max(fro(joints - want) / fro(want)))
    free = (ca >= 0) & (cb >= 0)
    for k in np.flatnonzero(~free):                                 # an edge of the gauge: its rows and columns are zeros
        lo = 0 if ca[k] < 0 else 3
        assert not joints[k, lo:lo + 3, :].any() and not joints[k, :, lo:lo + 3].any()
    worst_cross = float(np.max(fro(joints[free][:, :3, 3:] - want[free][:, :3, 3:]) / fro(want[free][:, :3, 3:])))
    return worst_diag, worst_cross, worst_joint, got[:-1]


def columns_matrix(sol, r, queries):
    """(3 n_free, 3 len(queries)): the block columns of the listed free nodes side by side, asked for in batches of at most 64;
    every batch runs the marginals' pass again, which must give the same bytes"""
    free = r.problem.free_nodes.astype(np.int32)
    out = np.zeros((3 * len(free), 3 * len(queries)))
    marginals = None
    for b0 in range(0, len(queries), 64):
        batch = [int(q) for q in queries[b0:b0 + 64]]
        summ = sol.ComputeCovarianceColumns(batch)
        assert summ["n_queries"] == len(batch) and summ["cov"]["n_free"] == len(free)
        again = sol.Covariances(free)
        assert marginals is None or marginals.tobytes() == again.tobytes(), "the marginals changed with the queries"
        marginals = again
        assert not sol.CovarianceColumn(batch[0], [int(r.problem.fixed)]).any(), "the gauge as a row is not zeros"
        for k, q in enumerate(batch):
            col = sol.CovarianceColumn(q, free)                    # (n_free, 3, 3): block (i, q)
            out[:, 3 * (b0 + k):3 * (b0 + k) + 3] = col.reshape(-1, 3)
    return out


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_against_the_rule(kartohip_lib, monkeypatch, name):
    case = cc.BY_NAME[name]
    g = cc.graph(name)
    if case.leaf:
        monkeypatch.setenv("KH_SPA_LEAF", str(case.leaf))         # read by the handle's analysis
    sol = make_solver(g)
    n = g["init"].shape[0]
    ms = cc.measure(g, current_poses(sol, n))
    r, p = ms.rule, ms.rule.problem
    tol, col_tol = cc.bounds(ms)
    assert max(ms[1:]) <= cc.REF_CEILING, (name, ms[1:])
    summ = sol.ComputeCovariances()
    assert summ["n_free"] == p.nfree and summ["levels"] >= 2
    worst_diag, worst_cross, worst_joint, marginals = marginals_and_joints(sol, r, g)
    # the inverse by columns
    free = p.free_nodes
    queries = free if name != cc.WIDE else free[[0, len(free) // 2, -1]]
    qcol = p.col_of[queries]
    X = columns_matrix(sol, r, queries)
    scale = ccr.scales(r.sigma)
    nq = len(queries)
    d = (X - r.sigma[:, (3 * qcol[:, None] + np.arange(3)[None, :]).reshape(-1)]).reshape(p.nfree, 3, nq, 3)
    err = np.sqrt(np.sum(d * d, axis=(1, 3))) / np.sqrt(np.outer(scale, scale[qcol]))
    worst_col = float(err.max())
    rows = (3 * qcol[:, None] + np.arange(3)[None, :]).reshape(-1)
    square = X[rows]                                               # the queries' own rows: block (q', q)
    asym = float(cc.block_errors(square, square.T, scale[qcol]).max())
    own = blocks_of(square, range(nq), range(nq))
    on_diag = float(np.max(fro(own - marginals[qcol]) / scale[qcol]))
    print(f"[covariance shapes] {name}: fronts {' '.join(str(s) for s in case.shapes)}, ref_err {ms.ref_err:.3e}, order_err {ms.order_err:.3e}, "
          f"diagonal blocks {worst_diag:.3e}, cross blocks {worst_cross:.3e}, joints {worst_joint:.3e}, bound {tol:.3e}; "
          f"columns: ref_err {ms.col_ref_err:.3e}, order_err {ms.col_order_err:.3e}, worst block {worst_col:.3e}, "
          f"column q against column i transposed {asym:.3e}, block (q, q) against the marginal {on_diag:.3e}, bound {col_tol:.3e}; "
          f"levels {summ['levels']}, {len(queries)} queries")
    assert worst_diag <= tol and worst_cross <= tol and worst_joint <= tol, (name, worst_diag, worst_cross, worst_joint, tol)
    assert worst_col <= col_tol and asym <= col_tol and on_diag <= col_tol, (name, worst_col, asym, on_diag, col_tol)
    # two nodes of different petals: no constraint, so only the columns know their cross block
    pair = cc.other_petal_pair(name)
    if pair is not None:
        a, b = pair
        have = {(int(i), int(j)) for i, j in g["edges"]}
        assert (a, b) not in have and (b, a) not in have
        sol.ComputeCovarianceColumns([a])
        raises(capi.KH_ERR_NOT_FOUND, sol.JointCovariance, a, b, text="pattern")
        ia, ib = p.col_of[a], p.col_of[b]
        for u, v, iu, iv in ((a, b, ia, ib), (b, a, ib, ia)):
            j = sol.JointCovarianceAny(u, v)
            assert np.array_equal(j, j.T), "the joint covariance is not bit-wise symmetric"
            assert np.array_equal(j[:3, :3], sol.Covariance(u)) and np.array_equal(j[3:, 3:], sol.Covariance(v))
            e = float(fro((j[:3, 3:] - blocks_of(r.sigma, [iu], [iv])[0])[None])[0] / np.sqrt(scale[iu] * scale[iv]))
            assert e <= col_tol, (name, u, v, e, col_tol)
        # RelativeCovariances against the host's first-order rule on the DENSE rule's joint: |J D J^T| <= |J|^2 |D| for what the
        # joint may be off by (tol on the two marginals, col_tol on the cross blocks), and the project's rounding floor carried
        # through the two 3 x 6 products
        ids, poses = sol.node_arrays()
        pose_of = {int(i): q for i, q in zip(ids, poses)}
        listed = [b, a, int(p.fixed)]
        rel = sol.RelativeCovariances(a, listed)
        assert not rel[1].any(), "the reference against itself is not exact zeros"
        worst_rel = 0.0
        for k, i in enumerate(listed):
            joint = cr.joint_block(r, a, i)
            want = relative_covariance(pose_of[a], pose_of[i], joint)
            dx, dy = pose_of[i][0] - pose_of[a][0], pose_of[i][1] - pose_of[a][1]
            jac2 = 2.0 * (2.0 + 1.0) + (dx * dx + dy * dy)          # |J|_F^2: two rotations, two ones, the lever arm
            si = scale[p.col_of[i]] if p.col_of[i] >= 0 else 0.0
            off = np.sqrt(tol * tol * (scale[ia] ** 2 + si ** 2) + 2.0 * col_tol * col_tol * scale[ia] * si)
            bound = jac2 * (off + 64.0 * cr.EPS * float(np.sqrt(np.sum(joint * joint))))
            worst_rel = max(worst_rel, float(np.sqrt(np.sum((rel[k] - want) ** 2))) / bound)
        print(f"[covariance shapes] {name}: nodes {a} and {b} of different petals, relative covariances |got - rule| / bound {worst_rel:.3e}")
        assert worst_rel <= 1.0, (name, worst_rel)
    sol.close()


# ---- a column does not depend on its company -------------------------------------------------------------------------------------
def test_column_bytes_do_not_depend_on_the_company_on_the_chain_of_five(kartohip_lib):
    g = cc.graph(cc.CHAIN5)
    sol = make_solver(g)
    n = g["init"].shape[0]
    others = [v for v in range(1, n) if v % 3 != 1][:63]           # (the queries below are all 1 mod 3)
    for q in (1, 94, n - 2):                                       # separator nodes and a petal's only node
        assert q % 3 == 1 and q not in others
        sol.ComputeCovarianceColumns([q])                          # columns 0..2
        alone = sol.CovarianceColumn(q).copy()
        assert alone.any()
        sol.ComputeCovarianceColumns(others[:5] + [q])             # columns 15 | 16, 17
        assert sol.CovarianceColumn(q).tobytes() == alone.tobytes(), f"column of node {q} changed with 5 others"
        sol.ComputeCovarianceColumns(others[:42] + [q] + others[42:])      # columns 126, 127 | 128
        assert sol.CovarianceColumn(q).tobytes() == alone.tobytes(), f"column of node {q} changed with 63 others"
    sol.close()


# ---- one handle across shapes ----------------------------------------------------------------------------------------------------
def handle_steps(sol, g):
    """what a handle answers to Compute, ComputeCovariances (twice), ComputeCovarianceColumns, Compute on a freshly loaded graph"""
    n = g["init"].shape[0]
    sol.load(g["init"], g["edges"], g["z"], g["cov"])
    out = []
    first = sol.Compute()
    assert first["usable"] == 1 and sol.last_warning == ""
    out.append(("Compute", [first[k] for k in COUNTERS], sol.iteration_log().tobytes(), sol.poses().tobytes()))
    sol.ComputeCovariances()
    marginals = sol.Covariances().copy()
    sol.ComputeCovariances()
    assert sol.Covariances().tobytes() == marginals.tobytes(), "a second pass on unchanged poses gave other bytes"
    out.append(("ComputeCovariances", marginals.tobytes()))
    queries = [1, n // 2, n - 1]
    sol.ComputeCovarianceColumns(queries)
    out.append(("ComputeCovarianceColumns", sol.Covariances().tobytes(), b"".join(sol.CovarianceColumn(q).tobytes() for q in queries)))
    assert out[-1][1] == marginals.tobytes()
    second = sol.Compute()
    assert second["usable"] == 1 and sol.last_warning == "", sol.last_warning
    out.append(("Compute again", [second[k] for k in COUNTERS], sol.iteration_log().tobytes(), sol.poses().tobytes()))
    return out


def test_one_handle_across_front_shapes_equals_fresh_handles(kartohip_lib):
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    graphs = [(cc.CHAIN5, cc.graph(cc.CHAIN5)), ("12/11", synth.make_pose_graph(12, 11, seed=2)), ("clique 85", cc.graph("clique 85")),
              ("petals(2, 42, 2)", cc.graph("petals(2, 42, 2)"))]
    reused = HipSpaSolver()
    for name, g in graphs:
        fresh = HipSpaSolver()
        want = handle_steps(fresh, g)
        fresh.close()
        got = handle_steps(reused, g)
        for a, b in zip(got, want):
            assert a == b, f"{name}: the reused handle differs from a fresh one at {a[0]}"
    reused.close()
