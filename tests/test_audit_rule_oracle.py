"""CPU: the audit rule (tests/audit_rule.py) against what is known about the leave-one-out statistic without it -- the actual
leave-one-out done the long way, the open and the closed chain, the rejection policy on graphs with an injected false closure --
and the conditions the GPU comparison (tests/test_audit_gpu.py) relies on, for every case of tests/audit_cases.py."""
import numpy as np
import pytest

import audit_cases as ac
import audit_rule as ar
import covariance_rule as cr

LD = np.longdouble


@pytest.fixture(scope="module")
def audited():
    """name -> (graph, float64 audit, long-double audit), computed once"""
    out = {}
    for name in ac.CASES:
        g, loss = ac.case(name)
        p = ar.problem(g, loss)
        out[name] = (g, ar.audit(p, g["init"], ac.MIN_REDUNDANCY), ar.audit(p, g["init"], ac.MIN_REDUNDANCY, LD))
    return out


@pytest.mark.parametrize("name", ["40/60", "40/60 false closure", "a->b and b->a", "gauge as a and as b", "huber"])
def test_chi2_loo_is_the_actual_leave_one_out(audited, name):
    """Edge dropped, the remaining linearised system solved once in long double, the residual the dropped edge is predicted to have
    and the covariance of that prediction.  The identity assumes the poses are the minimum of the full system (gradient zero); the
    tight solve (parameter tolerance 1e-14) leaves steps of 1e-13 m at the most, which the whitening (sigma 0.02 to 0.03) and the
    conditioning of the remaining system (1e4 on these graphs) turn into 1e-8 of a residual of order one at the very most: 1e-6
    relative, plus 1e-12 for the residuals that are zero by themselves, leaves two digits.  Under Huber the weights are those of
    the linearisation, held fixed."""
    _, a64, ald = audited[name]
    worst = 0.0
    n = 0
    for e in np.flatnonzero(ald.verifiable):
        chi2, e_loo, cov = ar.actual_leave_one_out(ald, e)
        worst = max(worst, abs(float(chi2 - ald.chi2_loo[e])) / max(float(chi2), 1e-6))
        assert abs(chi2 - ald.chi2_loo[e]) <= 1e-6 * chi2 + 1e-12, (e, chi2, ald.chi2_loo[e])
        # ... and the float64 route says the same to its own rounding
        assert abs(a64.chi2_loo[e] - chi2) <= 2e-6 * chi2 + 1e-12
        n += 1
    print(name, "edges", n, "worst relative difference", worst)
    assert n > 0


def test_every_edge_of_an_open_chain_is_unverifiable(audited):
    for name in ("open chain 5",):
        _, a64, ald = audited[name]
        for a in (a64, ald):
            assert not a.verifiable.any() and (a.chi2_loo == -1.0).all()
            assert np.abs(a.redundancy).max() < 1e-9 and np.abs(a.min_pivot).max() < 1e-9
    g = cr.chain(9)
    a = ar.audit(ar.problem(g), g["init"])
    assert not a.verifiable.any()


def test_all_edges_of_a_closed_chain_share_one_chi2_loo(audited):
    _, a64, ald = audited["closed chain 12"]
    assert ald.verifiable.all() and a64.verifiable.all()
    assert float(ald.chi2_loo.min()) > 1.0                                   # (a residual worth sharing)
    # one cycle: the only disagreement in the graph is the cycle's, whichever edge is left out
    assert float(ald.chi2_loo.max() - ald.chi2_loo.min()) <= 1e-9 * float(ald.chi2_loo.max())
    assert float(a64.chi2_loo.max() - a64.chi2_loo.min()) <= 1e-8 * float(a64.chi2_loo.max())
    # ... while the plain chi2 is spread over the edges by their information
    assert float(ald.chi2.max()) < float(ald.chi2_loo.min())


def test_weak_parallel_leaves_the_edge_unverifiable(audited):
    g, a64, ald = audited["weak parallel"]
    strong = 2
    weak = len(g["edges"]) - 1
    for a in (a64, ald):
        assert a.verifiable[strong] == 0 and 0.0 < a.min_pivot[strong] < 1e-8
        assert a.verifiable[weak] == 1 and a.redundancy[weak] > 3.0 - 1e-6
        assert a.verifiable.sum() == 1


def test_zero_residual_edges_audit_to_exact_zeros(audited):
    g, a64, _ = audited["zero residual"]
    zero = [e for e, (a, b) in enumerate(g["edges"]) if 3 not in (a, b)]
    assert len(zero) == 4 and (a64.chi2[zero] == 0.0).all() and (a64.chi2_loo[zero] == 0.0).all()
    assert (a64.chi2[[2, 3]] > 0.0).all() and a64.verifiable.all()


def test_huber_case_has_edges_on_both_sides_of_the_threshold(audited):
    from oracle import spa
    g, a64, _ = audited["huber"]
    p = ar.problem(g, "None")
    r, _ = spa._residuals(g["init"], p.edges[:, 0], p.edges[:, 1], p.z, p.U)
    sq = np.sum(r * r, axis=1)
    beyond = sq > 0.7 * 0.7
    assert beyond.any() and not beyond.all()
    # the audit sees the down-weighted residual: chi2 = rho' s < s beyond the threshold, = s below it
    assert np.all(a64.chi2[beyond] < sq[beyond]) and np.allclose(a64.chi2[~beyond], sq[~beyond], rtol=1e-12, atol=0)


@pytest.mark.parametrize("k", range(len(ac.SYNTHETIC)))
def test_clean_graphs_have_no_suspect(k):
    g = ac.synthetic(k)
    a = ar.audit(ar.problem(g), g["init"])
    v = a.verifiable == 1
    print(ac.SYNTHETIC[k], "largest chi2_loo", float(a.chi2_loo[v].max()))
    assert v.any() and float(a.chi2_loo[v].max()) < ar.CHI2_999


@pytest.mark.parametrize("k", range(len(ac.SYNTHETIC)))
@pytest.mark.parametrize("pair", (0, 1))
def test_policy_removes_exactly_the_injected_constraint(k, pair):
    n = ac.SYNTHETIC[k][0]
    g = ac.synthetic(k, pair)
    fa, fb = ac.false_pairs(n)[pair]
    index = len(g["edges"]) - 1
    assert tuple(g["edges"][index]) == (fa, fb)
    a = ar.audit(ar.problem(g), g["init"])
    cand = ar.candidates(g["edges"][:, 0], g["edges"][:, 1], a.verifiable, 2)
    order = np.argsort(-np.where(cand, a.chi2_loo, -np.inf))
    print(ac.SYNTHETIC[k], (fa, fb), "false", float(a.chi2_loo[index]), "chi2", float(a.chi2[index]), "largest", float(a.chi2_loo[order[0]]),
          "runner-up", float(a.chi2_loo[order[1]]))
    assert a.verifiable[index] == 1 and a.chi2_loo[index] > ar.CHI2_999
    removed, rounds, left, x, top = ar.reject_outliers(g)
    assert [(r[0], r[1], r[2]) for r in removed] == [(fa, fb, index)] and rounds == 2 and top <= ar.CHI2_999
    clean = ac.synthetic(k)
    assert np.array_equal(left["edges"], clean["edges"])
    d = x - clean["init"]
    d[:, 2] = (d[:, 2] + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() < 1e-6                                            # back at the clean solve
    # an unverifiable edge is never a candidate, so the components of the graph cannot multiply
    assert ar.components(n, left["edges"]) == ar.components(n, g["edges"]) == 1


def test_policy_exempts_odometry_and_breaks_ties_by_the_newest():
    chi2_loo = np.array([50.0, 50.0, 49.99999, 20.0, 50.0, -1.0])
    a = np.array([0, 1, 2, 3, 1, 7])
    b = np.array([1, 2, 9, 5, 3, 2])
    verifiable = np.array([1, 1, 1, 1, 1, 0])
    cand = ar.candidates(a, b, verifiable, 2)
    assert cand.tolist() == [False, False, True, True, True, False]
    assert ar.pick(chi2_loo, cand) == (4, 50.0)
    assert ar.pick(chi2_loo, cand, tie=0.0) == (4, 50.0)
    assert ar.pick(chi2_loo[:4], cand[:4], tie=1e-6) == (2, 49.99999)
    assert ar.pick(np.array([16.266, 3.0]), np.array([True, True])) == (-1, 16.266)          # top <= chi2 stops
    assert ar.pick(np.array([99.0]), np.array([False])) == (-1, 0.0)


def test_conditions_the_gpu_cases_rely_on(audited):
    thr = ac.MIN_REDUNDANCY
    for name, (g, a64, ald) in audited.items():
        for e, pivots in enumerate(ald.pivots):
            for d in pivots:
                assert d < thr / 100 or d > 100 * thr, (name, e, float(d))
        assert np.array_equal(a64.verifiable, ald.verifiable), name
        err = ar.ref_err(a64, ald)
        print(name, {k: f"{v:.2e}" for k, v in err.items()}, "verifiable", int(ald.verifiable.sum()), "of", len(ald.verifiable))
        per_edge = ar.error("chi2_loo", a64.chi2_loo, ald.chi2_loo)[ald.verifiable == 1]
        assert per_edge.size == 0 or per_edge.max() < 1e-6, name
        # candidates are tied with the top to rounding or clearly below it: the policy's pick cannot flip
        cand = ar.candidates(g["edges"][:, 0], g["edges"][:, 1], ald.verifiable, 2)
        if cand.any() and float(ald.chi2_loo[cand].max()) > 0:
            top = ald.chi2_loo[cand].max()
            rel = np.asarray((top - ald.chi2_loo[cand]) / top, dtype=np.float64)
            assert np.all((rel < 1e-8) | (rel > 1e-4)), (name, np.sort(rel)[:4])
