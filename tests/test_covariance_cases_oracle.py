"""CPU: does the table of tests/covariance_cases.py still reach the front shapes it is there for, and does the reference alone stay
far inside the ceiling that keeps a case's bound tight?

The shapes come from the library's own analysis (tools/sym_probe.cpp through tests/test_spa_symbolic.py's probe, at the options
the handle uses: the defaults, or the case's KH_SPA_LEAF as the leaf size).  Asserted: every case reaches the classes it claims; over
the table ns takes 3, a value in 4..15, 48, 96, a value in 97..111 (wave 6 of the one-wave-per-pivot-block kernels), a value in
113..125 and 126 (wave 7, the 36 tiles of Z11); nu takes 0, 3, a value in 4..15, a multiple of 16, a value in 113..128, one in
129..256 (the second round of the forward sweep's row loop) and one above 384; ns mod 8 and nu mod 8 take all eight residues (the
remainder step of selinv_product); a chain of three fronts whose two lower ones have an update block; a level of more than 256
fronts with an update block (the gather grid at its floor of one workgroup).

A small ns together with nu >= 129 is not asked for: the analysis merges such graphs into even chains (a 3-pivot separator under a
200-row update block does not survive as a front of its own).

The tolerance inputs are measured from the rule alone and printed per case (covariance_cases.measure): ref_err, rule (a) against
rule (b); order_err, rule (a) under the given node order against rule (a) under its reverse.  Asserted: max(ref_err, order_err) <=
1e-12 in both measures for every case, so that no bound 8 * max(...) is wide enough to hide a wrong tail entry."""
import numpy as np
import pytest

import covariance_cases as cc
import covariance_rule as cr
from test_spa_symbolic import _probe, probe_exe  # noqa: F401  (probe_exe is a fixture)

COVERAGE = ["ns 3", "ns 4..15", "ns 48", "ns 96", "ns 97..111", "ns 113..125", "ns 126",
            "nu 0", "nu 3", "nu 4..15", "nu 16k", "nu 113..128", "nu 129..256", "nu > 384", "chain", "wide level"] + \
           [f"{which} mod 8 = {r}" for which in ("ns", "nu") for r in range(8)]


def probe_case(exe, tmp_path, case):
    g = cc.graph(case.name)
    return g, _probe(exe, tmp_path, g["edges"], g["init"].shape[0], (case.leaf,) if case.leaf else ())


@pytest.fixture(scope="module")
def reached(probe_exe, tmp_path_factory):       # noqa: F811
    """{case name: (the classes its fronts are in, its fronts' shapes)}"""
    out = {}
    for case in cc.CASES:
        _, sym = probe_case(probe_exe, tmp_path_factory.mktemp("sym"), case)
        fronts = cc.fronts_of(sym)
        out[case.name] = ({name for name, pred in cc.CLASSES.items() if pred(fronts)}, cc.shapes(sym))
        print(f"[covariance cases] {case.name}: {len(fronts)} fronts, shapes {sorted(cc.shapes(sym), key=lambda t: (t[1], t[0]))}")
    return out


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_reaches_the_classes_it_claims(reached, name):
    case = cc.BY_NAME[name]
    assert case.claims and set(case.claims) <= set(cc.CLASSES)
    missing = [c for c in case.claims if c not in reached[name][0]]
    assert not missing, (name, missing)
    assert reached[name][1] == set(case.shapes), (name, reached[name][1])


@pytest.mark.parametrize("cls", COVERAGE)
def test_table_covers_the_class(reached, cls):
    assert any(cls in got for got, _ in reached.values()), cls
    assert any(cls in c.claims for c in cc.CASES), f"no case claims {cls}"


def test_free_nodes_stay_within_the_long_double_rule():
    for case in cc.CASES:
        n = cc.graph(case.name)["init"].shape[0] - 1
        assert (n > cr.LD_MAX_FREE) == (case.name == cc.WIDE), (case.name, n)


def test_shapes_helper_and_families(probe_exe, tmp_path):       # noqa: F811
    # the helper on the smallest member of each family, where the answer is known without the probe: one front of all free nodes
    g = cc.clique(5)
    sym = _probe(probe_exe, tmp_path, g["edges"], 5)
    assert cc.shapes(sym) == {(12, 0)} and len(g["edges"]) == 10
    g = cc.petals(2, 3, 2)
    assert g["init"].shape == (8, 3) and len(g["edges"]) == 1 + 2 * (2 * 3 + 3)
    pairs = {(int(a), int(b)) for a, b in g["edges"]}
    assert (2, 5) not in pairs and (4, 7) not in pairs and (1, 7) in pairs and (2, 4) in pairs and (5, 7) in pairs
    assert cc.other_petal_pair("petals(2, 3, 2)") == (3, 7) and cc.other_petal_pair("clique 5") is None


def test_order_err_is_the_rule_under_the_reverse_node_order():
    g = cc.petals(2, 3, 2)
    r = cr.rule(g["init"], g["edges"], g["z"], cov=g["cov"])
    n = r.problem.nfree
    rev = cr.inverse_float64_reversed(r.H)
    # by hand: reverse the block order, invert, reverse back
    order = np.concatenate([3 * k + np.arange(3) for k in range(n - 1, -1, -1)])
    want = np.empty_like(rev)
    want[np.ix_(order, order)] = cr.inverse_float64(r.H[np.ix_(order, order)])
    assert np.array_equal(rev, want) and not np.array_equal(rev, r.sigma)
    e = cr.order_err(r)
    assert 0.0 < e <= 64 * cr.EPS and e == cr.order_err(r, reversed_sigma=rev) == cr.ref_err(r._replace(sigma_ref=rev))
    # a wrong entry in one tail block shows at its size, in both measures
    bad = r.sigma.copy()
    bad[-1, -1] *= 1.0 + 1e-9
    scale = cc.ccr.scales(r.sigma)
    assert cr.ref_err(r._replace(sigma=bad)) > 1e-10 and cc.block_errors(bad, r.sigma, scale).max() > 1e-10
    assert cc.block_errors(r.sigma, rev, scale).max() <= 64 * cr.EPS


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_reference_alone_stays_far_inside_the_ceiling(name):
    ms = cc.measure(cc.graph(name))
    tol, col_tol = cc.bounds(ms)
    print(f"[covariance cases] {name}: free nodes {ms.rule.problem.nfree}, ref_err {ms.ref_err:.3e}, order_err {ms.order_err:.3e}, bound {tol:.3e}; "
          f"columns: ref_err {ms.col_ref_err:.3e}, order_err {ms.col_order_err:.3e}, bound {col_tol:.3e}")
    assert max(ms.ref_err, ms.order_err, ms.col_ref_err, ms.col_order_err) <= cc.REF_CEILING, (name, ms[1:])
