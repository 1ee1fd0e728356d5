"""GPU: the constraint audit of the solver (kh_spa_audit_constraints: k_edge_audit on the resident selected inverse) against the
dense rule of tests/audit_rule.py, on the cases of tests/audit_cases.py -- each audited at the poses the case names, so the device
and the rule linearise at the same point.

chi2, redundancy, min_pivot and chi2_loo of every constraint may differ from route (a) of the rule by at most
covariance_rule.tolerance(ref_err of that quantity on the case) in the measure audit_rule.error gives the quantity; the flags must
be equal exactly (tests/test_audit_rule_oracle.py checks on the CPU that no pivot of a case is near the threshold).

Reading of "a parallel constraint with its information scaled by 1e-9, which must come out unverifiable": the constraint such a
copy runs parallel to is the one that comes out unverifiable -- the copy is all that checks it, M = 1e-9 of the identity -- while the
copy itself is checked by the full-weight constraint (redundancy 3 to nine digits)."""
import numpy as np
import pytest

import audit_cases as ac
import audit_rule as ar
import covariance_rule as cr
from slam_toolbox_amd import capi

pytestmark = pytest.mark.gpu


def make_solver(g, loss="None"):
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    sol = HipSpaSolver(options={"loss_function": loss, "loss_scale": 0.7} if loss != "None" else None)
    sol.load(g["init"], g["edges"], g["z"], g["cov"])
    return sol


@pytest.fixture(scope="module")
def rules():
    """name -> (float64 audit, long-double audit) of the rule, computed once and shared"""
    cache = {}

    def get(name):
        if name not in cache:
            g, loss = ac.case(name)
            p = ar.problem(g, loss)
            cache[name] = (ar.audit(p, g["init"], ac.MIN_REDUNDANCY), ar.audit(p, g["init"], ac.MIN_REDUNDANCY, np.longdouble))
        return cache[name]
    return get


def compare(name, g, rec, a64, ald):
    err = ar.ref_err(a64, ald)
    assert len(rec) == len(g["edges"])
    assert np.array_equal(rec["index"], np.arange(len(rec)))
    assert np.array_equal(rec["id_a"], g["edges"][:, 0]) and np.array_equal(rec["id_b"], g["edges"][:, 1])
    line = []
    worst = {}
    for q in ar.QUANTITIES:
        e = ar.error(q, rec[q], getattr(a64, q))
        if q == "chi2_loo":
            e = e[a64.verifiable == 1]
        worst[q] = float(e.max()) if e.size else 0.0
        line.append(f"{q} {worst[q]:.2e} / {cr.tolerance(err[q]):.2e}")
    print(f"[audit] {name}: " + ", ".join(line) + f"; verifiable {int(rec['verifiable'].sum())} of {len(rec)}")
    assert np.array_equal(rec["verifiable"], a64.verifiable), name
    assert np.all(rec["chi2_loo"][rec["verifiable"] == 0] == -1.0)
    for q in ar.QUANTITIES:
        assert worst[q] <= cr.tolerance(err[q]), (name, q, worst[q], cr.tolerance(err[q]))


@pytest.mark.parametrize("name", list(ac.CASES))
def test_audit_matches_the_rule(kartohip_lib, rules, name):
    g, loss = ac.case(name)
    a64, ald = rules(name)
    sol = make_solver(g, loss)
    rec = sol.AuditConstraints(ac.MIN_REDUNDANCY)
    s = sol.audit_summary
    assert s["n_constraints"] == len(g["edges"]) and s["n_verifiable"] == int(rec["verifiable"].sum())
    assert s["cov"]["n_free"] == a64.problem.nfree and s["cov"]["total_ms"] > 0.0 and s["total_ms"] >= s["cov"]["total_ms"]
    assert s["kernel_ms"] == 0.0                                              # (no events without debug bit 1)
    compare(name, g, rec, a64, ald)
    if name == "open chain 5":
        assert not rec["verifiable"].any()
    if name == "complete 24":
        assert len(rec) == 276 and rec["verifiable"].all()                    # a full workgroup and a partial one
    if name == "weak parallel":
        assert rec["verifiable"].tolist() == [0, 0, 0, 0, 1] and 0.0 < rec["min_pivot"][2] < 1e-8
    if name == "zero residual":
        zero = [e for e, (a, b) in enumerate(g["edges"]) if 3 not in (a, b)]
        assert (rec["chi2"][zero] == 0.0).all() and (rec["chi2_loo"][zero] == 0.0).all() and rec["verifiable"].all()
    if name == "40/60 false closure":
        cand = ar.candidates(rec["id_a"], rec["id_b"], rec["verifiable"], 2)
        assert ar.pick(rec["chi2_loo"], cand)[0] == len(rec) - 1
    if name == "gauge as a and as b":
        assert rec["id_a"][0] == 0 and rec["id_b"][-1] == 0 and rec["verifiable"][0] == 1 and rec["verifiable"][-1] == 1
    sol.close()


def test_second_audit_rides_on_the_resident_pass(kartohip_lib):
    g, loss = ac.case("40/60")
    sol = make_solver(g, loss)
    first = sol.AuditConstraints()
    assert sol.audit_summary["cov"]["total_ms"] > 0.0
    second = sol.AuditConstraints()
    s = sol.audit_summary
    assert all(v == 0 for v in s["cov"].values()), s                         # nothing ran: all zeros
    assert s["n_constraints"] == len(first) and first.tobytes() == second.tobytes()
    # ... on a pass somebody else ran as well, whether it carried columns or not
    sol.ComputeCovariances()
    third = sol.AuditConstraints()
    assert all(v == 0 for v in sol.audit_summary["cov"].values())
    sol.ComputeCovarianceColumns([3, 17, 0])
    fourth = sol.AuditConstraints()
    assert all(v == 0 for v in sol.audit_summary["cov"].values())
    assert third.tobytes() == first.tobytes() and fourth.tobytes() == first.tobytes()
    # another threshold changes the flags' threshold alone: chi2 and redundancy keep their bits
    loose = sol.AuditConstraints(0.5)
    assert loose["chi2"].tobytes() == first["chi2"].tobytes() and loose["redundancy"].tobytes() == first["redundancy"].tobytes()
    assert loose["verifiable"].sum() < first["verifiable"].sum()
    sol.close()


def test_audit_with_events_reports_the_kernel_time(kartohip_lib):
    g, loss = ac.case("40/60")
    sol = make_solver(g, loss)
    sol.set_debug(phase_timing=True)
    plain = make_solver(g, loss)
    a, b = sol.AuditConstraints(), plain.AuditConstraints()
    assert sol.audit_summary["kernel_ms"] > 0.0 and a.tobytes() == b.tobytes()
    sol.close()
    plain.close()


def test_audit_after_add_constraint_recomputes(kartohip_lib):
    """the graph of the 40 / 60 case, audited, then the false closure added: the audit must run a new pass and answer for the new
    graph at the poses the handle holds (the rule at those poses; the analysis is an incremental one, so not the bits of a fresh
    handle)"""
    g, _ = ac.case("40/60")
    sol = make_solver(g)
    before = sol.AuditConstraints()
    gf, _ = ac.case("40/60 false closure")
    sol.AddConstraint(int(gf["edges"][-1, 0]), int(gf["edges"][-1, 1]), gf["z"][-1], gf["cov"][-1].reshape(3, 3))
    after = sol.AuditConstraints()
    assert sol.audit_summary["cov"]["total_ms"] > 0.0 and len(after) == len(before) + 1
    now = dict(gf, init=g["init"])
    p = ar.problem(now)
    compare("40/60 + closure, stale poses", now, after, ar.audit(p, now["init"], ac.MIN_REDUNDANCY),
            ar.audit(p, now["init"], ac.MIN_REDUNDANCY, np.longdouble))
    assert after["chi2_loo"][-1] > 100.0 and not np.array_equal(after["chi2_loo"][:-1], before["chi2_loo"])
    sol.RemoveConstraint(int(gf["edges"][-1, 0]), int(gf["edges"][-1, 1]))
    again = sol.AuditConstraints()
    assert sol.audit_summary["cov"]["total_ms"] > 0.0 and len(again) == len(before)
    sol.close()


def test_audit_is_bit_neutral_for_compute_and_getters(kartohip_lib):
    from slam_toolbox_amd import synth
    g = synth.make_pose_graph(60, 100, seed=11)
    plain, audited = make_solver(g), make_solver(g)
    audited.AuditConstraints()
    assert plain.Compute()["usable"] == 1 and audited.Compute()["usable"] == 1
    assert plain.poses().tobytes() == audited.poses().tobytes()
    plain.ComputeCovariances()
    rec = audited.AuditConstraints()                                        # runs the pass itself and leaves it resident
    assert audited.Covariances().tobytes() == plain.Covariances().tobytes()
    a, b = (int(v) for v in g["edges"][70])
    assert audited.JointCovariance(a, b).tobytes() == plain.JointCovariance(a, b).tobytes()
    assert len(rec) == len(g["edges"])
    assert plain.Compute()["usable"] == 1 and audited.Compute()["usable"] == 1
    assert plain.poses().tobytes() == audited.poses().tobytes()
    for s in (plain, audited):
        s.close()


def test_refusals_and_empty_graph(kartohip_lib):
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    sol = HipSpaSolver()
    sol.AddNode(0, [0.0, 0.0, 0.0])
    sol.AddNode(1, [1.0, 0.0, 0.0])
    rec = sol.AuditConstraints()                                            # no constraints: KH_OK and no records
    assert len(rec) == 0 and sol.audit_summary["n_constraints"] == 0
    # a component that is not tied to the gauge: the covariance pass refuses, and so does the audit
    sol.AddNode(2, [5.0, 0.0, 0.0])
    sol.AddNode(3, [6.0, 0.0, 0.0])
    cov = np.diag([0.01, 0.01, 0.002])
    sol.AddConstraint(0, 1, [1.0, 0.0, 0.0], cov)
    sol.AddConstraint(2, 3, [1.0, 0.0, 0.0], cov)
    with pytest.raises(capi.KartoHipError) as err:
        sol.AuditConstraints()
    assert err.value.code == capi.KH_ERR_SOLVER
    sol.close()
