"""The cases the constraint audit is compared on (tests/test_audit_gpu.py against tests/audit_rule.py), and the graphs with an
injected false closure of tests/test_audit_rule_oracle.py.  A case is a graph and the poses it is audited at: the poses of a tight
dense solve on the CPU (oracle.spa) unless the case says otherwise, so that the device and the rule linearise at the same point and
no Compute() stands between them.  tests/test_audit_rule_oracle.py checks, on the CPU and in long double, the conditions the GPU
comparison relies on for every case of the table: every Cholesky pivot is either below min_redundancy / 100 or above
100 min_redundancy (the flags cannot flip on rounding), and the rule's own float64 error of chi2_loo is below 1e-6."""
import functools

import numpy as np

import covariance_rule as cr
from oracle import spa
from slam_toolbox_amd import synth

MIN_REDUNDANCY = 1e-6
FALSE_OFFSET = np.array([1.0, -0.7, 0.4])
SYNTHETIC = ((40, 60, 7), (60, 100, 11), (30, 40, 3), (24, 30, 5))          # (nodes, edges, seed) of synth.make_pose_graph
FALSE_COV = np.diag([1e-3, 1e-3, 4e-4]).reshape(9)


def relative_pose(pa, pb):
    d, _ = spa.link_info(pa, pb, np.eye(3))
    return np.asarray(d)


def append_edge(g, a, b, z, cov):
    g = dict(g)
    g["edges"] = np.vstack([g["edges"], [[a, b]]]).astype(np.int32)
    g["z"] = np.vstack([g["z"], np.asarray(z, dtype=np.float64).reshape(1, 3)])
    g["cov"] = np.vstack([g["cov"], np.asarray(cov, dtype=np.float64).reshape(1, 9)])
    return g


def false_pairs(n):
    return ((2, n - 3), (n // 3, 2 * n // 3))


def with_false_closure(g, a, b):
    """one false closure appended: the true relative pose of (a, b) plus FALSE_OFFSET"""
    z = relative_pose(g["truth"][a], g["truth"][b]) + FALSE_OFFSET
    z[2] = spa.normalize_angle(z[2])
    return append_edge(g, a, b, z, FALSE_COV)


def solved(g, loss="None"):
    """the graph with `init` replaced by the poses of a tight dense solve"""
    opt = spa.Options.tight()
    opt.loss_function = loss
    x, info = spa.solve(g["init"], g["edges"], g["z"], g["cov"], opt)
    assert info["usable"]
    out = dict(g)
    out["init"] = x
    return out


@functools.lru_cache(maxsize=None)
def synthetic(k, false_pair=-1):
    n, e, seed = SYNTHETIC[k]
    g = synth.make_pose_graph(n, e, seed=seed)
    if false_pair >= 0:
        g = with_false_closure(g, *false_pairs(n)[false_pair])
    return solved(g)


def _closed_chain():
    g = cr.chain(12, closed=True)
    g["z"] = g["z"].copy()
    g["z"][-1] += [0.5, 0.3, 0.1]                 # the closing measurement disagrees with the odometry: a residual to share
    return solved(g)


def _gauge_ends():
    g = synth.make_pose_graph(12, 20, seed=2)
    assert (g["edges"][0] == [0, 1]).all()           # the gauge as a
    rng = np.random.default_rng(21)
    z = relative_pose(g["truth"][5], g["truth"][0]) + rng.normal(0, [0.01, 0.01, 0.003])
    return solved(append_edge(g, 5, 0, z, FALSE_COV))          # ... and as b


def _both_directions():
    g = synth.make_pose_graph(12, 20, seed=2)
    a, b = (int(v) for v in g["edges"][14])
    assert b > a + 1
    rng = np.random.default_rng(22)
    z = relative_pose(g["truth"][b], g["truth"][a]) + rng.normal(0, [0.01, 0.01, 0.003])
    return solved(append_edge(g, b, a, z, FALSE_COV))


def _weak_parallel():
    """an open chain whose edge 2 -> 3 has a parallel constraint with the information scaled by 1e-9: that copy is all that checks
    the edge, M = 1e-9 / (1 + 1e-9) of the identity, below min_redundancy -- unverifiable; the copy itself is checked by the edge"""
    g = cr.chain(5)
    g = append_edge(g, 2, 3, g["z"][2] + [0.03, -0.02, 0.01], g["cov"][2] * 1e9)
    return solved(g)


def _zero_residual():
    """a closed chain at its exact poses but for node 3, moved by 1/8 m along x: every product and difference is exact in binary, so
    the edges away from node 3 have a residual of exactly zero (FMA or none); audited as it stands, not solved"""
    g = cr.chain(6, closed=True)
    g["init"] = g["init"].copy()
    g["init"][3, 0] += 0.125
    return g


def _huber():
    g = synth.make_pose_graph(12, 20, seed=2)
    a, b = 3, 9
    z = relative_pose(g["truth"][a], g["truth"][b]) + [0.15, -0.1, 0.05]
    return solved(append_edge(g, a, b, z, FALSE_COV), loss="HuberLoss")


# name -> (builder, loss)
CASES = {
    "open chain 5": (lambda: cr.chain(5), "None"),
    "closed chain 12": (_closed_chain, "None"),
    "complete 24": (lambda: solved(cr.complete_graph(24)), "None"),
    "40/60": (lambda: synthetic(0), "None"),
    "40/60 false closure": (lambda: synthetic(0, 0), "None"),
    "gauge as a and as b": (_gauge_ends, "None"),
    "a->b and b->a": (_both_directions, "None"),
    "weak parallel": (_weak_parallel, "None"),
    "zero residual": (_zero_residual, "None"),
    "huber": (_huber, "HuberLoss"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    build, loss = CASES[name]
    return build(), loss
