"""Front shapes of the covariance kernels (csrc/spa_selinv.hip: k_selinv_head / _z21 / _z11, csrc/spa_cov_columns.hip: k_cov_columns_forward / _backward and
the gathers around them) as plain data: the graphs whose multifrontal analysis yields fronts at the edges of the kernels' tiles.
tests/test_covariance_cases_oracle.py checks on the CPU (tools/sym_probe.cpp, the library's own analysis) that every case still
has the shapes it claims and that the table covers every class; tests/test_covariance_shapes_gpu.py runs the table through the library
against the dense rule of tests/covariance_rule.py.

Two families, built like covariance_rule.complete_graph (random true poses, every listed pair joined by a noisy spa.link_info
measurement of covariance diag(0.01, 0.01, 0.004), node 0 the gauge):
  clique(n)         every pair of n nodes
  petals(s, l, k)   a clique of s nodes (node 0 among them) and k groups of l nodes, each group fully linked inside and to all s
                    nodes, no links between groups: the s nodes are the separator the analysis finds, every group a front below it

A case is (name, build, leaf, shapes, claims): leaf is the KH_SPA_LEAF value the handle's analysis reads (None: the default), shapes
the set of its fronts' (ns, nu), a front's pivot count and the size of its update block nu = m - ns, claims the classes of CLASSES
below that the case is in the table for.  Every case but the wide level stays at or below covariance_rule.LD_MAX_FREE free nodes,
so that the long-double restatement (b) of the rule applies.

A small ns together with nu >= 129 is not in the table: the analysis merges a small separator under a large update block into its
neighbour (a chain is cut into even parts), so no graph of these families yields one.

Front shapes (sym_probe at the default options) and the tolerance inputs, measured by tests/test_covariance_cases_oracle.py from the
reference alone, at the initial poses (eps = 2^-52; the bound on the library is max(8 * max(ref_err, order_err), 64 eps), the
convention of covariance_rule.tolerance and spa_cases.ORDER_ERR; the test asserts max(ref_err, order_err) <= 1e-12 for every case):

  case                       free  fronts (ns, nu)                                       ref_err order_err bound     columns: ref_err order_err bound
  clique 44                    43  (63, 0) (66, 63)                                      5.9e-15 2.2e-15 4.7e-14            3.8e-15 1.5e-15 3.0e-14
  clique 45                    44  (66, 0) (66, 66)                                      6.0e-15 3.4e-15 4.8e-14            3.6e-15 2.2e-15 2.8e-14
  clique 85                    84  (126, 0) (126, 126)                                   5.1e-15 4.1e-15 4.1e-14            2.4e-15 2.4e-15 2.0e-14
  clique 86                    85  (81, 0) (87, 81) (87, 168)                            1.3e-14 5.2e-15 1.0e-13            5.6e-15 2.7e-15 4.5e-14
  petals(2, 42, 2)             85  (3, 0) 2 x (126, 3)                                   5.7e-15 4.2e-15 4.6e-14            2.9e-15 2.3e-15 2.3e-14
  petals(6, 40, 3)            125  (15, 0) 3 x (120, 15)                                 5.4e-15 6.6e-15 5.3e-14            1.8e-15 2.6e-15 2.1e-14
  petals(8, 36, 2)             79  (21, 0) 2 x (108, 21)                                 5.0e-15 3.9e-15 4.0e-14            2.5e-15 1.6e-15 2.0e-14
  petals(12, 38, 2)            87  (33, 0) 2 x (114, 33)                                 4.3e-15 4.4e-15 3.5e-14            2.5e-15 2.1e-15 2.0e-14
  petals(5, 16, 3) leaf 4      52  (12, 0) 3 x (48, 12)                                  1.7e-15 2.5e-15 2.0e-14            9.1e-16 1.3e-15 1.4e-14
  petals(33, 16, 2)            64  (96, 0) (96, 96)                                      3.1e-15 3.1e-15 2.5e-14            1.4e-15 1.5e-15 1.4e-14
  petals(44, 30, 2)           103  (99, 0) (105, 99) (105, 204)                          3.0e-15 6.2e-15 5.0e-14            2.1e-15 2.6e-15 2.0e-14
  petals(190, 1, 2)           191  (105, 0) (117, 105) (117, 222) (117, 339) (117, 456)  1.4e-14 3.8e-14 3.0e-13            8.5e-15 1.2e-14 9.6e-14
  petals(3, 2, 300) leaf 1    602  (6, 0) 300 x (6, 6) on one level                      3.4e-14 2.3e-15 2.7e-13            6.6e-15 1.9e-15 5.3e-14

The first three figures are in the marginals' measure (a diagonal or edge block, relative to the block: covariance_rule.ref_err), the
last three in the columns' measure (any block, relative to sqrt(|Sigma_ii|_F |Sigma_qq|_F): covariance_columns_rule).  The two chains
that petals(44, 30, 2) and petals(190, 1, 2) turn into are the analysis's doing: separator and petals end up in one supernode chain.
The GPU test measures the same figures again at the poses the solver holds; those and the library's errors are in DESIGN.md.
"""
from collections import namedtuple

import numpy as np

import covariance_columns_rule as ccr
import covariance_rule as cr
from oracle import spa

Case = namedtuple("Case", "name build leaf shapes claims")

REF_CEILING = 1e-12          # max(ref_err, order_err) of every case stays below this: no bound wide enough to hide a wrong tail entry


def _graph(n, pairs, seed):
    rng = np.random.default_rng(seed)
    truth = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-3, 3, n)])
    edges = np.array(pairs)
    cov = np.tile(np.diag([0.01, 0.01, 0.004]).reshape(1, 9), (len(edges), 1))
    z = np.zeros((len(edges), 3))
    for e, (i, j) in enumerate(edges):
        d, _ = spa.link_info(truth[i], truth[j], np.eye(3))
        z[e] = np.asarray(d) + rng.normal(0, [0.02, 0.02, 0.01])
    init = truth + rng.normal(0, 0.02, truth.shape)
    init[0] = truth[0]
    return dict(init=init, edges=edges, z=z, cov=cov)


def clique(n, seed=3):
    return _graph(n, [(i, j) for i in range(n) for j in range(i + 1, n)], seed)


def petal_nodes(s, l, k):
    """the k groups' node lists"""
    return [list(range(s + g * l, s + (g + 1) * l)) for g in range(k)]


def petals(s, l, k, seed=3):
    pairs = [(i, j) for i in range(s) for j in range(i + 1, s)]
    for group in petal_nodes(s, l, k):
        pairs += [(i, j) for i in range(s) for j in group]
        pairs += [(i, j) for a, i in enumerate(group) for j in group[a + 1:]]
    return _graph(s + l * k, pairs, seed)


def shapes(sym):
    """the set of (ns, nu) of an analysis dumped by sym_probe (tests/test_spa_symbolic.py: _probe)"""
    return {(int(ns), int(m - ns)) for ns, m in zip(sym["front_ns"], sym["front_m"])}


# ---- classes: name -> predicate on the list of fronts [(ns, nu, level, parent index)] --------------------------------------------
def _ns(pred):
    return lambda fronts: any(pred(f[0]) for f in fronts)


def _nu(pred):
    return lambda fronts: any(pred(f[1]) for f in fronts)


def _chain(fronts):
    """three fronts child -> parent -> grandparent of which the two lower ones have an update block: the middle one's Z22 is
    gathered from a Z22 that was itself gathered"""
    for ns, nu, _, parent in fronts:
        if nu > 0 and parent >= 0 and fronts[parent][1] > 0 and fronts[parent][3] >= 0:
            return True
    return False


def _wide(fronts):
    count = {}
    for ns, nu, level, _ in fronts:
        if nu > 0:
            count[level] = count.get(level, 0) + 1
    return any(c > 256 for c in count.values())


CLASSES = {
    "ns 3": _ns(lambda v: v == 3), "ns 4..15": _ns(lambda v: 4 <= v <= 15), "ns 48": _ns(lambda v: v == 48),
    "ns 96": _ns(lambda v: v == 96), "ns 97..111": _ns(lambda v: 97 <= v <= 111), "ns 113..125": _ns(lambda v: 113 <= v <= 125),
    "ns 126": _ns(lambda v: v == 126),
    "nu 0": _nu(lambda v: v == 0), "nu 3": _nu(lambda v: v == 3), "nu 4..15": _nu(lambda v: 4 <= v <= 15),
    "nu 16k": _nu(lambda v: v > 0 and v % 16 == 0), "nu 113..128": _nu(lambda v: 113 <= v <= 128),
    "nu 129..256": _nu(lambda v: 129 <= v <= 256), "nu > 384": _nu(lambda v: v > 384),
    "chain": _chain, "wide level": _wide,
}
for _r in range(8):
    CLASSES[f"ns mod 8 = {_r}"] = _ns(lambda v, r=_r: v % 8 == r)
    CLASSES[f"nu mod 8 = {_r}"] = _nu(lambda v, r=_r: v % 8 == r)


def fronts_of(sym):
    return [(int(ns), int(m - ns), int(level), int(parent))
            for ns, m, level, parent in zip(sym["front_ns"], sym["front_m"], sym["level"], sym["parent"])]


CASES = [
    Case("clique 44", lambda: clique(44), None, ((63, 0), (66, 63)),
         ("ns mod 8 = 7", "nu mod 8 = 7", "ns mod 8 = 2")),
    Case("clique 45", lambda: clique(45), None, ((66, 0), (66, 66)),
         ("nu mod 8 = 2",)),
    Case("clique 85", lambda: clique(85), None, ((126, 0), (126, 126)),
         ("ns 126", "nu 113..128", "ns mod 8 = 6", "nu mod 8 = 6")),
    Case("clique 86", lambda: clique(86), None, ((81, 0), (87, 81), (87, 168)),
         ("nu 129..256", "chain", "nu mod 8 = 1", "nu mod 8 = 0")),
    Case("petals(2, 42, 2)", lambda: petals(2, 42, 2), None, ((3, 0), (126, 3)),
         ("ns 3", "ns 126", "nu 3", "nu 0", "ns mod 8 = 3", "nu mod 8 = 3")),
    Case("petals(6, 40, 3)", lambda: petals(6, 40, 3), None, ((15, 0), (120, 15)),
         ("ns 4..15", "ns 113..125", "nu 4..15", "ns mod 8 = 0")),
    Case("petals(8, 36, 2)", lambda: petals(8, 36, 2), None, ((21, 0), (108, 21)),
         ("ns 97..111", "nu mod 8 = 5", "ns mod 8 = 5", "ns mod 8 = 4")),
    Case("petals(12, 38, 2)", lambda: petals(12, 38, 2), None, ((33, 0), (114, 33)),
         ("ns 113..125", "ns mod 8 = 1", "ns mod 8 = 2", "nu mod 8 = 1")),
    Case("petals(5, 16, 3) leaf 4", lambda: petals(5, 16, 3), 4, ((12, 0), (48, 12)),
         ("ns 48", "ns 4..15", "nu 4..15", "ns mod 8 = 4", "nu mod 8 = 4")),
    Case("petals(33, 16, 2)", lambda: petals(33, 16, 2), None, ((96, 0), (96, 96)),
         ("ns 96", "nu 16k")),
    Case("petals(44, 30, 2)", lambda: petals(44, 30, 2), None, ((99, 0), (105, 99), (105, 204)),
         ("ns 97..111", "nu 129..256", "chain", "ns mod 8 = 3", "ns mod 8 = 1", "nu mod 8 = 4")),
    Case("petals(190, 1, 2)", lambda: petals(190, 1, 2), None, ((105, 0), (117, 105), (117, 222), (117, 339), (117, 456)),
         ("ns 113..125", "nu > 384", "nu 129..256", "chain", "ns mod 8 = 5")),
    Case("petals(3, 2, 300) leaf 1", lambda: petals(3, 2, 300), 1, ((6, 0), (6, 6)),
         ("wide level", "ns 4..15", "nu 4..15", "ns mod 8 = 6", "nu mod 8 = 6")),
]
WIDE = "petals(3, 2, 300) leaf 1"
CHAIN5 = "petals(190, 1, 2)"
BY_NAME = {c.name: c for c in CASES}
_GRAPHS = {}


def graph(name):
    """the case's graph, built once per process and shared: read-only for its users"""
    if name not in _GRAPHS:
        _GRAPHS[name] = BY_NAME[name].build()
    return _GRAPHS[name]


# ---- the tolerance inputs, from the reference alone ---------------------------------------------------------------------------------
Measure = namedtuple("Measure", "rule ref_err order_err col_ref_err col_order_err")


def block_errors(got, want, scale):
    """(n, n): |got - want|_F of every 3 x 3 block over sqrt(|Sigma_ii|_F |Sigma_jj|_F), the measure of covariance_columns_rule"""
    n = len(scale)
    d = np.asarray(np.asarray(got, dtype=cr.LD) - np.asarray(want, dtype=cr.LD), dtype=np.float64).reshape(n, 3, n, 3)
    return np.sqrt(np.sum(d * d, axis=(1, 3))) / np.sqrt(np.outer(scale, scale))


def measure(g, poses=None):
    """rule (a) at `poses` (None: the initial ones) with rule (b) for EVERY block in sigma_ref (np.linalg.inv above LD_MAX_FREE
    free nodes), and how far (a) is from (b) and from (a) under the reverse node order: ref_err / order_err on the diagonal and edge
    blocks relative to the block (covariance_rule.ref_err, the marginals' measure), col_* on every block in the columns' measure"""
    x = g["init"] if poses is None else poses
    r = cr.rule(x, g["edges"], g["z"], cov=g["cov"], reference=False)
    ref = cr.inverse_longdouble(r.H) if r.problem.nfree <= cr.LD_MAX_FREE else np.linalg.inv(r.H)
    r = r._replace(sigma_ref=ref)
    rev = cr.inverse_float64_reversed(r.H)
    scale = ccr.scales(r.sigma)
    return Measure(r, cr.ref_err(r), cr.order_err(r, reversed_sigma=rev), float(block_errors(r.sigma, ref, scale).max()),
                   float(block_errors(r.sigma, rev, scale).max()))


def bounds(ms):
    """(bound on a diagonal or edge block relative to the block, bound on any block in the columns' measure)"""
    return cr.tolerance(max(ms.ref_err, ms.order_err)), cr.tolerance(max(ms.col_ref_err, ms.col_order_err))


def other_petal_pair(name):
    """two nodes of different petals (no constraint joins them), or None for a clique"""
    if not name.startswith("petals"):
        return None
    s, l, k = (int(v) for v in name[name.index("(") + 1:name.index(")")].split(","))
    groups = petal_nodes(s, l, k)
    return groups[0][l // 2], groups[-1][-1]
