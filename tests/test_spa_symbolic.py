"""CPU: the solver's symbolic analysis (csrc/spa_symbolic.cpp: nested dissection with vertex-cover separators, supernode
chains, assembly tree, level numbering) checked against a plain symbolic Cholesky of the same ordering: every front's
row structure must equal the true structure of its first column's L pattern, children must sit on lower levels with
contiguous front ids per level, and the child -> parent position maps must point at the same elimination positions.
And the device-free stages of the problem setup around it (csrc/spa_problem_plan.hpp: edge endpoints, free numbering, BSR
pattern, contribution lists, slot destinations, reuse of cached supernodes) against a plain numpy restatement.  Both through
tools/sym_probe.cpp, built with the address and undefined-behaviour sanitizers where the compiler has them."""
import os
import subprocess

import numpy as np
import pytest

from slam_toolbox_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["free_of_elim", "front_first", "front_ns", "front_m", "level", "parent", "rows_ptr", "rows", "child_ptr", "child_list",
         "relpos_ptr", "relpos", "cinv_ptr", "cinv",
         "free_of_node", "ea", "eb", "row_ptr", "col", "slot_row", "diag", "slot_ptr", "slot_list", "node_ptr", "node_list",
         "slot_dest", "slot_ld", "front_off", "sn_of_elim", "reuse_ptr", "reuse_idx", "reuse_placed"]
INT64 = ("slot_dest", "front_off")


@pytest.fixture(scope="module")
def probe_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe") / "sym_probe")
    base = ["g++", "-O1", "-g", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "sym_probe.cpp"),
            os.path.join(ROOT, "slam_toolbox_amd", "csrc", "spa_symbolic.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, timeout=600).returncode != 0:
        subprocess.run(base, check=True, timeout=600)              # a compiler without the sanitizers' runtimes
    return exe


def _probe(exe, tmp_path, edges, n_nodes, args=(), ids=None, cached=None, threads=None):
    """ids: the nodes' ids in insertion order (default 0..n-1; the first is the gauge); cached: supernodes of an earlier
    dissection as lists of node ids; threads: the plan's parallel loops on that many plain threads"""
    ef = str(tmp_path / "edges.bin")
    np.asarray(edges, dtype=np.int32).tofile(ef)
    dump = str(tmp_path / "sym.bin")
    env = dict(os.environ, SYM_PROBE_DUMP=dump, SYM_PROBE_REPS="1")
    if ids is not None:
        env["SYM_PROBE_IDS"] = str(tmp_path / "ids.bin")
        np.asarray(ids, dtype=np.int32).tofile(env["SYM_PROBE_IDS"])
    if cached is not None:
        env["SYM_PROBE_CACHED"] = str(tmp_path / "cached.bin")
        np.asarray([v for sn in cached for v in [len(sn)] + list(sn)], dtype=np.int32).tofile(env["SYM_PROBE_CACHED"])
    if threads:
        env["SYM_PROBE_THREADS"] = str(threads)
    out = subprocess.run([exe, ef, str(n_nodes)] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(dump, dtype=np.int32)
    arrays, p = [], 0
    while p < raw.size:
        n = int(raw[p]); arrays.append(raw[p + 1:p + 1 + n]); p += 1 + n
    assert len(arrays) == len(NAMES)
    sym = dict(zip(NAMES, arrays))
    for name in INT64:
        sym[name] = sym[name].copy().view(np.int64)
    return sym


def _check(sym, edges, n_nodes):
    fon = sym["free_of_node"]                           # the first node is the gauge, nodes without constraints are not in the problem
    assert len(fon) == n_nodes
    N = int(fon.max()) + 1
    perm = sym["free_of_elim"]
    assert sorted(perm.tolist()) == list(range(N)), "not a permutation"
    pos = np.empty(N, dtype=np.int64); pos[perm] = np.arange(N)
    adj = [set() for _ in range(N)]
    for a, b in zip(sym["ea"].tolist(), sym["eb"].tolist()):
        a = fon[a]; b = fon[b]
        if a >= 0 and b >= 0 and a != b:
            adj[pos[a]].add(pos[b]); adj[pos[b]].add(pos[a])
    # plain symbolic factorisation in elimination positions
    struct = [None] * N
    kids = [[] for _ in range(N)]
    for j in range(N):
        s = {w for w in adj[j] if w > j}
        for c in kids[j]:
            s |= struct[c]
        s.discard(j)
        struct[j] = s
        if s:
            kids[min(s)].append(j)
    K = len(sym["front_first"])
    first, ns, m, level, parent = sym["front_first"], sym["front_ns"], sym["front_m"], sym["level"], sym["parent"]
    covered = np.zeros(N, dtype=bool)
    padding = total_rows = 0
    for k in range(K):
        ncols = ns[k] // 3
        assert ns[k] % 3 == 0 and 1 <= ncols <= 42
        cols = range(first[k], first[k] + ncols)
        assert not covered[list(cols)].any(); covered[list(cols)] = True
        rows = sym["rows"][sym["rows_ptr"][k]:sym["rows_ptr"][k + 1]]
        assert m[k] == 3 * (ncols + len(rows))
        assert np.all(np.diff(rows) > 0) and (len(rows) == 0 or rows[0] >= first[k] + ncols)
        # a supernode's rows = the structure of its first column beyond the supernode, which must contain every later
        # column's structure (dense trapezoid); equality with the first column = no padding beyond the supernode's own rule
        true_first = {w for w in struct[first[k]] if w >= first[k] + ncols}
        union = set()
        for c in cols:
            union |= {w for w in struct[c] if w >= first[k] + ncols}
        assert union <= set(rows.tolist()), f"front {k}: fill outside its rows"
        # a supernode is treated as dense: rows beyond the true structure are explicit zeros (a separator is not always a
        # clique after its halves are gone, and a part of a split chain carries the whole chain's rows), counted below
        padding += len(rows) - len(union)
        total_rows += len(rows)
        assert true_first <= union
        # parent = front of the first row; relpos maps every row to that elimination position inside the parent
        if len(rows):
            p = parent[k]
            assert p >= 0 and first[p] <= rows[0] < first[p] + ns[p] // 3
            assert level[p] > level[k]
            prow = sym["rows"][sym["rows_ptr"][p]:sym["rows_ptr"][p + 1]]
            ppos = np.concatenate([np.arange(first[p], first[p] + ns[p] // 3), prow])
            rel = sym["relpos"][sym["relpos_ptr"][k]:sym["relpos_ptr"][k + 1]]
            assert np.array_equal(ppos[rel], rows) and np.all(np.diff(rel) > 0)
            assert k in sym["child_list"][sym["child_ptr"][p]:sym["child_ptr"][p + 1]]
        else:
            assert parent[k] == -1
    assert covered.all()
    # gather maps = inverse of relpos per (front, child)
    for k in range(K):
        mp = m[k] // 3
        kids_k = sym["child_list"][sym["child_ptr"][k]:sym["child_ptr"][k + 1]]
        assert sym["cinv_ptr"][k + 1] - sym["cinv_ptr"][k] == len(kids_k) * mp
        for s_, c in enumerate(kids_k):
            inv = sym["cinv"][sym["cinv_ptr"][k] + s_ * mp:sym["cinv_ptr"][k] + (s_ + 1) * mp]
            rel = sym["relpos"][sym["relpos_ptr"][c]:sym["relpos_ptr"][c + 1]]
            assert np.array_equal(np.nonzero(inv >= 0)[0], rel) and np.array_equal(inv[rel], np.arange(len(rel)))
    assert padding <= 0.1 * max(1, total_rows), (padding, total_rows)
    assert np.all(np.diff(level) >= 0), "front ids are not level by level"
    for l in range(level.max() + 1):
        ids = np.nonzero(level == l)[0]
        assert np.all(np.diff(m[ids]) <= 0), "fronts of a level are not sorted by size"


def _check_plan(sym, edges, ids, cached=None):
    """the plan's arrays against a plain restatement: endpoints and free numbering from the ids, each row's sorted unique neighbours
    with the diagonal in its sorted place, per slot the ascending e * 4 + kind, per node the ascending e * 2 + role, slot_dest from
    the dumped structure (-1 above the diagonal in elimination order), and the cached supernodes as ascending free indices"""
    ids = [int(v) for v in ids]
    pos_of_id = {v: i for i, v in enumerate(ids)}
    assert len(pos_of_id) == len(ids)
    edges = [(int(a), int(b)) for a, b in edges]
    ea = np.array([pos_of_id[a] for a, _ in edges], dtype=np.int64); eb = np.array([pos_of_id[b] for _, b in edges], dtype=np.int64)
    assert np.array_equal(sym["ea"], ea) and np.array_equal(sym["eb"], eb)
    used = np.zeros(len(ids), dtype=bool); used[ea] = True; used[eb] = True
    free = [i for i in range(len(ids)) if used[i] and i != 0]
    fon = np.full(len(ids), -1, dtype=np.int64); fon[free] = np.arange(len(free))
    assert np.array_equal(sym["free_of_node"], fon)
    nf = len(free)
    fa, fb = fon[ea], fon[eb]
    rows = [{i} for i in range(nf)]
    for a, b in zip(fa.tolist(), fb.tolist()):
        if a >= 0 and b >= 0 and a != b:
            rows[a].add(b); rows[b].add(a)
    rows = [sorted(r) for r in rows]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    assert np.array_equal(sym["row_ptr"], row_ptr)
    assert np.array_equal(sym["col"], np.concatenate(rows))
    assert np.array_equal(sym["slot_row"], np.repeat(np.arange(nf), np.diff(row_ptr)))
    assert np.array_equal(sym["diag"], [row_ptr[i] + r.index(i) for i, r in enumerate(rows)])
    n_slots = int(row_ptr[-1])
    slot = {(i, j): int(row_ptr[i]) + q for i, r in enumerate(rows) for q, j in enumerate(r)}
    by_slot, by_node = [], []
    for e, (a, b) in enumerate(zip(fa.tolist(), fb.tolist())):
        if a >= 0:
            by_slot.append((slot[a, a], e * 4 + 0)); by_node.append((a, e * 2 + 0))
        if b >= 0:
            by_slot.append((slot[b, b], e * 4 + 1)); by_node.append((b, e * 2 + 1))
        if a >= 0 and b >= 0 and a != b:
            by_slot.append((slot[a, b], e * 4 + 2)); by_slot.append((slot[b, a], e * 4 + 3))
    for pairs, n, ptr, lst in ((by_slot, n_slots, "slot_ptr", "slot_list"), (by_node, nf, "node_ptr", "node_list")):
        pairs = sorted(pairs)                           # ascending value within every slot / node
        where = np.array([p[0] for p in pairs], dtype=np.int64)
        assert np.array_equal(sym[ptr], np.concatenate([[0], np.cumsum(np.bincount(where, minlength=n))]))
        assert np.array_equal(sym[lst], [p[1] for p in pairs])
    # where every block lands in its front
    first, ns, m = sym["front_first"], sym["front_ns"], sym["front_m"]
    assert np.array_equal(sym["front_off"], np.concatenate([[0], np.cumsum(m.astype(np.int64) ** 2)])[:-1])
    sn_of_elim = np.repeat(np.arange(len(first)), ns // 3)[np.argsort(np.repeat(first, ns // 3) + np.concatenate([np.arange(c) for c in ns // 3]))]
    assert np.array_equal(sym["sn_of_elim"], sn_of_elim)
    elim = np.empty(nf, dtype=np.int64); elim[sym["free_of_elim"]] = np.arange(nf)
    dest = np.full(n_slots, -1, dtype=np.int64); ld = np.zeros(n_slots, dtype=np.int64)
    for k in range(n_slots):
        ei, ej = int(elim[sym["slot_row"][k]]), int(elim[sym["col"][k]])
        if ei < ej:
            continue
        f = int(sn_of_elim[ej]); ncols = int(ns[f]) // 3
        if ei < first[f] + ncols:
            rowpos = ei - int(first[f])
        else:
            front_rows = sym["rows"][sym["rows_ptr"][f]:sym["rows_ptr"][f + 1]].tolist()
            rowpos = ncols + front_rows.index(ei)
        dest[k] = int(sym["front_off"][f]) + 3 * rowpos + 3 * (ej - int(first[f])) * int(m[f]); ld[k] = m[f]
    assert np.array_equal(sym["slot_dest"], dest) and np.array_equal(sym["slot_ld"], ld)
    assert np.all(dest[sym["diag"]] >= 0) and (n_slots - np.count_nonzero(dest < 0)) * 2 - nf == n_slots
    if cached is not None:
        free_of_id = {ids[p]: f for f, p in enumerate(free)}
        want = [sorted(free_of_id[v] for v in sn if v in free_of_id) for sn in cached]
        want = [g for g in want if g]
        got = [sym["reuse_idx"][sym["reuse_ptr"][k]:sym["reuse_ptr"][k + 1]].tolist() for k in range(len(sym["reuse_ptr"]) - 1)]
        assert got == want
        placed = np.zeros(nf, dtype=np.int64); placed[[f for g in want for f in g]] = 1
        assert np.array_equal(sym["reuse_placed"][:-1], placed) and sym["reuse_placed"][-1] == sum(len(g) for g in want)


@pytest.mark.parametrize("n,e,seed,args", [(60, 100, 2, ()), (700, 1800, 3, ()), (3000, 9000, 4, ()), (3000, 9000, 4, (4, 5, 2)),
                                           (2000, 1999, 5, ())])
def test_symbolic_structure(probe_exe, tmp_path, n, e, seed, args):
    g = synth.make_pose_graph(n, e, seed=seed)
    # an earlier dissection by node id: blocks of 37 ids, some of nodes that have left (beyond n), the last 50 nodes new
    cached = [list(range(k, k + 37)) for k in range(n + 60, -1, -37)]
    cached = [[v for v in sn if v < n - 50 or v >= n] for sn in cached]
    sym = _probe(probe_exe, tmp_path, g["edges"], n, args, cached=cached, threads=3 if n == 3000 else None)
    _check(sym, g["edges"], n)
    _check_plan(sym, g["edges"], range(n), cached)
    if n == 3000:                                       # more than one block of rows (1024) and of slots (8192)
        assert sym["free_of_node"].max() + 1 == 2999 and len(sym["col"]) > 2 * 8192


def test_symbolic_clique_is_a_chain_of_fronts(probe_exe, tmp_path):
    n = 151
    edges = [(i, j) for i in range(n) for j in range(i + 1, n)]
    sym = _probe(probe_exe, tmp_path, edges, n)
    _check(sym, edges, n)
    _check_plan(sym, edges, range(n))
    assert len(sym["front_first"]) == 4 and sym["level"].tolist() == [0, 1, 2, 3]       # 150 pivots nodes -> 38 + 38 + 38 + 36
    assert sym["front_ns"].max() <= 126


SPARSE_IDS = [7, -3, 2 ** 31 - 1, -2 ** 31, 1000000, 40, -41, 5]
PLAN_EDGE_CASES = {
    # the smallest graphs at which a stage of the plan can go wrong: (ids in insertion order, edges by id, cached supernodes)
    "one_free_node": ([0, 1], [(0, 1)], [[1], [9]]),
    "gauge_with_two_edges": ([0, 1, 2, 3], [(1, 0), (0, 3), (1, 2), (2, 3)], None),
    "unconstrained_node_mid_range": ([0, 1, 2, 3, 4], [(0, 1), (1, 3), (3, 4), (4, 1)], [[2, 3], [1, 4, 0]]),
    "same_pair_both_directions": ([0, 1, 2], [(1, 2), (0, 1), (2, 1)], None),
    # ids that miss both tables: the hashed paths of the endpoint lookup and of the supernode reuse
    "sparse_and_negative_ids": (SPARSE_IDS, [(SPARSE_IDS[k], SPARSE_IDS[k + 1]) for k in range(7)] + [(5, -3), (-2 ** 31, 40), (-3, 5)],
                                [[5, -41, 123456], [-2 ** 31, 2 ** 31 - 1], [77], [-3, 7]]),
}


@pytest.mark.parametrize("case", sorted(PLAN_EDGE_CASES))
def test_problem_plan_edge_cases(probe_exe, tmp_path, case):
    ids, edges, cached = PLAN_EDGE_CASES[case]
    sym = _probe(probe_exe, tmp_path, edges, len(ids), ids=ids, cached=cached)
    _check(sym, edges, len(ids))
    _check_plan(sym, edges, ids, cached)
    n_free = {"one_free_node": 1, "gauge_with_two_edges": 3, "unconstrained_node_mid_range": 3, "same_pair_both_directions": 2,
              "sparse_and_negative_ids": 7}[case]
    assert sym["free_of_node"].max() + 1 == n_free
