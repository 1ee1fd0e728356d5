"""GPU: marginalizing removal in the mapper (kh_mapper_set_removal_mode / kh_mapper_marginalize_nodes) over the 700-scan circuit
queue of tests/test_lifelong_policy_gpu.py, driven once under KH_REMOVE_MARGINALIZE and once under the default plain removal.

Marginalized, the alive scans form ONE component (union-find over kh_mapper_get_adjacency); the same queue in plain mode falls
into more than one, which also guards that the queue removes chain nodes at all.  The mapper's edges and the solver's constraints
correspond one to one, kh_mapper_num_edges counts them, kh_mapper_get_covariances answers for every alive scan (plain mode's
fragments make it refuse), and save -> load -> save is byte-identical."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from slam_toolbox_amd import capi, synth

pytestmark = pytest.mark.gpu

N_SCANS = 700


def _queue(n_scans):
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(n_scans)
    rng = np.random.default_rng(4)
    ranges = np.ascontiguousarray(np.stack([synth.make_scan(world, truth[i], rng) for i in range(n_scans)]))
    return ranges, np.ascontiguousarray(odom)


def _components(m):
    alive = [int(a) for a in m.alive()]
    parent = {a: a for a in alive}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a in alive:
        for b in m.adjacency(a):
            parent[find(a)] = find(int(b))
    return len({find(a) for a in alive})


def _run(ranges, odom, marginalize):
    from slam_toolbox_amd.mapper import Mapper
    m = Mapper(synth.Laser())
    m.SetLifelong(True)
    if marginalize:
        m.SetRemovalMode(True)
    for i in range(ranges.shape[0]):
        m.Process(ranges[i], odom[i], 0.1 * i)
    return m


@pytest.fixture(scope="module")
def mappers(kartohip_lib):
    ranges, odom = _queue(N_SCANS)
    marg, plain = _run(ranges, odom, True), _run(ranges, odom, False)
    yield marg, plain
    marg.close(); plain.close()


def test_the_marginalized_graph_stays_one_component(mappers):
    marg, plain = mappers
    st = marg.stats()
    n_plain, n_marg = _components(plain), _components(marg)
    print(f"[marginalize] {N_SCANS} scans: plain removal {plain.stats()['nodes_removed']} nodes -> {n_plain} components; marginalizing "
          f"{st['nodes_removed']} nodes ({st['marginalize_fallbacks']} plainly) -> {n_marg} components, lifelong_ms {st['lifelong_ms']:.1f} "
          f"against {plain.stats()['lifelong_ms']:.1f}")
    assert st["nodes_removed"] >= 20, "the queue does not exercise the decay"
    assert n_plain > 1, "the queue does not remove chain nodes: plain removal must split it"
    assert n_marg == 1
    assert plain.stats()["marginalize_fallbacks"] == 0


def _constraints(m):
    L = capi.lib()
    s = L.kh_mapper_solver(m._h)
    a, b, z, w = C.c_int32(), C.c_int32(), np.zeros(3), np.zeros(6)
    out = []
    for k in range(L.kh_spa_num_constraints(s)):
        capi.check(L.kh_spa_get_constraint(s, k, C.byref(a), C.byref(b), z, w), "kh_spa_get_constraint")
        out.append((a.value, b.value))
    return out


def test_edges_and_constraints_correspond(mappers):
    marg, _ = mappers
    alive = [int(a) for a in marg.alive()]
    ends = Counter()
    for a in alive:
        for b in marg.adjacency(a):
            assert int(b) in alive
            ends[frozenset((a, int(b)))] += 1
    cons = Counter(frozenset(c) for c in _constraints(marg))
    assert all(v % 2 == 0 for v in ends.values()), "an edge is missing from one of its two adjacency lists"
    assert {k: v // 2 for k, v in ends.items()} == dict(cons)
    assert marg.num_edges() == sum(cons.values()) == capi.lib().kh_spa_num_constraints(capi.lib().kh_mapper_solver(marg._h))


def test_covariances_answer_for_every_alive_scan(mappers):
    marg, plain = mappers
    cov = marg.covariances(marg.alive())
    assert cov.shape == (len(marg.alive()), 3, 3) and np.all(np.isfinite(cov))
    assert all(np.linalg.eigvalsh(0.5 * (c + c.T)).min() > 0.0 for a, c in zip(marg.alive(), cov) if a != 0)
    with pytest.raises(capi.KartoHipError):
        plain.covariances(plain.alive())


def test_session_round_trip_is_byte_identical(mappers, tmp_path):
    from slam_toolbox_amd.mapper import Mapper
    marg, _ = mappers
    marg.save(tmp_path / "a.khms")
    again = Mapper.load(tmp_path / "a.khms")
    again.save(tmp_path / "b.khms")
    assert open(tmp_path / "a.khms", "rb").read() == open(tmp_path / "b.khms", "rb").read()
    assert np.array_equal(again.alive(), marg.alive()) and again.num_edges() == marg.num_edges()
    again.close()


def test_explicit_call_mirrors_the_topology(kartohip_lib, tmp_path):
    """kh_mapper_marginalize_nodes on a short non-lifelong run: the scan leaves, its two neighbours are joined, the log has the
    C line of the new constraint before the E / D lines of the removal"""
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = _queue(40)
    log = str(tmp_path / "m.log")
    m = Mapper(synth.Laser(), log_path=log)
    for i in range(40):
        m.Process(ranges[i], odom[i], 0.1 * i)
    alive = [int(a) for a in m.alive()]
    v = alive[len(alive) // 3]
    nb = sorted(int(b) for b in m.adjacency(v))
    edges = m.num_edges()
    with pytest.raises(capi.KartoHipError):
        m.MarginalizeNodes([alive[-1]])                       # the last scan: refused like RemoveNode
    with pytest.raises(capi.KartoHipError):
        m.MarginalizeNodes([v, v])
    assert m.num_edges() == edges and v in m.alive()
    m.MarginalizeNodes([v])
    m.set_log(None)
    assert v not in m.alive() and _components(m) == 1
    assert m.num_edges() == len(_constraints(m))
    lines = [l.split() for l in open(log)]
    d = next(k for k, l in enumerate(lines) if l[0] == "D" and int(l[1]) == v)
    tail = [l[0] for l in lines[d - len(nb) - (len(set(nb)) - 1):d + 1]]
    assert len(set(nb)) >= 2 and tail == ["C"] * (len(set(nb)) - 1) + ["E"] * len(nb) + ["D"], tail
    m.close()
