"""The matcher's host half after it stopped building one distance-penalty table per job: the table of a search geometry is made once,
kept on the handle (a few entries, least recently used out first) and read by every job of every chunk from one device copy; the
positional covariance walks the lattice separably (csrc/covariance_walk.hpp).  Chunked batches (preset K, force_chunks, 150 matches
as in test_matcher_gpu.py::test_chunked_batch_equals_single) against one-at-a-time calls and against the CPU oracle, bit for bit."""
import numpy as np
import pytest

from common import PRESETS, Scenario, bits, make_hip_matcher, make_oracle_matcher

pytestmark = pytest.mark.gpu

N = 150
KH_OK, KH_ERR_SEARCH = 0, 4
ORACLE_FAILED = -1e9                                   # what the oracle returns where the reference throws (Mapper.cpp:786-796, 828)


def _assert_same(a, b, what):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert np.array_equal(bits(a), bits(b)), f"{what}: {a} vs {b} (max abs diff {np.max(np.abs(a - b))})"


def _assert_batch(batch, singles, what):
    resp, means, covs, status = batch
    assert (status == KH_OK).all(), what
    for i in range(len(resp)):
        r, m, c = singles[i % len(singles)]
        _assert_same(r, resp[i], f"{what}: response of match {i}")
        _assert_same(m, means[i], f"{what}: mean of match {i}")
        _assert_same(c, covs[i], f"{what}: covariance of match {i}")


@pytest.fixture(scope="module")
def scenarios():
    return [Scenario(seed=60 + i, n_base=5 + i % 4, start=23 * i + 2, perturb=(0.02 * i, -0.01 * i, 0.005 * i)) for i in range(8)]


@pytest.fixture(scope="module")
def pairs(scenarios):
    return [sc.hip_scans() for sc in scenarios]


def _chunked_handle():
    hm = make_hip_matcher("K", max_batch=N)
    hm.set_debug(False, force_chunks=True)             # small searches are not chunked on their own
    return hm


def _params(distance_variance_penalty, minimum_distance_penalty):
    return dict(PRESETS["K"]["params"], distance_variance_penalty=distance_variance_penalty, minimum_distance_penalty=minimum_distance_penalty)


def test_chunked_batch_after_set_params(kartohip_lib, scenarios, pairs):
    """The two distance-penalty parameters change between calls: every set is a new table for the coarse and for the fine geometry, more
    sets than the handle keeps, and the first set once more after its tables have been evicted."""
    from slam_toolbox_amd.scan_matcher import MapperParams
    sets = [(0.5, 0.5), (0.3, 0.6), (0.2, 0.4), (0.1, 0.7), (0.5, 0.5)]
    hm1, hmb, om = make_hip_matcher("K"), _chunked_handle(), make_oracle_matcher("K")
    qs = [pairs[i % 8][0] for i in range(N)]
    bs = [pairs[i % 8][1] for i in range(N)]
    seen = []
    for dvp, mdp in sets:
        p = _params(dvp, mdp)
        hm1.SetParams(MapperParams(**p))
        hmb.SetParams(MapperParams(**p))
        om.set_params(**p)
        singles = [hm1.MatchScan(q, b) for q, b in pairs]
        _assert_batch(hmb.MatchScanBatch(qs, bs), singles, f"penalties {dvp}, {mdp}")
        for k in (0, 5):                                # ... and both are the reference's
            r_o, mean_o, cov_o = om.match_scan(*scenarios[k].oracle_scans(), True, True)
            _assert_same(r_o, singles[k][0], "response against the oracle")
            _assert_same(mean_o, singles[k][1], "mean against the oracle")
            _assert_same(cov_o, singles[k][2], "covariance against the oracle")
        seen.append([r for r, _, _ in singles])
    # the parameters reach the results (a stale table would go unnoticed otherwise), and the first set gives its results again
    for a, b in zip(seen[:4], seen[1:4]):
        assert a != b
    assert seen[0] == seen[4]
    hm1.close()
    hmb.close()


def _resident(scenarios, pairs):
    """a chunked handle with the grids of the 150 matches in its slots; the queries and their centres"""
    from slam_toolbox_amd.scan_matcher import _scan_array
    hm = _chunked_handle()
    queries, centers = [], []
    for b in range(N):
        q, base = pairs[b % 8]
        hm.AddScans(q, base, slot=b)
        queries.append(q)
        centers.append(scenarios[b % 8].query_pose)
    return hm, queries, np.asarray(centers), (_scan_array(queries), N)


def test_two_geometries_alternating(kartohip_lib, scenarios, pairs):
    """Four chunked calls, two search geometries in turn (the second with nx != ny and res_x != res_y): each call finds its table
    where the call before last left it."""
    hm, queries, centers, arr = _resident(scenarios, pairs)
    p = PRESETS["K"]["params"]
    angles = (p["coarse_search_angle_offset"], p["coarse_angle_resolution"])
    geometries = [((0.15, 0.15), (0.02, 0.02)), ((0.1, 0.14), (0.01, 0.02))]
    singles = [[hm.CorrelateScan(queries[b], centers[b], *g, *angles, True, None, False, slot=b) for b in range(8)] for g in geometries]
    assert [r for r, _, _ in singles[0]] != [r for r, _, _ in singles[1]]
    for call in range(4):
        g = geometries[call % 2]
        _assert_batch(hm.CorrelateScanBatch(None, centers, *g, *angles, True, False, scan_array=arr), singles[call % 2], f"call {call}")
    hm.close()


def test_unpenalised_call_after_a_penalised_one(kartohip_lib, pairs):
    hm1, hmb = make_hip_matcher("K"), _chunked_handle()
    qs = [pairs[i % 8][0] for i in range(N)]
    bs = [pairs[i % 8][1] for i in range(N)]
    results = {}
    for penalize in (True, False, True):
        singles = [hm1.MatchScan(q, b, penalize, True) for q, b in pairs]
        _assert_batch(hmb.MatchScanBatch(qs, bs, penalize, True), singles, f"penalize {penalize}")
        results[penalize] = [r for r, _, _ in singles]
    assert results[True] != results[False]
    hm1.close()
    hmb.close()


def test_empty_grid_slot_in_a_chunked_batch(kartohip_lib, scenarios, pairs):
    """One match of the batch has no base scans: every pose of its searches ties at response 0 and the host walks the whole volume,
    with the pose offsets of the shared table.  That match and its neighbours against the oracle."""
    hmb, om = _chunked_handle(), make_oracle_matcher("K")
    empty = 70                                          # in the second chunk
    qs = [pairs[i % 8][0] for i in range(N)]
    bs = [[] if i == empty else pairs[i % 8][1] for i in range(N)]
    for _ in range(2):                                  # second pass: the table is the cached one
        resp, means, covs, status = hmb.MatchScanBatch(qs, bs)
        assert (status == KH_OK).all()
        for i in (0, empty - 1, empty, empty + 1, N - 1):
            oq, ob = scenarios[i % 8].oracle_scans()
            r_o, mean_o, cov_o = om.match_scan(oq, [] if i == empty else ob, True, True)
            _assert_same(r_o, resp[i], f"response of match {i}")
            _assert_same(mean_o, means[i], f"mean of match {i}")
            _assert_same(cov_o, covs[i], f"covariance of match {i}")
        assert resp[empty] == 0.0
    hmb.close()


def test_coarse_search_wider_than_the_search_size(kartohip_lib, scenarios, pairs):
    """Offsets beyond the matcher's search size put lattice poses outside the side x side probability grid: the reference throws
    (Mapper.cpp:786-796), the oracle reports it, the batch's status carries it for every match; the next call is untouched by it."""
    hm, queries, centers, arr = _resident(scenarios, pairs)
    p = PRESETS["K"]["params"]
    angles = (p["coarse_search_angle_offset"], p["coarse_angle_resolution"])
    om = make_oracle_matcher("K")
    oracle = {}
    for k in (0, 3):
        oq, ob = scenarios[k].oracle_scans()
        om.add_scans(oq, ob)
        for name, g in (("wide", ((0.2, 0.2), (0.02, 0.02))), ("wide in y", ((0.15, 0.17), (0.02, 0.02))), ("fits", ((0.15, 0.15), (0.02, 0.02)))):
            oracle[k, name] = (g, om.correlate_scan(oq, scenarios[k].query_pose, *g, *angles, True, False))
    for name in ("wide", "wide in y", "fits", "wide"):
        g = oracle[0, name][0]
        resp, means, covs, status = hm.CorrelateScanBatch(None, centers, *g, *angles, True, False, scan_array=arr)
        for k in (0, 3):
            r_o, mean_o, cov_o = oracle[k, name][1]
            want = KH_ERR_SEARCH if r_o == ORACLE_FAILED else KH_OK
            assert want == (KH_OK if name == "fits" else KH_ERR_SEARCH)          # the cases are what they are meant to be
            for i in range(k, N, 8):
                assert status[i] == want, (name, i)
            if want == KH_OK:
                _assert_same(r_o, resp[k], "response")
                _assert_same(mean_o, means[k], "mean")
                _assert_same(cov_o, covs[k], "covariance")
    hm.close()
