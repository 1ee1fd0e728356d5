"""The search-space probabilities (per lattice cell the best response over the angles, ScanMatcher.search_probabilities) on both
scoring routes, bit for bit against the CPU oracle's response volume reduced over the angle axis.

On the LDS-staged route k_score_lds keeps them itself: its epilogue folds the workgroup's angles cell by cell and raises the cell in
the result block with an atomic maximum, and K4 is the tie scan alone (k_ties_only).  On every other route k_ties still derives them
from the stored sums (cell_maxima).  The cases (tests/cell_maxima_cases.py; tests/test_cell_maxima_cases_oracle.py proves on the CPU
that they sit where they must) run on a matcher with the LDS route forced and on one with the windowed route forced, every `pens`
value of the case; the all-invalid search follows a search with a non-zero lattice in the same slot (nothing may survive); batches
of 7, 8 and 9 cover the XCD mapping on and off and empty job slots, twice for byte-identical results; chunked batches put the two
side streams in play.

Mutant, run once on the device and not kept: k_score_lds with the epilogue's atomics left out.  31 of the 33 tests of this file
then failed at their LDS-route comparison (the lattice stays at K2's zero); the two that passed are the read-back before any search
and "every reading invalid", whose lattice IS all zeros.  K4 no longer supplies the lattice on the LDS route."""
import numpy as np
import pytest

import cell_maxima_cases as cm
import lds_cases as lc
from common import bits

pytestmark = pytest.mark.gpu

CASES = cm.picked()


def _same(a, b, what):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum()) if a.shape == b.shape else 'shapes'} differ"


class Rig:
    """one geometry: the matcher with the LDS route forced, the one with the windowed route forced, the oracle"""

    def __init__(self, case):
        self.om = case.oracle_matcher()
        self.lds = case.hip_matcher()
        self.win = case.hip_matcher()
        self.lds.set_debug(True, lds_score=True, dense_score=True)
        self.win.set_debug(True, windowed_score=True, dense_score=True)

    def search(self, hm, case, pen):
        hq = case.query.hip()
        hm.AddScans(hq, [b.hip() for b in case.base_scans()])
        centre, off, res, ang_off, ang_res = case.args()
        out = hm.CorrelateScan(hq, centre, off, res, ang_off, ang_res, pen, None, case.fine)
        return out, hm.search_probabilities()

    def check(self, case, pen):
        """the case on both routes against the oracle; returns the expected lattice"""
        want = lc.run_oracle(self.om, case, pen)
        lattice = cm.expected_lattice(self.om)
        for route, hm in (("LDS", self.lds), ("windowed", self.win)):
            got, probs = self.search(hm, case, pen)
            tag = f"{case.name} (pen={pen}), {route} route"
            _same(lattice, probs, f"search-space probabilities vs oracle, {tag}")
            for what, o, g in zip(("response", "mean", "covariance"), want, got):
                _same(o, g, f"{what} vs oracle, {tag}")
        return lattice

    def close(self):
        self.lds.close()
        self.win.close()


@pytest.fixture(scope="module")
def rigs(kartohip_lib):
    cache = {}

    def get(case):
        if case.geometry() not in cache:
            cache[case.geometry()] = Rig(case)
        return cache[case.geometry()]
    yield get
    for r in cache.values():
        r.close()


def test_no_coarse_search_yet(kartohip_lib):
    from slam_toolbox_amd import capi
    hm = CASES[0].hip_matcher()
    try:
        with pytest.raises(capi.KartoHipError) as e:
            hm.search_probabilities()
        assert e.value.code == capi.KH_ERR_NOT_FOUND
    finally:
        hm.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(rigs, case):
    rig = rigs(case)
    for pen in case.pens:
        lattice = rig.check(case, pen)
        assert lattice.any() == (case.name != cm.ALL_INVALID)


def test_same_slot_twice(rigs):
    """a search with a non-zero lattice, then "every reading invalid" in the same slot of the same matcher: all zeros, on both routes"""
    first = next(c for c in CASES if c.name == "one-cell lattice 61 x 64")
    second = next(c for c in CASES if c.name == cm.ALL_INVALID)
    assert first.geometry() == second.geometry()
    rig = rigs(first)
    assert rig.check(first, True).any()
    lattice = rig.check(second, True)
    assert lattice.shape == (second.want[1], second.want[0]) and not lattice.any()
    for hm in (rig.lds, rig.win):
        probs = hm.search_probabilities()
        assert probs.shape == lattice.shape and not probs.any(), "something of the earlier search survived"


def _batch(rig, jobs, copies=1, force_chunks=False):
    """the jobs, `copies` times over, in ONE CorrelateScanBatch on the LDS route, twice: every slot's lattice against the oracle, the
    second call byte-identical to the first"""
    n = len(jobs) * copies
    expect = []
    for j in jobs:
        want = lc.run_oracle(rig.om, j, True)
        expect.append((want, cm.expected_lattice(rig.om)))
    hmb = jobs[0].hip_matcher(max_batch=n)
    try:
        hmb.set_debug(False, lds_score=True, dense_score=True, force_chunks=force_chunks)
        hmb.profile(True)
        scans = [jobs[i % len(jobs)].query.hip() for i in range(n)]
        for i in range(n):
            hmb.AddScans(scans[i], [b.hip() for b in jobs[i % len(jobs)].base_scans()], slot=i)
        _, off, res, ang_off, ang_res = jobs[0].args()
        centres = np.array([jobs[i % len(jobs)].centre for i in range(n)])
        runs = []
        for _ in range(2):
            hmb.score_loads()
            resp, means, covs, status = hmb.CorrelateScanBatch(scans, centres, off, res, ang_off, ang_res, True, False)
            assert hmb.score_loads() > 0 and (status == 0).all()
            runs.append((resp.copy(), means.copy(), covs.copy(), [hmb.search_probabilities(slot=i) for i in range(n)]))
        for i in range(n):
            (r, m, c), lattice = expect[i % len(jobs)]
            _same(lattice, runs[0][3][i], f"search-space probabilities of job {i} of {n} vs oracle")
            for what, o, g in zip(("response", "mean", "covariance"), (r, m, c), (runs[0][0][i], runs[0][1][i], runs[0][2][i])):
                _same(o, np.asarray(g).reshape(np.asarray(o).shape), f"{what} of job {i} of {n} vs oracle")
        for k, what in enumerate(("response", "mean", "covariance")):
            assert runs[0][k].tobytes() == runs[1][k].tobytes(), f"{what}: the second call differs"
        for i in range(n):
            assert runs[0][3][i].tobytes() == runs[1][3][i].tobytes(), f"lattice of job {i}: the second call differs"
    finally:
        hmb.close()


@pytest.mark.parametrize("n", [7, 8, 9])
def test_batch(rigs, n):
    jobs = lc.batch_jobs(n)
    _batch(rigs(jobs[0]), jobs)


@pytest.mark.parametrize("copies", [1, 16])
def test_forced_chunking(rigs, copies):
    """force_chunks: a batch of 8, and -- the library chunks batches of 128 and more only -- the same 8 searches sixteen times over
    in one call of 128, which goes through as 24 + 64 + 40 on the two side streams"""
    jobs = lc.batch_jobs(8)
    _batch(rigs(jobs[0]), jobs, copies=copies, force_chunks=True)
