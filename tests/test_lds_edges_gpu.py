"""The LDS-staged scoring kernels (k_offsets_lds / k_score_lds, csrc/matcher_kernels.hip) at their chunk and lattice edges: every case of
tests/lds_cases.py (tests/test_lds_cases_oracle.py proves on the CPU that each sits on its edge) through a matcher with the path forced
(dense scoring, profiling on), a second one on the windowed kernel and the CPU oracle -- lookup table, stored integer sums, the bits of
the response volume, response, mean and covariance, bit for bit -- and then the ROUTE: kh_matcher_score_loads must read what
lds_cases.predict() derives from the restated chunk builder (4 x row waves x the fast windows in chunks); just past a limit it must
read the windowed kernel's own count instead.  A case that took another route than predicted fails.

That the table bites was shown with one-line mutants of k_score_lds, each run once against this file and tests/test_matcher_gpu.py:
the tail step's selector keeping one slot too many (`rem > 2` -> `rem > 1`) failed 44 of the 65 tests here (6 of 31 there); the kFull
epilogue without its class shift (`(b + c) & 3` -> `b`) failed 17 (3 there).  The first-step formula of a part without step_base
failed nothing, here or there, and cannot: it is an equivalent mutant (lds_cases.deal(), and
test_lds_cases_oracle.py::test_every_step_is_dealt_once_whatever_step_base_is)."""
import numpy as np
import pytest

import lds_cases as lc
from common import bits

pytestmark = pytest.mark.gpu

CASES = lc.cases()


def _same(a, b, what):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert np.array_equal(bits(a), bits(b)), f"{what}: {a} vs {b}"


class Rig:
    """one geometry: the matcher with the path forced, the windowed one, the oracle"""

    def __init__(self, case):
        self.om = case.oracle_matcher()
        self.lds = case.hip_matcher()
        self.win = case.hip_matcher()
        self.lds.profile(True)
        self.win.profile(True)

    def search(self, hm, case, pen):
        hq = case.query.hip()
        hm.AddScans(hq, [b.hip() for b in case.base_scans()])
        hm.score_loads()
        centre, off, res, ang_off, ang_res = case.args()
        out = hm.CorrelateScan(hq, centre, off, res, ang_off, ang_res, pen, None, case.fine)
        loads = hm.score_loads()
        sums, resp = hm.volume()
        return out, sums, resp, hm.lookup_table(), loads

    def run(self, case):
        for dense in case.dense:
            self.lds.set_debug(True, lds_score=True, dense_score=dense)
            self.win.set_debug(True, windowed_score=True, dense_score=dense)
            for pen in case.pens:
                tag = f"{case.name} (pen={pen} dense={dense})"
                want = lc.run_oracle(self.om, case, pen)
                vol, table = self.om.volume(), self.om.lookup_table()
                cl = lc.classify(self.om, case)
                ch = lc.chunks(case, cl)
                got_l, sums_l, resp_l, table_l, loads_l = self.search(self.lds, case, pen)
                got_w, sums_w, resp_w, table_w, loads_w = self.search(self.win, case, pen)
                assert np.array_equal(table, table_l), f"lookup table vs oracle, {tag}"
                assert np.array_equal(sums_w, sums_l), f"stored sums vs the windowed kernel, {tag}: {int((sums_w != sums_l).sum())} of {sums_l.size} differ"
                assert np.array_equal(bits(vol[..., 0]), bits(resp_l)), f"response volume vs oracle, {tag}"
                assert np.array_equal(bits(vol[..., 0]), bits(resp_w)), f"response volume of the windowed kernel vs oracle, {tag}"
                for what, o, g in zip(("response", "mean", "covariance"), want, got_l):
                    _same(o, g, f"{what} vs oracle, {tag}")
                # ---- the route
                lds, formula = lc.predict(case, cl, ch)
                print(f"{tag}: predicted {'LDS' if lds else 'windowed'}, formula {formula}, loads {loads_l}, windowed kernel's {loads_w}, "
                      f"n_slow {ch['n_slow']}, chunks {[sum(len(w) for w in g) for g in ch['groups']]}")
                assert lds == case.probe["lds"]
                if not dense:
                    continue                      # (with the block map on, empty windows leave the count: results only)
                if lds:
                    assert loads_l == formula, f"route of {tag}: the LDS path reports 4 x row waves x fast windows in chunks"
                else:
                    assert loads_l == loads_w and loads_l != formula, f"route of {tag}: past the limit the windowed kernel scores"

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


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(rigs, case):
    rigs(case).run(case)


@pytest.mark.parametrize("n", [7, 8, 9])
def test_batch(rigs, n):
    """CorrelateScanBatch with the path forced: 8 jobs switch the XCD mapping of k_score_lds on, 9 leave seven of its job slots empty;
    queries of 64, 257 and 1081 beams mixed.  Every job equals the same search run alone, and the oracle's."""
    jobs = lc.batch_jobs(n)
    rig = rigs(jobs[0])
    hmb = jobs[0].hip_matcher(max_batch=n)
    try:
        hmb.set_debug(True, lds_score=True, dense_score=True)
        hmb.profile(True)
        scans = [j.query.hip() for j in jobs]
        for i, j in enumerate(jobs):
            hmb.AddScans(scans[i], [b.hip() for b in j.base_scans()], slot=i)
        hmb.score_loads()
        _, off, res, ang_off, ang_res = jobs[0].args()
        resp, means, covs, status = hmb.CorrelateScanBatch(scans, np.array([j.centre for j in jobs]), off, res, ang_off, ang_res, True, False)
        loads = hmb.score_loads()
        assert (status == 0).all()
        rig.lds.set_debug(True, lds_score=True, dense_score=True)
        formula = 0
        for i, j in enumerate(jobs):
            want = lc.run_oracle(rig.om, j, True)
            vol = rig.om.volume()
            cl = lc.classify(rig.om, j)
            lds, f = lc.predict(j, cl, lc.chunks(j, cl))
            assert lds
            formula += f
            alone, sums_a, resp_a, table_a, _ = rig.search(rig.lds, j, True)
            sums_b, resp_b = hmb.volume(slot=i)
            assert np.array_equal(sums_a, sums_b), f"job {i} of {n}: sums in the batch vs alone"
            assert np.array_equal(bits(vol[..., 0]), bits(resp_b)), f"job {i} of {n}: response volume vs oracle"
            assert np.array_equal(table_a, hmb.lookup_table(slot=i))
            for what, o, a, b in zip(("response", "mean", "covariance"), want, alone, (resp[i], means[i], covs[i])):
                _same(a, b, f"{what} of job {i} of {n}, batch vs alone")
                _same(o, b, f"{what} of job {i} of {n}, batch vs oracle")
        assert loads == formula, "route: every job of the batch on the LDS path"
    finally:
        hmb.close()


def test_small_two_cell_search_on_a_slot_with_decimated_copies(rigs):
    """Group G.  A slot that holds column-decimated copies (a large two-cell search allocates them) scores later two-cell searches from
    them with the windowed kernel's sx = 1 instance (CorrJob::dec); prepare_job reports such a job as sx = 1.  The LDS-staged kernels
    read the grid itself and must run the instance of the lattice's own step.

    It WAS a defect: enqueue_chunk handed the windowed kernel's instance number to launch_score_lds, so these searches ran
    k_score_lds<1> on a lattice stepping two cells -- rows 1 cell apart instead of 2, 61 poses per tile row instead of 31, the epilogue
    mapping byte j to pose j instead of j / 2: the sums differed from the oracle's at almost every pose.  The launch now takes
    JobShape::lds_sx, the lattice's step.  A one-cell job never has `dec`, so its instance (and the config-2 route) is what it was."""
    large, small, jobs = lc.decimated_cases()
    rig = rigs(small)
    hm = small.hip_matcher()
    plain = small.hip_matcher()
    try:
        hm.set_debug(True)
        rig.search(hm, large, False)                                   # the slot gets its column-decimated copies
        hm.set_debug(True, lds_score=True, dense_score=True)
        plain.set_debug(True, lds_score=True, dense_score=True, no_dual_copy=True)
        hm.profile(True)
        for pen in small.pens:
            want = lc.run_oracle(rig.om, small, pen)
            vol = rig.om.volume()
            cl = lc.classify(rig.om, small)
            lds, formula = lc.predict(small, cl, lc.chunks(small, cl))
            got, sums, resp, table, loads = rig.search(hm, small, pen)
            _, sums_p, resp_p, _, _ = rig.search(plain, small, pen)
            print(f"forced, pen={pen}: {int((sums != sums_p).sum())} of {sums.size} sums differ from the matcher without copies; loads {loads}, formula {formula}")
            assert np.array_equal(sums_p, sums), "sums vs a matcher without copies"
            assert np.array_equal(bits(vol[..., 0]), bits(resp)), "response volume vs oracle"
            for what, o, g in zip(("response", "mean", "covariance"), want, got):
                _same(o, g, f"{what} vs oracle (pen={pen})")
            assert lds and loads == formula, "route: the LDS path"
    finally:
        hm.close()
        plain.close()
    # ---- a batch large enough for the default rule: the slots get their copies from this very search.  First with no debug bit set
    # (the block map leaves empty windows out: the count is the copy-less matcher's), then with dense scoring alone, which leaves the
    # choice of the path to the default rule and makes the count the formula's
    n = len(jobs)
    hmb = jobs[0].hip_matcher(max_batch=n)
    plain = jobs[0].hip_matcher(max_batch=n)
    try:
        hmb.profile(True)
        plain.profile(True)
        scans = [j.query.hip() for j in jobs]
        _, off, res, ang_off, ang_res = jobs[0].args()
        centres = np.array([j.centre for j in jobs])
        ref = []                                                       # (the jobs alternate between two searches)
        for j in jobs[:2]:
            want = lc.run_oracle(rig.om, j, False)
            vol = rig.om.volume()
            cl = lc.classify(rig.om, j)
            lds, per_job = lc.predict(j, cl, lc.chunks(j, cl))
            assert lds
            ref.append((want, vol, per_job))
        formula = sum(ref[i % 2][2] for i in range(n))
        for dense in (False, True):
            hmb.set_debug(False, dense_score=dense)
            plain.set_debug(False, dense_score=dense, no_dual_copy=True)
            out, loads = {}, {}
            for key, m in (("copies", hmb), ("plain", plain)):
                for i, j in enumerate(jobs):
                    m.AddScans(scans[i], [b.hip() for b in j.base_scans()], slot=i)
                m.score_loads()
                out[key] = m.CorrelateScanBatch(scans, centres, off, res, ang_off, ang_res, False, False)
                loads[key] = m.score_loads()
            for i, j in enumerate(jobs):
                assert np.array_equal(j.centre, jobs[i % 2].centre) and j.query.n == jobs[i % 2].query.n
                want, vol, _ = ref[i % 2]
                sums, _ = hmb.volume(slot=i, responses=False)
                sums_p, _ = plain.volume(slot=i, responses=False)
                assert np.array_equal(sums_p, sums), f"job {i}: sums vs a matcher without copies ({int((sums != sums_p).sum())} of {sums.size} differ)"
                # (no penalties: the response is the sum over 100 x the beams)
                assert np.array_equal(bits(vol[..., 0]), bits(sums / float(100 * j.query.n))), f"job {i}: sums vs oracle"
                for k, what in enumerate(("response", "mean", "covariance")):
                    _same(want[k], out["copies"][k][i], f"{what} of job {i} vs oracle")
            assert (out["copies"][3] == 0).all()
            print(f"default-route batch, dense={dense}: loads {loads}, formula {formula}")
            assert 0 < loads["copies"] == loads["plain"] <= formula, "route: the count of the matcher without copies, which is on the LDS path"
            if dense:
                assert loads["copies"] == formula, "route: the default rule takes the LDS path for this batch"
    finally:
        hmb.close()
        plain.close()
