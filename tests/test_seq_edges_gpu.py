"""The fused path of ONE MatchScan (csrc/matcher_seq.cpp, the kseq_* kernels) at its limits, hand-backs and launch shapes: every case of
tests/seq_cases.py (tests/test_seq_cases_oracle.py proves on the CPU that each sits on its edge) through the fused matcher, a second
matcher on the general path (no_fused_match) and the CPU oracle -- response, mean, covariance, correlation grid, lookup table and
stored sums of the last search bit for bit -- and then the ROUTE, exactly: seq_stats() must read what seq_cases.predict() derives
from the restated limits and the oracle's volumes (0 refused at N, 1 with the named reason at N + 1; which pass the device finished)."""
import numpy as np
import pytest

import seq_cases as sc
from common import bits

pytestmark = pytest.mark.gpu

CASES = sc.cases()
BY_NAME = {c.name: c for c in CASES}


def _same(a, b, what):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert np.array_equal(bits(a), bits(b)), f"{what}: {a} vs {b}"


class Rig:
    """one geometry: the fused matcher, the general one, the oracle, and the counters the calls so far must have left"""

    def __init__(self, case):
        self.om = case.oracle_matcher()
        self.geo = sc.geometry(self.om)
        self.fused = case.hip_matcher()
        self.general = case.hip_matcher()
        self.general.set_debug(False, no_fused_match=True)
        self.want = sc.zero_stats()
        self.key = case.geometry()

    def run(self, case):
        assert case.geometry() == self.key
        # (reason 1: the fused matcher is asked to keep the response volume; bit 7 stays clear, so only the refusal keeps it off the path)
        self.fused.set_debug(bool(case.debug))
        hq, hb = case.query.hip(), [b.hip() for b in case.base]
        for pen, refine in case.pairs:
            st = sc.stages(self.om, case, pen, refine)
            got_f = self.fused.MatchScan(hq, hb, pen, refine)
            got_g = self.general.MatchScan(hq, hb, pen, refine)
            tag = f"{case.name} (pen={pen} refine={refine})"
            for what, o, f, g in zip(("response", "mean", "covariance"), st["result"], got_f, got_g):
                _same(g, f, f"{what}, fused vs general, {tag}")
                _same(o, f, f"{what}, fused vs oracle, {tag}")
            grid_f = self.fused.GetCorrelationGrid()
            assert np.array_equal(st["grid"], grid_f), f"grid vs oracle, {tag}"
            assert np.array_equal(self.general.GetCorrelationGrid(), grid_f), f"grid vs general, {tag}"
            assert np.array_equal(st["lookup"], self.fused.lookup_table()), f"lookup table vs oracle, {tag}"
            assert np.array_equal(self.general.lookup_table(), self.fused.lookup_table()), f"lookup table vs general, {tag}"
            sf, _ = self.fused.volume(responses=False)
            sg, _ = self.general.volume(responses=False)
            assert np.array_equal(sf, sg), f"stored sums of the last search, {tag}"
            sc.predict(self.want, case, self.geo, st, refine)
            got = self.fused.seq_stats()
            print(f"{tag}: coarse ties {st['coarse_ties']}, fine ties {st.get('fine_ties')}, seq_stats {got}")
            assert got == self.want, f"route of {tag}"
        assert self.general.seq_stats() == sc.zero_stats()

    def close(self):
        self.fused.close()
        self.general.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(kartohip_lib, case):
    rig = Rig(case)
    try:
        rig.run(case)
        st = rig.fused.seq_stats()
        assert st["fine_mismatches"] == 0
        reason = case.probe["reason"]
        assert st["ineligible"] == (len(case.pairs) if reason else 0) and st["ineligible_reason"] == reason
        assert st["calls"] == (0 if reason else len(case.pairs))
        if "on_device" in case.probe:
            n_refine = sum(1 for _, r in case.pairs if r)
            assert (st["fine_on_device"], st["fine_fallbacks"]) == ((n_refine, 0) if case.probe["on_device"] else (0, n_refine))
        if case.kind == "tie cap":
            assert st["coarse_fallbacks"] == (len(case.pairs) if case.probe["ties"] > sc.TIE_CAP else 0)
        if case.kind == "coarse ties" and isinstance(case.probe["ties"], tuple):
            assert st["coarse_fallbacks"] == 0 and st["fine_on_device"] == 0
            assert st["fine_fallbacks"] == sum(1 for _, r in case.pairs if r)
        if case.kind == "expansion":
            assert st["coarse_fallbacks"] == 0 and st["fine_on_device"] == 0
            assert st["fine_fallbacks"] == (0 if case.probe["expansion"] else sum(1 for _, r in case.pairs if r))
    finally:
        rig.close()


@pytest.mark.parametrize("name,names", sc.SEQUENCES, ids=[s[0] for s in sc.SEQUENCES])
def test_sequence_on_one_handle(kartohip_lib, name, names):
    """N, N + 1, N (and: many tiles, few, many) on ONE handle: the first-point table, the previous-tiles list and the result flag are
    left right by a large call and by a refused one -- every call is compared with the oracle's grid and result of that call alone"""
    rig = Rig(BY_NAME[names[0]])
    try:
        for n in names:
            rig.run(BY_NAME[n])
        st = rig.fused.seq_stats()
        refused = sum(len(BY_NAME[n].pairs) for n in names if BY_NAME[n].probe["reason"])
        assert st["ineligible"] == refused and st["calls"] == sum(len(BY_NAME[n].pairs) for n in names) - refused
        assert st["fine_mismatches"] == 0
    finally:
        rig.close()
