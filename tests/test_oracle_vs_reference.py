"""The C oracle against the reference's own karto_sdk build (oracle/_ref) on seeded scenarios beyond the golden fixtures of
test_oracle_golden.py.  Where oracle/_ref is built the reference runs live beside the oracle and must also reproduce its
recorded results (tests/golden/ref_checks.npz, tests/golden/make_golden_ref_checks.py); elsewhere the oracle is held to the
recording: response, mean and covariance bit for bit, grid and lookup table by digest."""
import numpy as np
import pytest

from common import LASER, PRESETS, Scenario, bits, make_oracle_matcher, ref_digest, ref_recorded, ref_row
from oracle import ref

LIVE = ref.available()
MATCH_CASES = [
    ("K", 31, 40, 5, (0.08, 0.02, -0.05)),
    ("K", 32, 150, 12, (-0.1, 0.1, 0.2)),
    ("S", 33, 77, 10, (0.02, 0.03, 0.01)),
    ("L", 34, 10, 30, (1.5, -2.0, 0.15)),
    ("L", 35, 300, 15, (-3.0, 0.5, -0.3)),
]
MATCH_FLAGS = [(True, True), (False, False)]
# (seed, n_base, start, perturb, preset), then the calls made in turn on ONE matcher: "*_empty" matches against no base scans
SINGLE_CASES = [((36, 6, 50, (0.0, 0.0, 1.2), "S"), ("expansion",)),
                ((37, 3, 90, (25.0, 25.0, 0.0), "K"), ("far_empty", "far_base"))]


def match_key(preset, seed, pen, refine):
    return f"match_{preset}_{seed}_{int(pen)}{int(refine)}"


@pytest.fixture(scope="module")
def recorded():
    if LIVE:
        ref.init_laser(LASER)
    return ref_recorded()


def _same_row(a, b):
    assert np.array_equal(bits(a), bits(b)), (a, b)


@pytest.mark.parametrize("preset,seed,start,n_base,perturb", MATCH_CASES)
def test_match_scan_equals_reference(oracle_lib, recorded, preset, seed, start, n_base, perturb):
    sc = Scenario(seed=seed, n_base=n_base, start=start, perturb=perturb)
    oq, ob = sc.oracle_scans()
    p = PRESETS[preset]
    mo = make_oracle_matcher(preset)
    if LIVE:
        rq, rb = sc.ref_scans()
        mr = ref.RefMatcher(*p["create"], p["params"])
    for pen, refine in MATCH_FLAGS:
        key = match_key(preset, seed, pen, refine)
        b = mo.match_scan(oq, ob, pen, refine)
        lt = mo.lookup_table()
        if LIVE:
            a = mr.match_scan(rq, rb, pen, refine)
            assert np.array_equal(bits(a[0]), bits(b[0]))
            assert np.array_equal(bits(a[1]), bits(b[1]))
            assert np.array_equal(bits(a[2]), bits(b[2]))
            assert np.array_equal(mr.grid(), mo.grid())
            assert np.array_equal(mr.lookup_table(*lt.shape), lt)
            _same_row(ref_row(a), recorded[key])
        _same_row(ref_row(b), recorded[key])
        assert ref_digest(mo.grid()) == str(recorded[key + "_grid"])
        assert ref_digest(lt) == str(recorded[key + "_lut"])


def _singles(case, recorded):
    (seed, n_base, start, perturb, preset), keys = SINGLE_CASES[case]
    sc = Scenario(seed=seed, n_base=n_base, start=start, perturb=perturb)
    oq, ob = sc.oracle_scans()
    mo = make_oracle_matcher(preset)
    if LIVE:
        rq, rb = sc.ref_scans()
        p = PRESETS[preset]
        mr = ref.RefMatcher(*p["create"], p["params"])
    for key in keys:
        empty = key.endswith("_empty")
        b = mo.match_scan(oq, [] if empty else ob)
        if LIVE:
            a = mr.match_scan(rq, [] if empty else rb)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
            assert np.array_equal(bits(a[2]), bits(b[2]))
            _same_row(ref_row(a), recorded[key])
        _same_row(ref_row(b), recorded[key])


def test_response_expansion_path(oracle_lib, recorded):
    """Query 90 degrees off: the coarse search finds nothing and the +20 degree expansion loop runs."""
    _singles(0, recorded)


def test_empty_base_and_far_query(oracle_lib, recorded):
    _singles(1, recorded)
