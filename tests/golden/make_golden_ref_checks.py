"""Generates tests/golden/ref_checks.npz from the reference build (oracle/_ref/libkarto_ref.so, see oracle/Makefile): the
reference's own results for the seeded cases of tests/test_oracle_vs_reference.py and of the reference check in
tests/test_find_valid_algorithm.py, so that those tests pin the C oracle where the reference is not present.  Run where
oracle/_ref is built:

    make -C oracle ref && python tests/golden/make_golden_ref_checks.py

Per MatchScan: response, mean and covariance (13 doubles) and a digest of the rasterised grid and of the lookup table
(ref_digest: sha256 of the int64 values and the shape).  Per FindValidPoints case: the scan's points and the valid points.
Per call of tests/geometry_cases.py's table (keys geo_*): the same three, from the table's own laser.  Entries that exist are
never rewritten with other bytes: the run stops if the reference gives anything else for them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from common import LASER, OFFLINE_PARAMS, PRESETS, Scenario, make_oracle_matcher, ref_digest, ref_row  # noqa: E402
from oracle import ref  # noqa: E402
import geometry_cases as gc  # noqa: E402
import test_find_valid_algorithm as fv  # noqa: E402
import test_geometry_cases_oracle as tg  # noqa: E402
import test_oracle_vs_reference as ovr  # noqa: E402


def main():
    assert ref.available(), "oracle/_ref not built"
    ref.init_laser(LASER)
    out = {}
    for preset, seed, start, n_base, perturb in ovr.MATCH_CASES:
        sc = Scenario(seed=seed, n_base=n_base, start=start, perturb=perturb)
        rq, rb = sc.ref_scans()
        p = PRESETS[preset]
        mr = ref.RefMatcher(*p["create"], p["params"])
        oq, ob = sc.oracle_scans()
        mo = make_oracle_matcher(preset)
        for pen, refine in ovr.MATCH_FLAGS:
            key = ovr.match_key(preset, seed, pen, refine)
            out[key] = ref_row(mr.match_scan(rq, rb, pen, refine))
            out[key + "_grid"] = np.asarray(ref_digest(mr.grid()))
            # the table's shape (angles x points) is the one of the last search, read from the oracle as the test does
            mo.match_scan(oq, ob, pen, refine)
            out[key + "_lut"] = np.asarray(ref_digest(mr.lookup_table(*mo.lookup_table().shape)))
    for (seed, n_base, start, perturb, preset), keys in ovr.SINGLE_CASES:
        sc = Scenario(seed=seed, n_base=n_base, start=start, perturb=perturb)
        rq, rb = sc.ref_scans()
        p = PRESETS[preset]
        mr = ref.RefMatcher(*p["create"], p["params"])
        for key in keys:
            out[key] = ref_row(mr.match_scan(rq, [] if key.endswith("_empty") else rb))
    pose, view = fv.REF_POSE, fv.REF_POSE[:2] + fv.REF_VIEW_OFFSET
    for case, ranges in enumerate(fv._range_cases()):
        rs = ref.RefScan(ranges, pose)
        rm = ref.RefMatcher(*PRESETS["S"]["create"], OFFLINE_PARAMS)
        out[f"fv_points_{case}"] = rs.points()
        out[f"fv_valid_{case}"] = np.ascontiguousarray(rm.find_valid_points(rs, view))
    # the geometries off the presets: the table's laser (181 beams over 270 degrees), one reference matcher per params set
    ref.init_laser(gc.laser())
    for geo in gc.GEOMETRIES:
        sc = gc.Scene(geo)
        rq, rb = tg.ref_scans(sc)
        oq, ob = sc.query.oracle(), [b.oracle() for b in sc.base]
        for pname, params in geo.params_sets():
            mr = ref.RefMatcher(*geo.create, params)
            mo = geo.oracle_matcher(params)
            for key, p, kind, arg in tg.calls(geo):
                if p != pname:
                    continue
                out[key] = ref_row(tg.run_call(mr, kind, arg, rq, rb))
                out[key + "_grid"] = np.asarray(ref_digest(mr.grid()))
                tg.run_call(mo, kind, arg, oq, ob)          # (the table's shape, read from the oracle as the test does)
                out[key + "_lut"] = np.asarray(ref_digest(mr.lookup_table(*mo.lookup_table().shape)))
    ref.init_laser(LASER)
    path = os.path.join(HERE, "ref_checks.npz")
    if os.path.exists(path):
        old = np.load(path)
        for k in old.files:
            if k.startswith("geo_"):
                continue
            a, b = old[k], out[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"existing entry {k} would change"
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays")


if __name__ == "__main__":
    main()
