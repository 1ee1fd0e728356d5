"""TEST INFRASTRUCTURE: the searches tests/test_cell_maxima_gpu.py reads the search-space probabilities of, picked from the table of
tests/lds_cases.py -- the coarse cases of its groups A (lattices: every instance of k_score_lds and both forms of its merge), B (1, 2,
3, 9 angles: a dead second angle), D3 (tails), D5 (slow entries) and "every reading invalid".  The 61 x 61 x 81 x 1081 case stays
with tests/test_lds_edges_gpu.py.  tests/test_cell_maxima_cases_oracle.py proves on the CPU that the picked cases sit where the GPU
test needs them.  Nothing here calls the library."""
import lds_cases as lc

ALL_INVALID = "every reading invalid"
BIG = "config-2 shape"


def picked():
    out = []
    for c in lc.cases():
        if c.fine or not c.probe.get("lds") or c.name == BIG:
            continue
        if c.kind in ("lattice", "angles", "tails", "fallback") or c.name == ALL_INVALID:
            out.append(c)
    return out


def expected_lattice(om):
    """the search-space probabilities of the oracle's last CorrelateScan: its response volume reduced over the angle axis"""
    return om.volume()[..., 0].max(axis=2)
