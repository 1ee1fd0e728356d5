"""TEST INFRASTRUCTURE (not a test): the fit of a submap's placement and the automatic alignment built on it (DESIGN.md section 7a,
"Fit and alignment"), restated in numpy on top of tests/merge_rule.py -- hence on the occupancy oracle -- and, for the hypotheses
of a probe, of tests/relocalize_rule.py.  It reads nothing of the library.

    reference grid   merge_rule.merged_grid(others, their corrections, ...): dimensions, offset and cells of a merge WITHOUT the
                     moving submap M
    per candidate C  p, h = merge_rule.submap_counters(M, C, width, height, offset, resolution): M's transformed scans traced on the
                     reference grid's geometry; visits outside the grid are dropped
    six counters     for s in (unknown 0, occupied 100, free 255): pass_s = sum p[cells == s], hits_s = sum h[cells == s]
    derived          agree = hits_occ + (pass_free - 2 hits_free); conflict = (pass_occ - 2 hits_occ) + hits_free;
                     known = agree + conflict; score = agree / known, one IEEE double division, 0.0 when known == 0
                     (pass - 2 hits: the visits that are not the end cell of a hit beam -- that cell is visited twice)
    ranking          known >= min_known first, then score descending, agree descending, candidate index ascending
    probes           M's alive scans in scan-id order; probe j is entry floor(j * n_alive / n_probes), n_probes clipped to n_alive
    refused          fit_refused: a moving laser with range_threshold * scale + 2 > 2^20 cells, or a candidate under which a sensor
                     lies more than 2^30 cells from the reference grid's offset (the library: KH_ERR_INVALID_ARG, nothing launched)
    candidates       0: M's current correction; then per probe, per hypothesis in rank order, (T_target . P) . inverse(Q) with P the
                     hypothesis' robot pose and Q the probe's corrected pose in M; no de-duplication
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import merge_rule

STATES = (("unknown", 0), ("occupied", 100), ("free", 255))
COUNTERS = tuple(f"pass_{n}" for n, _ in STATES) + tuple(f"hits_{n}" for n, _ in STATES)
FIELDS = COUNTERS + ("agree", "conflict", "known", "score")


def reference_grid(others, transforms, resolution, min_pass_through=2, occupancy_threshold=0.1):
    if not others or not any(sm["scans"] for sm in others):
        raise ValueError("no other submap, or no scan in any of them")          # the library: KH_ERR_INVALID_ARG
    return merge_rule.merged_grid(others, transforms, resolution, min_pass_through, occupancy_threshold)


def derive(counters):
    """the six counters (python ints) -> dict with the derived values"""
    f = {k: int(counters[k]) for k in COUNTERS}
    f["agree"] = f["hits_occupied"] + (f["pass_free"] - 2 * f["hits_free"])
    f["conflict"] = (f["pass_occupied"] - 2 * f["hits_occupied"]) + f["hits_free"]
    f["known"] = f["agree"] + f["conflict"]
    assert min(f.values()) >= 0 and f["known"] < 2 ** 53
    f["score"] = float(np.float64(f["agree"]) / np.float64(f["known"])) if f["known"] else 0.0
    return f


def count(cells, p, h):
    out = {}
    for name, state in STATES:
        out[f"pass_{name}"] = int(p[cells == state].sum(dtype=np.uint64))
        out[f"hits_{name}"] = int(h[cells == state].sum(dtype=np.uint64))
    return out


def fit_on(moving, candidates, grid, resolution):
    """candidates (n, 3) of `moving` on a reference grid (merged_grid's dict) -> list of n dicts (FIELDS)"""
    out = []
    for c in np.asarray(candidates, dtype=np.float64).reshape(-1, 3):
        if moving["scans"]:
            p, h = merge_rule.submap_counters(moving, tuple(c), grid["width"], grid["height"], grid["offset"], resolution)
        else:
            p = h = np.zeros(grid["cells"].shape, dtype=np.uint32)
        out.append(derive(count(grid["cells"], p, h)))
    return out


MAX_FIT_WALK, MAX_FIT_CELL = 2 ** 20, 2.0 ** 30


def fit_refused(moving, candidates, grid, resolution):
    """What kh_merge_fit / kh_merge_align refuse before anything is launched (KH_ERR_INVALID_ARG), so that no beam walks more than
    2^20 cells and no cell index leaves the int32 lattice: None = accepted, ("laser", -1) = the moving submap's laser has
    range_threshold * scale + 2 > 2^20 (or a range_threshold that is not finite and positive), ("pose", k) = candidate k, the first
    such, puts the sensor of one of its scans more than 2^30 cells from the reference grid's offset on either axis --
    |(sensor - offset) * scale| > 2^30 with scale = 1 / resolution, one subtraction and one product."""
    laser, scale = moving["laser"], 1.0 / float(resolution)
    rt = float(laser.range_threshold)
    if not (np.isfinite(rt) and rt > 0.0 and rt * scale + 2.0 <= float(MAX_FIT_WALK)):
        return ("laser", -1)
    if np.isnan(float(laser.min_range)) or np.isnan(float(laser.max_range)):
        return ("laser", -1)
    ox, oy = float(grid["offset"][0]), float(grid["offset"][1])
    for k, c in enumerate(np.asarray(candidates, dtype=np.float64).reshape(-1, 3)):
        for s in moving["scans"]:
            sensor = merge_rule.sensor_at(merge_rule.transform_pose(tuple(c), s["corrected"]), getattr(laser, "offset", (0.0, 0.0, 0.0)))
            cx, cy = (float(sensor[0]) - ox) * scale, (float(sensor[1]) - oy) * scale
            if not (np.isfinite(cx) and np.isfinite(cy) and abs(cx) <= MAX_FIT_CELL and abs(cy) <= MAX_FIT_CELL):
                return ("pose", k)
    return None


def fit(moving, candidates, others, transforms, resolution, min_pass_through=2, occupancy_threshold=0.1):
    return fit_on(moving, candidates, reference_grid(others, transforms, resolution, min_pass_through, occupancy_threshold), resolution)


def ranking(fits, min_known=0):
    """-> candidate indices, best first"""
    return sorted(range(len(fits)), key=lambda i: (not fits[i]["known"] >= min_known, -fits[i]["score"], -fits[i]["agree"], i))


def probe_entries(n_alive, n_probes):
    n = min(int(n_probes), int(n_alive))
    return [(j * int(n_alive)) // n for j in range(n)]


def candidate(t_target, p, q):
    """(T_target . P) . inverse(Q), section 7a's composition, left to right"""
    return merge_rule.compose(merge_rule.compose(t_target, p), merge_rule.inverse(q))


def hypotheses_of(result, laser_offset=(0.0, 0.0, 0.0)):
    """a relocalize_rule.Result -> [(robot pose, fine response)] in rank order: what a probe's relocalization hands to `candidates`"""
    import relocalize_rule
    return [(relocalize_rule.robot_at(result.hyps[i].fine_mean, laser_offset), result.hyps[i].fine_response) for i in result.ranking]


Candidate = namedtuple("Candidate", "correction probe_scan hypothesis fine_response")


def candidates(current, t_target, scan_ids, corrected, n_probes, top_k, relocalize):
    """current: M's correction; scan_ids / corrected: M's alive scans in scan-id order and their corrected poses (n_alive, 3);
    relocalize(entry) -> [(robot pose P, fine response)] of that scan in the target's map, best first (hypotheses_of a rule run, or
    the library's own answer).  -> list of Candidate in candidate-index order"""
    out = [Candidate(np.asarray(current, dtype=np.float64).copy(), -1, -1, 0.0)]
    for entry in probe_entries(len(scan_ids), n_probes):
        for rank, (p, fine) in enumerate(relocalize(entry)[:top_k]):
            out.append(Candidate(candidate(t_target, p, corrected[entry]), int(scan_ids[entry]), rank, float(fine)))
    return out
