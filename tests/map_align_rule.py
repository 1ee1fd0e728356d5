"""TEST INFRASTRUCTURE (not a test): the rule of kh_map_align in numpy on the CPU oracle -- placing one map in
another with no scan of either.  It reads nothing of the library.  Seeds and fit are tests/map_localize_rule.py's, the cast
tests/map_raycast_rule.py's, composition and inverse tests/merge_rule.py's, the derived values and the ranking tests/merge_fit_rule.py's.

  casting      seeds of the moving view at probe_spacing; every seed a robot pose of heading 0, the sensor through the laser offset;
               all cast with max_unknown and the default no_return
  probes       the n_probes seeds with the most HIT beams, ties to the lower seed index; a seed with no HIT is never a probe
  relocalizing relocalize(ranges) -> [(robot pose P, fine response)] best first, at most top_k: each gives C = P . inverse(Q), Q the
               probe's robot pose
  candidates   0: `initial`; then the probes in pick order, each one's hypotheses in rank order; nothing is de-duplicated
  fit          candidate i, probe j: the six counters of the probe's ranges at sensor pose C_i . S_j against the target; summed over
               the probes, derived as merge_fit_rule.derive
  rank         known >= min_known first, then score descending, agree descending, index ascending
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import map_localize_rule as ml
import map_raycast_rule as cast_rule
import merge_fit_rule as fr
import merge_rule
import relocalize_rule as rr

Probe = namedtuple("Probe", "seed robot sensor ranges hits")
Candidate = namedtuple("Candidate", "correction probe_seed hypothesis fine_response")
Result = namedtuple("Result", "seed_cells hits probes candidates counters fits order")


def pick_probes(hits, n_probes):
    """hit counts per seed -> seed indices: most hits first, ties to the lower index, none without a hit"""
    order = sorted((k for k in range(len(hits)) if hits[k] > 0), key=lambda k: (-int(hits[k]), k))
    return order[:max(0, int(n_probes))]


def correction(p, q):
    """C = P . inverse(Q): the probe, at robot pose Q in the moving map, stands at P in the target's"""
    return merge_rule.compose(p, merge_rule.inverse(q))


def probes_of(moving, laser, probe_spacing, n_probes, max_unknown):
    offset = tuple(getattr(laser, "offset", (0.0, 0.0, 0.0)))
    cells, xy = ml.seeds(moving, probe_spacing)
    robots = [np.array([x, y, 0.0]) for x, y in xy]
    sensors = [np.asarray(rr.sensor_at(tuple(r), offset), dtype=np.float64) for r in robots]
    casts = [cast_rule.cast(moving, laser, s, max_unknown) for s in sensors]
    hits = [int((c.codes == cast_rule.HIT).sum()) for c in casts]
    return cells, hits, [Probe(k, robots[k], sensors[k], casts[k].ranges, hits[k]) for k in pick_probes(hits, n_probes)]


def sum_counters(target, laser, probes, corrections):
    out = []
    for c in corrections:
        total = dict.fromkeys(fr.COUNTERS, 0)
        for p in probes:
            one = ml.fit_counters(target, laser, p.ranges, merge_rule.transform_pose(c, p.sensor))
            for k in fr.COUNTERS:
                total[k] += one[k]
        out.append(total)
    return out


def align(target, moving, laser, relocalize, probe_spacing, n_probes=3, top_k=4, max_unknown=20, min_known=0, initial=(0.0, 0.0, 0.0)):
    """relocalize(ranges) -> [(robot pose, fine response)] in the target map, best first (a rule run on the oracle, or the library's
    own answer).  -> Result; `order` holds candidate indices, best first"""
    cells, hits, probes = probes_of(moving, laser, probe_spacing, n_probes, max_unknown)
    cands = [Candidate(np.asarray(initial, dtype=np.float64).copy(), -1, -1, 0.0)]
    for p in probes:
        for rank, (pose, fine) in enumerate(relocalize(p.ranges)[:top_k]):
            cands.append(Candidate(correction(pose, p.robot), p.seed, rank, float(fine)))
    counters = sum_counters(target, laser, probes, [c.correction for c in cands])
    fits = [fr.derive(c) for c in counters]
    return Result(cells, hits, probes, cands, counters, fits, fr.ranking(fits, min_known))
