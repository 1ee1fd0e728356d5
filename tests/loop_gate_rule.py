"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The covariance gate of the loop search restated in numpy, independent of the library:

  gated_sq          the gated squared distance of kh_graph_find_loop_candidates_gated, every operation an IEEE double operation
                    of its own in the order the header states
  find_loop_candidates   the walk of oracle/loops.py (FindNearLinkedScans + successive FindPossibleLoopClosure calls) driven by
                    the two predicates `q < r^2 + KT_TOLERANCE` (candidate) and `q <= r^2 - KT_TOLERANCE` (visitable)
  prepare_rows      what the mapper does to the difference covariances before the call (scale, cap at max_reach)
  semi_axis         the largest semi-axis of the widened ellipse of a row
  jump_rejects      the jump test on a 3 x 3
  column_passes     how many refreshes a mapper log implies for a refresh_scans setting

tests/test_loop_gate_rule_oracle.py pins the walk to oracle/loops.py (D = 0, chi2 = 0 on the golden graph)."""
import math
from collections import deque

import numpy as np

KT_TOLERANCE = 1e-06          # Math.h:41
f64 = np.float64


def gated_sq(dx, dy, s, dxx, dxy, dyy):
    """delta^T (I + s D)^-1 delta, or the plain dx dx + dy dy where the row is no covariance or the quotient is not finite"""
    dx, dy, s, dxx, dxy, dyy = (f64(v) for v in (dx, dy, s, dxx, dxy, dyy))
    with np.errstate(all="ignore"):
        a = f64(1.0) + s * dxx
        c = f64(1.0) + s * dyy
        b = s * dxy
        det = a * c - b * b
        num = (c * (dx * dx) - f64(2.0) * b * (dx * dy)) + a * (dy * dy)
        q = num / det
        plain = (not det > 0.0) or (not a >= 1.0) or (not c >= 1.0) or (not np.isfinite(q))
        return float(dx * dx + dy * dy) if plain else float(q)


def gate_s(chi2, max_distance):
    with np.errstate(all="ignore"):
        return float(f64(chi2) / (f64(max_distance) * f64(max_distance)))


def gated_sq_all(q, ref_xy, max_distance, chi2, rows):
    """q_i for every scan i; rows (n, 3, 3) or (n, 9): the row of this query"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    s = gate_s(chi2, max_distance)
    out = np.zeros(ref_xy.shape[0])
    for i in range(ref_xy.shape[0]):
        dx = f64(ref_xy[i, 0]) - f64(ref_xy[q, 0])
        dy = f64(ref_xy[i, 1]) - f64(ref_xy[q, 1])
        out[i] = gated_sq(dx, dy, s, rows[i, 0], rows[i, 1], rows[i, 4])
    return out


def find_loop_candidates(q, ref_xy, adj_ptr, adj_idx, max_distance, min_chain_size, chi2, rows, start=0, n_visit=None):
    """oracle.loops.find_possible_loop_closures with the squared distance replaced by gated_sq in BOTH tests"""
    d2 = gated_sq_all(q, ref_xy, max_distance, chi2, rows)
    sq = f64(max_distance) * f64(max_distance)
    lim_visit, lim_range = sq - KT_TOLERANCE, sq + KT_TOLERANCE
    # near_linked_scans
    to_visit, seen, linked = deque([q]), {q}, set()
    while to_visit:
        v = to_visit.popleft()
        if d2[v] <= lim_visit:
            linked.add(v)
            for w in adj_idx[adj_ptr[v]: adj_ptr[v + 1]]:
                w = int(w)
                if w not in seen:
                    seen.add(w)
                    to_visit.append(w)
    # find_possible_loop_closures
    n = ref_xy.shape[0] if n_visit is None else int(n_visit)
    out = []
    start = int(start)
    while True:
        chain = []
        returned = False
        while start < n:
            if d2[start] < lim_range:
                if start in linked:
                    chain = []
                else:
                    chain.append(start)
            else:
                if len(chain) >= min_chain_size:
                    returned = True
                    break
                chain = []
            start += 1
        if not chain:
            break
        out.append((chain[0], chain[-1]))
        if not returned:
            break
    return out


def prepare_rows(D, max_distance, chi2_position, covariance_scale, max_reach):
    """(n, 3, 3) difference covariances -> the rows the mapper hands to the gated call: G = covariance_scale D, scaled down where
    s (Gxx + Gyy) > (max_reach / r)^2 - 1"""
    G = float(covariance_scale) * np.asarray(D, dtype=np.float64).reshape(-1, 3, 3)
    r = float(max_distance)
    s = chi2_position / (r * r)
    limit = max(0.0, (max_reach / r) * (max_reach / r) - 1.0)
    for g in G:
        reach = s * (g[0, 0] + g[1, 1])
        if reach > limit:
            g *= limit / reach
    return G


def semi_axis(row, max_distance, chi2):
    """the largest semi-axis of delta^T (r^2 I + chi2 G)^-1 delta < 1"""
    g = np.asarray(row, dtype=np.float64).reshape(3, 3)[:2, :2]
    lam = float(np.linalg.eigvalsh(0.5 * (g + g.T))[-1])
    return math.sqrt(max_distance * max_distance + chi2 * max(lam, 0.0))


def jump_rejects(e, D3, C_fine, covariance_scale, chi2_jump):
    """e = fine mean - current sensor pose (angle normalised): rejected when e^T (covariance_scale D3 + C_fine)^-1 e > chi2_jump or
    the 3 x 3 is not positive definite"""
    M = covariance_scale * np.asarray(D3, dtype=np.float64).reshape(3, 3) + np.asarray(C_fine, dtype=np.float64).reshape(3, 3)
    if not np.isfinite(M).all():
        return True
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return True
    y = np.linalg.solve(L, np.asarray(e, dtype=np.float64))
    return not float(y @ y) <= chi2_jump


def column_passes(log_lines, refresh_scans):
    """Refreshes a run with this mapper log made (gate enabled with parameters that need covariances, no pass refused): every
    accepted scan (an `N id ...` line) is one TryCloseLoop call; a refresh is owed at the start and after every closure (an `X`
    line: the search goes on behind the closed chain, with refreshed covariances), and falls due when refresh_scans calls have
    passed since the last one.  The first scan has no constraint yet: nothing to compute, the refresh stays owed."""
    passes, age, due = 0, 0, True
    for line in log_lines:
        if line.startswith("N "):
            age += 1
            if int(line.split()[1]) == 0:
                continue
            if due or age >= refresh_scans:
                passes, age, due = passes + 1, 0, False
        elif line.startswith("X "):
            passes, age, due = passes + 1, 0, False
    return passes
