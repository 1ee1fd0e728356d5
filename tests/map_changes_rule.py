"""TEST INFRASTRUCTURE (not a test): the rule of the map change layer in numpy -- what kh_map_changes_* must
compute.  It reads nothing of the library.  The lattice, the gate and the line are tests/map_localize_rule.py's (section 7k), the
observed state is the occupancy oracle's UpdateCell (tests/test_map_changes_rule_oracle.py holds the two side by side).

  layer     two uint32 grids pass / hits on the view's window, zero at creation
  observe   every beam that passes AddScan's gate is walked by TraceLine from the sensor cell to the end cell: pass += 1 on every visited
            cell inside the window; a hit end cell inside it: pass += 1 and hits += 1 once more
  label     against the MAP's states, with t cells of tolerance: blocked = visited window cells of the line (the hit's re-visit apart) of
            state 100 further than t from the end cell (Chebyshev); near = a window cell of state 100 within t of the end cell
  decay     pass >>= shift, hits >>= shift
  bound     + 2 * n_beams per scan, shifted by a decay; a call that would take it above 2^32 - 1 is refused
  diff      observed = pass > min_pass_through ? (hits / pass > threshold ? 100 : 255) : 0; the code per cell, six counts, the patched
            grid, the cells of code >= 2 in row-major window order
"""
from __future__ import annotations

import numpy as np

import map_localize_rule as ml

DROPPED, EXPLAINED, NOVEL, UNKNOWN, THROUGH, CLEAR = range(6)
UNOBSERVED, CONFIRMED, APPEARED, VANISHED, DISCOVERED_OCCUPIED, DISCOVERED_FREE = range(6)
MAX_TOLERANCE = 4
MAX_COUNT = 2 ** 32 - 1


class Refused(ValueError):
    """the library answers KH_ERR_INVALID_ARG and changes nothing"""


def bound_after(bound, n_scans, n_beams):
    """the layer's bound after observing n_scans scans; Refused where it would pass 2^32 - 1"""
    after = bound + 2 * n_beams * n_scans
    if n_scans < 1 or n_beams < 1 or after > MAX_COUNT:
        raise Refused("bound")
    return after


def chebyshev_near(view, ex, ey, t):
    """is a window cell of state 100 within Chebyshev distance t of lattice cell (ex, ey)?"""
    for cy in range(ey - t, ey + t + 1):
        for cx in range(ex - t, ex + t + 1):
            if ml.state_at(view, cx, cy) == 100:
                return True
    return False


class Layer:
    def __init__(self, view):
        self.view = view
        shape = view["cells"].shape                             # (height, width_step)
        self.passes, self.hits = np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32)
        self.bound, self.scans, self.beams = 0, 0, 0

    def clear(self):
        self.passes[:], self.hits[:] = 0, 0
        self.bound, self.scans, self.beams = 0, 0, 0

    def decay(self, shift):
        if not 1 <= shift <= 31:
            raise Refused("shift")
        self.passes >>= np.uint32(shift)
        self.hits >>= np.uint32(shift)
        self.bound >>= shift

    def observe(self, laser, ranges, poses, t=1, points=None):
        """ranges (n_scans, n_beams), poses (n_scans, 3) -> labels (n_scans, n_beams, 2) int32: class, blocked"""
        from oracle import karto
        ranges = np.asarray(ranges, dtype=np.float64).reshape(-1, laser.n_beams)
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        view = self.view
        if not 0 <= t <= MAX_TOLERANCE or len(poses) < 1 or len(poses) != len(ranges) or any(ml.fit_refused(view, laser, p) for p in poses):
            raise Refused("arguments")
        bound = bound_after(self.bound, len(poses), laser.n_beams)
        ax, ay, scale = view["anchor"][0], view["anchor"][1], view["scale"]
        labels = np.zeros((len(poses), laser.n_beams, 2), dtype=np.int32)
        for s, (scan, pose) in enumerate(zip(ranges, poses)):
            pts = karto.scan_points(scan, pose, laser) if points is None else points[s]
            x0, y0 = ml.lattice_cell(pose[0], ax, scale), ml.lattice_cell(pose[1], ay, scale)
            for i, (r, p) in enumerate(zip(scan, pts)):
                kept, hit, end = ml.gate(r, p, pose, laser)
                if not kept:
                    continue                                    # DROPPED, 0
                x1, y1 = ml.lattice_cell(end[0], ax, scale), ml.lattice_cell(end[1], ay, scale)
                cx, cy = ml.line_cells(x0, y0, x1, y1)
                wx, wy = cx - view["ox"], cy - view["oy"]
                inside = (wx >= 0) & (wx < view["width"]) & (wy >= 0) & (wy < view["height"])
                wx, wy = wx[inside], wy[inside]
                np.add.at(self.passes, (wy, wx), np.uint32(1))
                end_state = ml.state_at(view, x1, y1)
                if hit and end_state is not None:
                    self.passes[y1 - view["oy"], x1 - view["ox"]] += np.uint32(1)
                    self.hits[y1 - view["oy"], x1 - view["ox"]] += np.uint32(1)
                far = np.maximum(np.abs(cx[inside] - x1), np.abs(cy[inside] - y1)) > t
                blocked = int(np.count_nonzero((view["cells"][wy, wx] == 100) & far))
                if blocked > 0:
                    label = THROUGH
                elif not hit:
                    label = CLEAR
                elif chebyshev_near(view, x1, y1, t):
                    label = EXPLAINED
                else:
                    label = NOVEL if end_state == 255 else UNKNOWN
                labels[s, i] = (label, blocked)
        self.bound, self.scans, self.beams = bound, self.scans + len(poses), self.beams + ranges.size
        return labels

    def diff(self, min_pass_through=2, occupancy_threshold=0.1):
        """-> dict(codes (h, ws) uint8, counts [6], patched (h, ws) uint8 with the padding 0, cells (n, 3) int32: lattice i, j, code)"""
        view = self.view
        h, w = view["height"], view["width"]
        raw = view["cells"][:h, :w]
        p, n = self.passes[:h, :w], self.hits[:h, :w]
        ratio = n.astype(np.float64) / np.maximum(p, 1).astype(np.float64)
        seen = np.where(p > np.uint32(min_pass_through), np.where(ratio > np.float64(occupancy_threshold), 100, 255), 0).astype(np.uint8)
        known = np.where((raw == 100) | (raw == 255), raw, 0).astype(np.uint8)
        code = np.zeros((h, w), dtype=np.uint8)
        code[(seen != 0) & (seen == known)] = CONFIRMED
        code[(known == 255) & (seen == 100)] = APPEARED
        code[(known == 100) & (seen == 255)] = VANISHED
        code[(known == 0) & (seen == 100)] = DISCOVERED_OCCUPIED
        code[(known == 0) & (seen == 255)] = DISCOVERED_FREE
        codes, patched = np.zeros_like(view["cells"]), np.zeros_like(view["cells"])
        codes[:h, :w] = code
        patched[:h, :w] = np.where(seen != 0, seen, raw)
        j, i = np.nonzero(code >= 2)                             # row-major
        cells = np.stack([i + view["ox"], j + view["oy"], code[j, i]], axis=1).astype(np.int32).reshape(-1, 3)
        return dict(codes=codes, counts=np.bincount(code.ravel(), minlength=6).astype(np.int64), patched=patched, cells=cells)


def nav_of(cells, width):
    """kh_occupancy_read_nav's mapping of the three states: 0 -> -1, 100 -> 100, 255 -> 0"""
    c = np.asarray(cells)[:, :width]
    out = np.full(c.shape, -1, dtype=np.int8)
    out[c == 100] = 100
    out[c == 255] = 0
    return out


def patched_view(view, patched):
    """the view a diff's patched cells make on the source view's lattice"""
    return dict(view, cells=patched)
