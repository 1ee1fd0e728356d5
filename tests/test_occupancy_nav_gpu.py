"""GPU: kh_occupancy_read_nav (k_occ_to_nav, csrc/occupancy.hip) -- vis_utils::toNavMap on the device, from the width_step-strided
cells into a dense width x height array -- on grids whose width sits around the 4 bytes of an output dword and the 8 of the row
padding, by height 1 and 2.  Each grid is filled through kh_occupancy_add_scans + kh_occupancy_update from one-cell beams of
tests/occupancy_cases.py: cell k of the grid (row-major) is made occupied, free or left unknown by (k + phase) % 3, for each of the
three phases, so that every cell of every grid -- the single cell of the 1 x 1 grid too -- is seen in all three states."""
import numpy as np
import pytest

import map_feed_rule as mf
import occupancy_cases as oc
from test_occupancy_edges_gpu import hip_scans

pytestmark = pytest.mark.gpu
RES, OFF = 0.5, (1.0, -0.5)
WANT = {0: 100, 1: 255, 2: 0}              # (k + phase) % 3 -> karto's cell state


def _fill(g, w, h, phase):
    """a beam that starts and ends in one cell visits it once; with a hit reading it counts the cell a second time and as a hit
    (1 / 2 > 0.1: occupied), with a reading too long for a hit it does not (0 / 1: free).  min_pass_through 0."""
    scans = []
    for k in range(w * h):
        state = (k + phase) % 3
        if state < 2:
            scans.append(oc.beams(OFF, RES, (k % w, k // w), [(k % w, k // w)], oc.HIT if state == 0 else oc.NO_HIT))
    g.Clear()
    if scans:
        g.AddScans(hip_scans(scans), oc.GATES)
    g.Update(0, 0.1)


@pytest.mark.parametrize("height", [1, 2])
@pytest.mark.parametrize("width", [1, 3, 4, 7, 8, 9, 63, 64, 65])
def test_read_nav(kartohip_lib, width, height):
    from slam_toolbox_amd.occupancy_grid import OccupancyGrid
    g = OccupancyGrid(width, height, OFF, RES)
    assert (g.nav() == -1).all() and g.nav().shape == (height, width), "an untouched grid is all -1"
    seen = np.zeros((3, height, width), dtype=bool)
    for phase in range(3):
        _fill(g, width, height, phase)
        cells = g.cells()
        assert cells.shape == (height, oc.align8(width)) and not cells[:, width:].any()
        want_cells = np.array([WANT[(k + phase) % 3] for k in range(width * height)], dtype=np.uint8).reshape(height, width)
        assert np.array_equal(cells[:, :width], want_cells), "the fill did not make the states the test wants"
        if width * height >= 3:
            assert set(np.unique(cells[:, :width]).tolist()) == {0, 100, 255}
        for k, v in enumerate((0, 100, 255)):
            seen[k] |= cells[:, :width] == v
        nav = g.nav()
        assert nav.dtype == np.int8 and nav.shape == (height, width)
        assert np.array_equal(nav, mf.to_nav(cells[:, :width])), f"{width} x {height}, phase {phase}"
    assert seen.all(), "a cell was not seen in all three states"
    g.Clear()
    g.Update(0, 0.1)
    assert (g.nav() == -1).all()
    g.close()
