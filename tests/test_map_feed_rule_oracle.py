"""CPU: the rule the map feed's GPU tests rely on (tests/map_feed_rule.py), checked on the oracle alone: the nav values of the
oracle's cells of a small scene, floor-division tile coordinates left of and below the anchor, a consumer that grows on the low
side, and the scene of tests/test_map_feed_gpu.py whose beams must change single cells in tile corners."""
import numpy as np
import pytest

import live_map_rule as rule
import map_feed_rule as mf
import occupancy_cases as oc
from test_edge_cases_oracle import run_oracle


def test_to_nav_on_the_oracles_cells(oracle_lib):
    case = next(oc.direction_cases())
    cells = run_oracle(case)[0][:, :case.width]
    assert set(np.unique(cells).tolist()) == {0, 100, 255}
    nav = mf.to_nav(cells)
    assert nav.dtype == np.int8 and nav.shape == cells.shape
    assert (nav[cells == 0] == -1).all() and (nav[cells == 100] == 100).all() and (nav[cells == 255] == 0).all()
    assert set(np.unique(nav).tolist()) == {-1, 0, 100}
    with pytest.raises(AssertionError):
        mf.to_nav(np.array([0, 100, 255, 1], dtype=np.uint8))


def test_tile_coordinates_are_floor_quotients():
    assert mf.tile_of([-17, -16, -1, 0, 15, 16]).tolist() == [-2, -1, -1, 0, 0, 1]
    old = np.full((64, 64), -1, dtype=np.int8)
    new = old.copy()
    new[0, 0] = 0            # lattice cell (-32, -48): tile (-2, -3)
    new[15, 31] = 100        # lattice cell (-1, -33): tile (-1, -3)
    new[16, 16] = 0          # lattice cell (-16, -32): tile (-1, -2)
    new[63, 63] = 0          # lattice cell (31, 15): tile (1, 0)
    assert mf.tiles_that_differ(old, new, -32, -48).tolist() == [[-2, -3], [-1, -3], [-1, -2], [1, 0]]
    assert mf.single_cell_tiles(old, new, -32, -48) == [(-2, -3, 0, 0), (-1, -3, 15, 15), (-1, -2, 0, 0), (1, 0, 15, 15)]
    with pytest.raises(AssertionError):
        mf.tiles_that_differ(old, new, -8, 0)


def test_equal_maps_have_no_tiles():
    nav = np.random.default_rng(1).choice(np.array([-1, 0, 100], dtype=np.int8), size=(32, 48))
    got = mf.tiles_that_differ(nav, nav.copy(), 64, -64)
    assert got.shape == (0, 2) and got.dtype == np.int32


def test_patch_after_a_growth_on_the_low_side():
    rng = np.random.default_rng(2)
    first = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(32, 32))
    consumer = mf.patch(None, (0, 0, 32, 32), mf.tiles_that_differ(np.full((32, 32), -1, dtype=np.int8), first, 0, 0),
                        [first[y:y + 16, x:x + 16] for y in (0, 16) for x in (0, 16)])
    assert np.array_equal(consumer[0], first)
    tile = np.full((16, 16), 100, dtype=np.int8)
    grown, win = mf.patch(consumer, (-64, -16, 128, 64), [[-4, -1], [0, 1]], [tile, tile])
    assert win == (-64, -16, 128, 64) and grown.shape == (64, 128)
    want = np.full((64, 128), -1, dtype=np.int8)
    want[16:48, 64:96] = first
    want[0:16, 0:16] = 100             # tile (-4, -1): the window's low corner
    want[32:48, 64:80] = 100           # tile (0, 1): over the old content
    assert np.array_equal(grown, want) and np.array_equal(consumer[0], first)
    with pytest.raises(AssertionError):
        mf.patch(consumer, (16, 0, 32, 32), [], [])


def test_corner_scene_changes_single_cells_in_tile_corners(oracle_lib):
    """the precondition of tests/test_map_feed_gpu.py::test_single_cells_in_tile_corners, from the oracle alone"""
    assert mf.corner_precondition() == ((0, 0, 15, 15), (-2, -1, 0, 0))
