"""GPU: a distance field that follows a live map (kh_live_map_field_*, LiveMap.field / MapField.sync) on the mappers of
tests/test_live_map_gpu.py: after every live update and sync the field is byte-equal to a fresh MapField of the live map's view, and
at the end of the run to tests/map_field_rule.py (the rule costs seconds at that size)."""
import numpy as np
import pytest

import map_field_rule as rule
import map_match_rule as mr
import test_live_map_gpu as lm
import test_localization_gpu as loc
from slam_toolbox_amd import capi
from slam_toolbox_amd.map_field import MapField

pytestmark = pytest.mark.gpu
NOTHING = dict(rebuilt=0, relayout=0, cells_box=(0, 0, 0, 0), values_box=(0, 0, 0, 0), cells_recomputed=0, cells_compared=0, times_ms=[0.0] * 4)


def same_as_fresh(field, live, max_distance, obstacles="occupied", what=""):
    fresh = MapField(live, max_distance=max_distance, obstacles=obstacles)
    i = live.info()
    for f in (field, fresh):
        assert (f.stats["ox"], f.stats["oy"], f.stats["width"], f.stats["height"]) == (i["ox"], i["oy"], i["width"], i["height"]), what
    d2 = field.d2
    assert np.array_equal(d2, fresh.d2), f"{what}: {int((d2 != fresh.d2).sum())} values differ from a fresh field"
    assert {k: field.stats[k] for k in ("n_obstacles", "n_far", "max_d2")} == {k: fresh.stats[k] for k in ("n_obstacles", "n_far", "max_d2")}, what
    fresh.close()
    return d2


def test_the_lap_queue(kartohip_lib, oracle_lib):
    """the lap queue at the default rebuild fraction, a sync after every live update of 25 accepted scans"""
    ranges, odom = loc._queue()
    m = lm._mapper()
    live = m.live_map(0.1, lm.ANCHOR)
    with pytest.raises(capi.KartoHipError) as e:
        live.field(max_distance=1.0)
    assert e.value.code == capi.KH_ERR_NOT_FOUND, "before the live map has a window"
    field, since, closures_then = None, 0, 0
    relayouts = behind_closure = partial = idle = 0
    for i in range(lm.SWITCH):
        since += int(m.Process(ranges[i], odom[i], 0.1 * i)[0])
        if since < 25 and i != lm.SWITCH - 1:
            continue
        live.update()
        if field is None:
            field = live.field(max_distance=1.0)
            assert field.stats["radius_cells"] == 10
            u = field.sync()
            assert u == NOTHING, "the field was made from this very window"
        else:
            u = field.sync()
        d2 = same_as_fresh(field, live, 1.0, what=f"queue scan {i}")
        info = live.info()
        window = (info["ox"], info["oy"], info["width"], info["height"])
        if u["relayout"]:
            assert u["rebuilt"] == 1 and u["values_box"] == window and u["cells_recomputed"] == window[2] * window[3]
        relayouts += u["relayout"]
        if m.stats()["loop_closures"] > closures_then:
            behind_closure += 1
            assert u["cells_compared"] > 0 or u["rebuilt"], "the closure's update handed nothing over"
        if u["rebuilt"] == 0 and 0 < u["cells_recomputed"] < window[2] * window[3]:
            partial += 1
            assert u["values_box"][2] * u["values_box"][3] == u["cells_recomputed"] and u["times_ms"][1] > 0 and u["times_ms"][2] > 0
        again = field.sync()
        assert again == NOTHING, "nothing pending, and something was launched"
        idle += 1
        since, closures_then = 0, m.stats()["loop_closures"]
    assert relayouts >= 1, "no sync saw the window grow"
    assert behind_closure >= 1, "no sync came behind a loop closure"
    assert partial >= 1, "no sync recomputed less than the window"
    assert idle >= 1
    view = mr.view_dict(live.cells(), info["anchor"], 1.0 / info["resolution"], info["ox"], info["oy"], info["width"])
    want = rule.d2_separable(view, 10)
    assert np.array_equal(d2, want) and {k: field.stats[k] for k in ("n_obstacles", "n_far", "max_d2")} == rule.stats(want)
    field.close(); live.close(); m.close()


def test_removal_and_two_fields_at_different_paces(kartohip_lib, oracle_lib):
    """every fifth node removed, then more: a field of R = 10 synced after every update, one of R = 4 under NOT_FREE after the second only"""
    m, _ = loc._build_map()
    live = m.live_map(0.1, lm.ANCHOR)
    live.update()
    often, seldom = live.field(max_distance=1.0), live.field(max_distance=0.4, obstacles="not_free")
    assert seldom.stats["radius_cells"] == 4
    same_as_fresh(often, live, 1.0, what="before")
    same_as_fresh(seldom, live, 0.4, "not_free", what="before")
    n = m.num_scans()
    for i in range(5, n - 2 * lm.BUFFER, 5):
        m.RemoveNode(i)
    assert live.update()["scans_removed"] > 0
    u = often.sync()
    assert u["cells_compared"] > 0
    same_as_fresh(often, live, 1.0, what="a fifth removed")
    for i in [int(k) for k in m.alive() if k < n - 2 * lm.BUFFER][::3]:
        m.RemoveNode(i)
    live.update()
    for field, distance, obstacles in ((seldom, 0.4, "not_free"), (often, 1.0, "occupied")):
        u = field.sync()
        assert u["cells_compared"] > 0
        same_as_fresh(field, live, distance, obstacles, what="more removed")
        assert field.sync() == NOTHING
    assert seldom.sync()["cells_compared"] == 0
    often.close(); seldom.close(); live.close(); m.close()


def test_lifetimes(kartohip_lib, oracle_lib):
    """the field destroyed before the live map, and after it: then it stays readable and its sync is refused"""
    m, _ = loc._build_map()
    live = m.live_map(0.1, lm.ANCHOR)
    live.update()
    first, second = live.field(max_distance=0.5), live.field(max_distance=0.5)
    first.close()                                              # detaches: the next update hands it nothing
    live.update()
    assert second.sync() == NOTHING
    want = second.d2
    plain = MapField(live, max_distance=0.5)
    with pytest.raises(capi.KartoHipError) as e:
        plain.sync()
    assert e.value.code == capi.KH_ERR_INVALID_ARG, "a field that is not attached"
    assert np.array_equal(plain.d2, want)
    plain.close()
    live.close()
    with pytest.raises(capi.KartoHipError) as e:
        second.sync()
    assert e.value.code == capi.KH_ERR_INVALID_ARG, "the live map is gone"
    assert np.array_equal(second.d2, want) and second.costs(inscribed_radius=0.2, inflation_radius=0.5).shape == want.shape
    second.close(); m.close()
