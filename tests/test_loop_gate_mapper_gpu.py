"""GPU: the covariance gate of the mapper's loop search (kh_mapper_set_loop_gate) on a lap queue of 260 scans
that closes loops under the default parameters.

  * null parameters -- chi2_position = 0 with chi2_jump = 0, and covariance_scale = 0 with chi2_jump = 1e300 -- leave the run as it
    is: the solver-call log is line-identical to the plain run's
  * chi2_jump = 1e-300 rejects every chain that passes the fine match: no closure, and the rejections are counted
  * with the defaults the run completes, the column passes are the refreshes tests/loop_gate_rule.column_passes predicts from the
    run's own log (refresh_scans 1 and 10), no semi-axis exceeds max_reach, and a saved and loaded mapper has the gate off"""
import numpy as np
import pytest

import loop_gate_rule as rule
from slam_toolbox_amd import synth

pytestmark = pytest.mark.gpu
N_SCANS = 260


def _lines(path):
    with open(path) as f:
        return [" ".join(l.split()[:2]) if l.startswith("X ") else l.rstrip("\n") for l in f if not l.startswith("Z ")]


@pytest.fixture(scope="module")
def queue():
    world = synth.make_world(12345)
    truth, odom = synth.trajectory_laps(N_SCANS)
    rng = np.random.default_rng(4)
    return np.ascontiguousarray(np.stack([synth.make_scan(world, truth[i], rng) for i in range(N_SCANS)])), np.ascontiguousarray(odom)


def run(queue, log, gate=None, keep=False):
    from slam_toolbox_amd.mapper import Mapper
    ranges, odom = queue
    m = Mapper(synth.Laser(), log_path=log)
    if gate is not None:
        m.SetLoopGate(True, **gate)
    for i in range(N_SCANS):
        m.Process(ranges[i], odom[i], 0.1 * i)
    out = dict(stats=m.stats(), gate=m.loop_gate_stats(), params=m.loop_gate(), poses=m.poses())
    m.set_log(None)
    out["log"] = _lines(log)
    if keep:
        return out, m
    m.close()
    return out


@pytest.fixture(scope="module")
def plain(kartohip_lib, queue, tmp_path_factory):
    out = run(queue, str(tmp_path_factory.mktemp("gate") / "plain.log"))
    assert out["stats"]["loop_closures"] > 0, "the queue closes no loop under the default parameters"
    assert out["params"]["enabled"] == 0 and out["gate"]["column_passes"] == 0
    return out


@pytest.mark.parametrize("gate", [dict(chi2_position=0.0, chi2_jump=0.0), dict(covariance_scale=0.0, chi2_jump=1e300)],
                         ids=["chi2 = 0", "covariance_scale = 0"])
def test_null_parameters_leave_the_run_as_it_is(plain, queue, tmp_path, gate):
    got = run(queue, str(tmp_path / "null.log"), gate)
    assert got["params"]["enabled"] == 1
    for k, (a, b) in enumerate(zip(plain["log"], got["log"])):
        assert a == b, f"solver-call logs diverge at line {k}:\n  plain: {a}\n  gated: {b}"
    assert len(plain["log"]) == len(got["log"])
    assert np.array_equal(plain["poses"], got["poses"])
    assert got["gate"]["jump_rejected"] == 0 and got["gate"]["column_passes"] == 0
    assert got["stats"]["loop_closures"] == plain["stats"]["loop_closures"]


def test_a_jump_bound_nothing_meets_rejects_every_closure(plain, queue, tmp_path):
    got = run(queue, str(tmp_path / "jump.log"), dict(chi2_jump=1e-300))
    print(f"[loop gate] chi2_jump 1e-300: {got['gate']}")
    assert got["stats"]["loop_closures"] == 0 and got["gate"]["jump_rejected"] > 0
    assert not any(l.startswith("X ") for l in got["log"])


@pytest.mark.parametrize("refresh_scans", [1, 10])
def test_defaults_refresh_as_the_rule_predicts(plain, queue, tmp_path, refresh_scans):
    from slam_toolbox_amd.mapper import Mapper
    got, m = run(queue, str(tmp_path / "gated.log"), dict(refresh_scans=refresh_scans), keep=True)
    g, p = got["gate"], got["params"]
    print(f"[loop gate] defaults, refresh_scans {refresh_scans}: {g}, closures {got['stats']['loop_closures']} (plain {plain['stats']['loop_closures']})")
    assert p["enabled"] == 1 and p["refresh_scans"] == refresh_scans and p["max_reach"] == 3.0 + 8.0 / 2
    assert got["stats"]["scans_processed"] == plain["stats"]["scans_processed"] and np.isfinite(got["poses"]).all()
    assert g["ungated_searches"] == 0
    assert g["column_passes"] == rule.column_passes(got["log"], refresh_scans)
    assert g["column_passes"] > 0 and g["column_ms"] > 0.0
    assert 3.0 < g["max_semi_axis"] <= p["max_reach"]
    path = str(tmp_path / "session.khms")
    m.save(path)
    m.close()
    loaded = Mapper.load(path)
    assert loaded.loop_gate()["enabled"] == 0 and loaded.loop_gate_stats()["column_passes"] == 0
    loaded.close()
