"""The launch scripts of the three Co-ES engines against tests/golden/es_launch_scripts.json, which was minted when
ESEngine.update_device and DQNESEngine.generation each still wrote the update sequence out and DQNESEngine built its own game
table (tests/golden/make_golden_launches.py, whose driver this test replays): every entry point, in order, with every argument,
the calls on the two rollout objects and the tables they are constructed with, the gather callbacks with their kind, torch's
copy_ / fill_ / div_ and indexed assignments into the engine's tensors, and the evaluation graph's capture and replays.  On the
CPU, with the built library."""
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope="module")
def driver(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_launches", os.path.join(golden_dir, "make_golden_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want(driver):
    assert os.path.getsize(driver.ES_FIXTURE) < 1 << 20
    with open(driver.ES_FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def got(driver):
    return driver.mint_es()


def test_the_fixture_holds_every_case_of_the_driver(driver, want):
    assert sorted(want) == sorted(driver.ES_CASES) and len(want) == 19
    assert not set(driver.ES_CASES) & set(driver.CASES)
    entry_points = {rec[1] for recs in want.values() for rec in recs if rec[0] == "call"}
    for name in ("coevo_fc_perturb_flags", "coevo_fc_distance", "coevo_sharing_score", "coevo_centered_ranks",
                 "coevo_es_partial", "coevo_es_apply",
                 "coevo_fc16_perturb_dist", "coevo_fc16_distance", "coevo_fc16_distance_finalize",
                 "coevo_es16_fitness", "coevo_es16_partial", "coevo_es16_apply",
                 "coevo_dqn_perturb", "coevo_fc_distance_finalize", "coevo_dqn_es_partial", "coevo_dqn_es_apply",
                 "coevo_dqn_relayout"):
        assert name in entry_points, name
    gathers = {rec[1] for recs in want.values() for rec in recs if rec[0] == "gather"}
    assert gathers == {"stats", "partials"}
    kinds = {rec[0] for recs in want.values() for rec in recs}
    assert kinds == {"call", "ro", "eval_ro", "ro.new", "plan.new", "upload", "gather", "torch", "setitem", "graph.capture",
                     "graph.replay"}
    # the evaluation graph: captured once and replayed every generation where it is on, absent where it is off
    for case, recs in want.items():
        if case.startswith("dqn_es"):
            on = case not in ("dqn_es_eval_eager", "dqn_es_host_frames") and "shard" not in case
            assert [r[0] for r in recs if r[0].startswith("graph")] == (["graph.capture", "graph.replay", "graph.replay"]
                                                                         if on else []), case
    # both rollout classes of every engine family were constructed, each engine's training rollout before its evaluation one
    classes = {x for recs in want.values() for rec in recs if rec[0] == "ro.new" for x in rec[2:4] if isinstance(x, str)}
    assert {"DeviceRollout", "HostEnvRollout", "SynthRollout", "HostFrameRollout"} <= classes
    for case, recs in want.items():
        assert [rec[1] for rec in recs if rec[0] == "ro.new"] == ["ro", "eval_ro"], case


def test_the_driver_puts_back_what_it_replaced(driver, got):
    import torch
    from coevonet_amd import dqn_population, lib as L, population, rollout
    assert L.call.__module__ == L.__name__ and L._p.__module__ == L.__name__
    assert rollout.HostEnvRollout.reset_from_ordinals.__module__ == rollout.__name__
    assert "reset_from_ordinals" not in vars(rollout.DeviceRollout)
    assert dqn_population.HostFrameRollout.enqueue.__module__ == dqn_population.__name__
    assert population.captured.__module__ == population.__name__ and dqn_population.captured is population.captured
    assert "__setitem__" not in vars(torch.Tensor) and "div_" not in vars(torch.Tensor)


def _cases():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "es_launch_scripts.json")) as f:
        return sorted(json.load(f)["cases"])


@pytest.mark.parametrize("case", _cases())
def test_launch_script_equals_the_one_recorded_before_the_update_was_shared(got, want, case):
    g, w = got[case], want[case]
    for i, (a, b) in enumerate(zip(g, w)):
        assert a == b, f"{case}: record {i} differs"
    assert len(g) == len(w), f"{case}: {len(g)} records, the fixture has {len(w)}"
