"""The launch scripts of the four Co-GA engines against tests/golden/ga_launch_scripts.json, which was minted when every engine
still wrote its generation tail out on its own (tests/golden/make_golden_launches.py, whose driver this test replays): every
entry point, in order, with every argument - pointers resolved to "<engine attribute>+<byte offset>", ctypes structures field
by field - and the calls on the rollout object, the gather callbacks and torch's copy_ / fill_ into the engine's tensors between
them.  On the CPU, with the built library."""
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
    with open(driver.FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def got(driver):
    return driver.mint()


def test_the_fixture_holds_every_case_of_the_driver(driver, want):
    assert sorted(want) == sorted(driver.CASES) and len(want) == 20
    entry_points = {rec[1] for recs in want.values() for rec in recs if rec[0] == "call"}
    # every form of the tail is in there: fused and launch-per-step selection and promotion, the elite rebuild of a shard, the
    # packed exchange, the multi-role children, both float16 engines (coevo_ga_promote_tick closes the pipelined loop's tail
    # only, which the GPU tests carry)
    for name in ("coevo_ga_select", "coevo_ga_select_adapt", "coevo_sharing_score", "coevo_ga_promote",
                 "coevo_ga_promote_rebuild", "coevo_fc_rebuild_elites", "coevo_fc_perturb", "coevo_fc_perturb_dist",
                 "coevo_fc_perturb_dist_multi", "coevo_fc_distance_finalize_multi_tick", "coevo_gather_f32",
                 "coevo_ga16_promote", "coevo_fc16_perturb_dist", "coevo_dqn_perturb", "coevo_dqn16_perturb_dist",
                 "coevo_dqn16_distance", "coevo_fc16_distance_finalize", "coevo_net_gather", "coevo_counter_add"):
        assert name in entry_points, name
    kinds = {rec[0] for recs in want.values() for rec in recs}
    assert kinds == {"call", "ro", "ro.new", "upload", "gather", "gather_packed", "torch"}


def test_the_driver_puts_back_what_it_replaced(driver, got):
    import torch
    from coevonet_amd import lib as L, population, rollout
    assert L.call.__module__ == L.__name__ and L._p.__module__ == L.__name__
    assert rollout.DeviceRollout.enqueue.__module__ == rollout.__name__
    assert population.SlabIO.upload.__module__ == population.__name__
    assert torch.cuda.synchronize.__module__ == "torch.cuda" and "collect_stamps" not in vars(rollout.HostEnvRollout)


def _cases():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "ga_launch_scripts.json")) as f:
        return sorted(json.load(f)["cases"])


@pytest.mark.parametrize("case", _cases())
def test_launch_script_equals_the_one_recorded_before_the_tail_was_shared(got, want, case):
    g, w = got[case], want[case]
    for i, (a, b) in enumerate(zip(g, w)):
        assert a == b, f"{case}: record {i} differs"
    assert len(g) == len(w), f"{case}: {len(g)} records, the fixture has {len(w)}"
