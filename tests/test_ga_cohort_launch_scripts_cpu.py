"""The launch scripts of GAEngine's cohort breeding and resets (_breed_cohort / _reset_cohort, what a cohort's stream is handed in
the pipelined loops), of its selection under hof_mean / population_sharing (_select_shared) and of HalfGAEngine's multi-role
breeding against tests/golden/ga_cohort_launch_scripts.json, which was minted before population.co_ga_reset_segments, the
shared job-array builder and the engine's declared state existed (tests/golden/make_golden_launches.py, whose driver this test
replays).  Records as in test_ga_launch_scripts_cpu.py.  On the CPU, with the built library.

The stubbed RolloutPlan builds every shape the cases ask for (it keeps only n_games), so the cohort counts and bounds are the
ones named: the driver asserts them."""
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
    with open(driver.COHORT_FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def got(driver):
    return driver.mint_cohorts()


def _calls(recs, name):
    return [rec for rec in recs if rec[:2] == ["call", name]]


def test_the_fixture_holds_every_case_of_the_driver_and_every_branch(driver, want):
    assert sorted(want) == sorted(driver.COHORT_CASES) and len(want) == 10
    entry_points = {rec[1] for recs in want.values() for rec in recs if rec[0] == "call"}
    for name in ("coevo_fc_perturb_dist_multi", "coevo_fc_distance_finalize_multi", "coevo_fc_distance_finalize_multi_tick",
                 "coevo_counter_add", "coevo_fc16_perturb_dist_multi", "coevo_fc16_distance_finalize_multi",
                 "coevo_fc_pairwise_distance", "coevo_niche_counts", "coevo_ga_fitness_shared", "coevo_sharing_score"):
        assert name in entry_points, name
    # the evaluation segment: only with the last cohort and only from generation 1 on
    resets = [rec for rec in want["ga_cohorts_2_of_6"] if rec[:2] == ["ro", "reset_segments"]]
    assert [(rec[3]["arm"][0], len(rec[2])) for rec in resets] == [(1, 3), (0, 3), (1, 4), (0, 3), (1, 4), (0, 3)]
    # cohort 0 holds individual 0: its first child is child 0 (the clamp) and the best's distance heads the reduction
    jobs = [rec[2][0] for rec in _calls(want["ga_cohorts_2_of_6"], "coevo_fc_perturb_dist_multi")]
    assert [(j["child_first"], j["n_children"]) for j in jobs] == [(3, 3), (1, 2)] * 2
    heads = [rec[2][0]["head"] for rec in _calls(want["ga_cohorts_2_of_6"], "coevo_fc_distance_finalize_multi")]
    assert heads == [None, "best_dist[agent_0]+0"] * 2
    # a cohort that holds only the unchanged best: no breeding launch, the distance copied, the counter ticked on its own
    best = want["ga_cohorts_only_the_best_from_counter"]
    assert len(_calls(best, "coevo_counter_add")) == 3 and len(_calls(best, "coevo_fc_perturb_dist_multi")) == 3
    assert sum(rec[:2] == ["torch", "copy_"] for rec in best) == 9
    # the shard's offset: rank 1 of 2 resets games 0.. of its own table under the ordinals of individuals 6..
    first = [rec for rec in want["ga_cohorts_shard_1_of_2"] if rec[:2] == ["ro", "reset_segments"]][1]
    assert first[2][0] == [0, 6, 1 + 6 * 2] and first[3]["arm"][0] == 0
    # the second generation of the sharing modes finds the stale-agent distances current
    for case in ("ga_host_hof_mean", "ga_host_population_sharing", "ga_host_hof_mean_population_sharing"):
        assert len(_calls(want[case], "coevo_fc_distance")) == 3 and len(_calls(want[case], "coevo_rank_desc")) == 6


def _cases():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "ga_cohort_launch_scripts.json")) as f:
        return sorted(json.load(f)["cases"])


@pytest.mark.parametrize("case", _cases())
def test_launch_script_equals_the_one_recorded_before_the_engine_wrote_these_once(got, want, case):
    g, w = got[case], want[case]
    for i, (a, b) in enumerate(zip(g, w)):
        assert a == b, f"{case}: record {i} differs"
    assert len(g) == len(w), f"{case}: {len(g)} records, the fixture has {len(w)}"
